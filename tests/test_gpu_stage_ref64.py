"""Each fp32 stage against a float64 restatement of that stage alone (tests/stage_ref64.py), fed the GPU's own input to the
stage (the debug taps), at a frame count in every bucket of every launch form the fp32 path picks -- and at full size for the
one-launch attention layer.

Launch forms by chunk size Nc = round_up(N, 128) and CU count (lstm.hip launch_time_any, attn.hip sdfa_launch_attn_key_score /
sdfa_attn_fuses_tail):
  time LSTM    time_lstm_split16_kernel while Nc / 4 <= CUs; time_lstm_split_kernel<2> while Nc / 8 <= CUs;
               time_lstm_kernel<1> below 8192; time_lstm_kernel<2> from 8192
  attention    attn_key_score_f32_kernel + attn_kernel<true> (units of 64 >> ts_shift time steps) while Nc / 16 < CUs - CUs / 8;
               attn_fused_f32_kernel (one launch) from there

Bounds are on max|gpu - ref| / max|ref| of a stage, over every frame of every size.  A bug confined to some frames (a stale
tile, a unit boundary, the padded tail) or to one step of a recurrence shows at that scale; the sensitivity controls at the
bottom show that it does.

The debug_keep engine swaps the fused conv stack and the share-map recurrence for their unfused forms, and keeps layer 1 of the
BiLSTM on the projection GEMM + time_lstm_kernel pair: the shipping engine's layer 1 contracts its input projection inside the
recurrence (time_lstm_fused_kernel<1> / <2>, lstm.hip sdfa_time_lstm_fuses_x) wherever one workgroup per tile fills the last round
of the CUs to 93 % -- at 8,192 frames among others -- so the float64 comparison of the taps never runs that kernel itself.  Every
size here is also run through the shipping engine, which must give the same bits; that comparison is what covers it.

The offsets head (three FCs to 59 coefficients, the PCA expansion to 15,069 columns) is checked at the same sizes by the section at
the bottom: its coefficients and rows against float64, the ragged last column tile, rows written through a 4-byte-aligned output
pointer, and the fp32 GEMM variants bitwise.

`python tests/test_gpu_stage_ref64.py` prints the measured errors per stage and size (how the bounds below were set);
`python tests/test_gpu_stage_ref64.py offsets` those of the offsets head.
"""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "..", "oracle"), os.path.join(_HERE, "..", "sdfa-2019_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from stage_ref64 import StageRef64                                               # noqa: E402

pytestmark = pytest.mark.gpu

# max|gpu - ref| / max|ref| per stage, over every size, the front-end batch and (z, align) the full-size run; each bound is at
# most 4x the largest value measured on an MI355X (256 CUs), written next to it.  The frequency stage is the largest: its
# Linear(8192 -> 256) sums 8,192 fp32 products per output (about sqrt(8192) x 6e-8 relative), with no dependence on frame position.
BOUNDS = {
    "conv3": 2e-6,       # 5.7e-7
    "freq": 1e-5,        # 6.6e-6
    "bilstm": 5e-6,      # 1.8e-6
    "z": 3e-6,           # 1.0e-6 (full size; 8.8e-7 over the sizes)
    "align": 1e-5,       # 5.8e-6 (full size; 4.6e-6 over the sizes)
    "coef": 5e-6,        # 1.4e-6
    "rows": 4e-6,        # 1.1e-6
}
FULL = 8192          # max_frames of both engines: every size below runs in one chunk


def round_up(n, m=128):
    return -(-n // m) * m


def time_lstm_form(nc, cus):
    """The kernel launch_time_any runs for an fp32 chunk of nc frames (no CUs reserved)."""
    if nc // 4 <= cus:
        return "time_lstm_split16_kernel"
    if nc // 8 <= cus:
        return "time_lstm_split_kernel<2>"
    return "time_lstm_kernel<2>" if (nc // 64) * 2 >= 256 else "time_lstm_kernel<1>"


def attention_form(nc, cus):
    """The fp32 attention layer's kernels for a chunk of nc frames: the one-launch form, or the two-kernel form and its ts_shift."""
    if nc // 16 >= cus - cus // 8:
        return "attn_fused_f32_kernel"
    ts = 0
    while ts < 3 and ((nc // 16) << ts) < 2 * cus:
        ts += 1
    return f"attn_key_score_f32_kernel+attn_kernel<true> ts_shift={ts}"


# The launch choices of the mixed-precision modes (tests/test_gpu_stage_mixed_ref64.py), restated from the launch code.
# api_forward.cpp stage_terms: bf16 terms per operand of the (body, attention, regressor) contractions; 0 = that stage's fp32 kernels.
MIXED_TERMS = {"bf16x3": (3, 3, 3), "bf16x6": (6, 6, 6), "bf16x3_attention": (0, 3, 0), "bf16": (1, 1, 1)}
PCA_TRIANGLE_BLOCKS = 312      # pca.hip: (29,928 rotation columns + 95) / 96


def split_gemm_form(terms, ppad, qpad, cus):
    """gemm.hip launch_any with GemmArgs.terms set: the 256 x 256 tile where it divides the problem and gives at least half the
    CUs a tile, else the 128 x 128 one.  (K is a multiple of 16 in every GEMM of the model, as the six-product big tile asks.)"""
    big = ppad % 256 == 0 and qpad % 256 == 0 and (ppad // 256) * (qpad // 256) * 2 >= cus
    if terms == 6:
        return "gemm_bf16x6_big_kernel" if big else "gemm_bf16x6_kernel"
    return f"gemm_bf16_big_kernel<{terms}>" if big else f"gemm_bf16_kernel<{terms}>"


def key_score_ts_shift(nc, cus):
    """attn.hip sdfa_launch_attn_key_score: a work unit is 16 frames x (64 >> ts_shift) time steps."""
    ts = 0
    while ts < 3 and ((nc // 16) << ts) < 2 * cus:
        ts += 1
    return ts


def mixed_forms(mode, nc, cus):
    """stage -> the kernels a chunk of nc frames launches for it in a mixed-precision mode of the dgrad model; only the stages
    that run kernels of the mode's own (an fp32 stage of such a mode is the arithmetic test_stage_against_float64 covers).
      conv3    conv123_bf16_kernel at every size (conv.hip)
      freq     lstm.hip launch_freq_bf16: one persistent workgroup per CU pulling 2 nc 64-column tiles from a queue -- one round of
               the queue, or several -- then the Linear(8192 -> 256) as a split GEMM over Mc = 64 nc columns
      bilstm   the input projections (2048 x Mc) as split GEMMs; lstm.hip launch_time_any / time_big: 64-frame tiles from
               (nc / 64) * 2 >= 256 workgroups on, except in the six-product mode (three planes of h: 32-frame tiles only)
      z        the query Conv1d (512 x nc) and projection (128 x nc) as split GEMMs, then attn_key_score_kernel<terms> +
               attn_kernel<true> at the ts_shift of the size; sdfa_attn_fuses_tail never applies at 1 or 3 terms.  The six-product
               mode runs the fp32 key-score / one-launch kernels behind its query GEMMs.
      coef     the regressor's FCs (512, 256 and 128 padded rows x nc) as split GEMMs
      rows     bf16x3 only: pca_dgrad_res_kernel<true>, whose work units are `fbu` 128-frame blocks of one triangle block; the last
               unit of a triangle block is partial unless fbu divides nc / 128.  (fbu itself is a trip count: 129 frames already
               run two frame blocks in one unit.)"""
    body, attn, regr = MIXED_TERMS[mode]
    mc = 64 * nc
    f = {}
    if body:
        f["conv3"] = "conv123_bf16_kernel"
        if body == 1:
            lstm = "freq_lstm_bf16_kernel<1>"
        else:
            lstm = f"freq_lstm_bf16p_v3_kernel<persistent, {3 if body == 6 else 2} planes>, " + \
                   ("one round of the tile queue" if 2 * nc <= cus else "several rounds of the tile queue")
        f["freq"] = lstm + " + " + split_gemm_form(body, 256, mc, cus)
        nt = 1 if body == 6 or (nc // 64) * 2 < 256 else 2
        f["bilstm"] = split_gemm_form(body, 2048, mc, cus) + f" + time_lstm_bf16_kernel<{nt},{body}>"
    if attn:
        f["z"] = split_gemm_form(attn, 512, nc, cus) + " + " + split_gemm_form(attn, 128, nc, cus) + " + " + \
                 ("the fp32 attention kernels" if attn == 6 else f"attn_key_score_kernel<{attn}>+attn_kernel<true> ts_shift={key_score_ts_shift(nc, cus)}")
    if regr:
        f["coef"] = " + ".join(sorted({split_gemm_form(regr, p, nc, cus) for p in (512, 256, 128)}))
    if mode == "bf16x3":
        nfb = nc // 128
        fbu = 16 if PCA_TRIANGLE_BLOCKS * ((nfb + 15) // 16) >= 4 * cus else 8 if PCA_TRIANGLE_BLOCKS * ((nfb + 7) // 8) >= 4 * cus else 4
        f["rows"] = "pca_dgrad_res_kernel<true>, " + ("last unit partial" if nfb % fbu else "whole units")
    return f


def offsets_expand_form(mode, nc, cus):
    """The offsets head's PCA expansion in a split mode: a GEMM of nc rows by 15,104 = 59 x 256 padded columns (api_forward.cpp expand_rows)."""
    return split_gemm_form(MIXED_TERMS[mode][2], nc, 15104, cus)


def sizes_for(cus):
    """1, 17 and 129 (a short clip, ragged tiles), 8191 and 8192 (time_lstm_kernel<2>, ragged and whole) and, for every edge
    between the forms that depend on the CU count, the largest frame count at or below it and the smallest above it."""
    edges = {4 * cus // 128 * 128, 8 * cus // 128 * 128, round_up(16 * (cus - cus // 8)) - 128}
    out = {1, 17, 129, 8191, 8192}
    for e in edges:
        if 128 <= e < FULL:
            out |= {e, e + 1}
    return sorted(out)


def sampled_frames(n, k=32):
    """First, last, the 16- and 128-frame tile edges, the real frames of the last (padded) 128-frame tile, then evenly spread."""
    pick = {0, n - 1, 15, 16, 127, 128}
    tail0 = (n - 1) // 128 * 128
    pick |= set(range(max(tail0, n - 16), n))
    pick = {f for f in pick if 0 <= f < n}
    spread = k
    while len(pick) < min(k, n):
        pick |= set(np.linspace(0, n - 1, spread).astype(int).tolist())
        spread += 1
    return np.array(sorted(pick), np.int64)


def edge_mask(frames, n):
    """Frames at a 16-frame unit edge or in the padded last 128-frame tile: where a position-dependent bug would show."""
    frames = np.asarray(frames)
    tail = (frames >= (n - 1) // 128 * 128) if n % 128 else np.zeros(len(frames), bool)
    return (frames % 16 == 0) | (frames % 16 == 15) | tail


def frame_err(got, ref):
    """(max |got - ref| per frame, max |ref|)"""
    return (got.double() - ref).abs().flatten(1).amax(1).cpu().numpy(), float(ref.abs().max())


class Stages:
    """Per-frame errors of every stage of one size, plus the bitwise comparisons with the shipping engine."""

    def __init__(self, n):
        self.n = n
        self.err = {}           # stage -> (frames, per-frame abs err, max|ref|)
        self.mismatch = []      # what differed from the shipping engine

    def add(self, stage, frames, err, refmax):
        if stage in self.err:
            f0, e0, r0 = self.err[stage]
            frames, err, refmax = np.concatenate([f0, frames]), np.concatenate([e0, err]), max(r0, refmax)
        self.err[stage] = (np.asarray(frames), np.asarray(err), refmax)

    def rel(self, stage, mask=None):
        frames, err, refmax = self.err[stage]
        if mask is not None:
            m = mask(frames)
            err = err[m] if m.any() else np.zeros(1)
        return float(err.max()) / refmax


def run_size(ref, keep, ship, feat, spk, table=None):
    """Both engines on `feat` (one chunk); every stage of the debug_keep run against the float64 stage fed the previous tap."""
    n = feat.shape[0]
    st = Stages(n)
    z, align = keep.encoder(feat)
    coef, rows = keep.regress(z, spk, want_coef=True)
    taps = {k: keep.tap(k, n) for k in (1, 2, 3)}
    for name, args in (("plain", {}), ("table", table)):
        if args is None:
            continue
        z2, a2 = ship.encoder(feat, **args)
        c2, r2 = ship.regress(z2, spk, want_coef=True)
        for what, a, b in (("z", z, z2), ("align", align, a2), ("coef", coef, c2), ("rows", rows, r2)):
            if not torch.equal(a, b):
                st.mismatch.append(f"{name}:{what}")
        del z2, a2, c2, r2
    fr = sampled_frames(n)
    fi = torch.from_numpy(fr).to(feat.device)
    st.add("conv3", fr, *frame_err(taps[1][fi], ref.conv_stack(feat[fi])))
    st.add("freq", np.arange(n), *frame_err(taps[2], ref.freq(taps[1])))
    st.add("bilstm", np.arange(n), *frame_err(taps[3], ref.bilstm(taps[2])))
    zr, ar = ref.attention(taps[3])
    st.add("z", np.arange(n), *frame_err(z, zr))
    st.add("align", np.arange(n), *frame_err(align, ar))
    st.add("coef", np.arange(n), *frame_err(coef, ref.regress(z, spk)))
    for f0 in range(0, n, 1024):
        sl = slice(f0, min(n, f0 + 1024))
        st.add("rows", np.arange(sl.start, sl.stop), *frame_err(rows[sl], ref.expand(coef[sl])))
    keep_host = dict(tap2=taps[2][:32].cpu(), tap3=taps[3][:32].cpu(), z=z[:32].cpu(), coef=coef[:32].cpu(), rows=rows[:32].cpu())
    return st, keep_host


def random_batch(n, seed):
    rs = np.random.RandomState(seed)
    feat = torch.from_numpy(rs.uniform(0, 1, (n, 64, 128, 3)).astype(np.float32)).cuda()
    spk = torch.from_numpy(rs.permutation(np.arange(n) % 8)).cuda()
    return feat, spk


def measure(sd):
    """Every size of sizes_for(CUs), random features and mixed speakers; one front-end batch with its frame table."""
    from sdfa_amd import synth
    from sdfa_amd.engine import Engine
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ref = StageRef64(sd, device="cuda:0")
    keep = Engine(sd, max_frames=FULL, debug_keep=True)
    ship = Engine(sd, max_frames=FULL)
    out = dict(cus=cus, sizes={}, host=None)
    for n in sizes_for(cus):
        feat, spk = random_batch(n, 7000 + n)
        out["sizes"][n], host = run_size(ref, keep, ship, feat, spk)
        if n == 129:
            out["host"] = host
        del feat, spk
    # real front-end features: speechlike and sweep clips of several lengths, at 16 kHz, with the frame table (column sharing)
    pcms = [synth.make_pcm(c, L, kind) for c, (L, kind) in enumerate([(48000, "speechlike"), (32000, "sweep"), (40000, "speechlike"),
                                                                      (24000, "sweep"), (56000, "speechlike"), (36000, "sweep")])]
    feat, _, _ = ship.mel_frontend(pcms, 16000)
    fc, fs, hop = ship.last_frame_table
    spk = torch.arange(feat.shape[0], device="cuda:0") % 8
    out["frontend"], _ = run_size(ref, keep, ship, feat, spk, table=dict(frame_clip=fc, frame_start=fs, hop=hop))
    out["forms"] = {n: (time_lstm_form(round_up(n), cus), attention_form(round_up(n), cus)) for n in out["sizes"]}
    return out


@pytest.fixture(scope="module")
def measured(synth_sd):
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    out = measure(synth_sd["dgrad"])
    torch.cuda.synchronize()
    out["seconds"] = time.time() - t0
    out["peak_bytes"] = torch.cuda.max_memory_allocated()
    return out


def table(out):
    """Per stage and size: max relative error over all frames, over edge / padded-tail frames, over the rest."""
    lines = [f"CUs {out['cus']}  ({out.get('seconds', 0):.0f} s, peak {out.get('peak_bytes', 0) / 2**30:.1f} GiB)"]
    runs = list(out["sizes"].items()) + [("frontend", out["frontend"])]
    for stage in BOUNDS:
        for n, st in runs:
            nn = st.n
            lines.append(f"{stage:7s} {str(n):>8s}  all {st.rel(stage):.2e}  edge {st.rel(stage, lambda f: edge_mask(f, nn)):.2e}  "
                         f"rest {st.rel(stage, lambda f: ~edge_mask(f, nn)):.2e}")
    return "\n".join(lines)


def test_sizes_hit_every_launch_form(measured):
    cus = measured["cus"]
    forms = measured["forms"]
    lstm = {f[0] for f in forms.values()}
    attn = {f[1] for f in forms.values()}
    every_lstm = {time_lstm_form(nc, cus) for nc in range(128, FULL + 1, 128)}
    every_attn = {attention_form(nc, cus) for nc in range(128, FULL + 1, 128)}
    assert lstm == every_lstm and attn == every_attn, (forms, every_lstm, every_attn)
    if cus == 256:
        assert sorted(forms) == [1, 17, 129, 1024, 1025, 2048, 2049, 3456, 3457, 8191, 8192]
    print("\n" + "\n".join(f"{n:5d}  {a}  {b}" for n, (a, b) in sorted(forms.items())))


def test_debug_keep_engine_gives_the_shipping_bits(measured):
    """z, align, coef and rows of the debug_keep engine (unfused conv, unshared recurrence) equal the default engine's, at every
    size; for the front-end batch also through the frame table (share map, shared layer-0 projection)."""
    bad = {n: st.mismatch for n, st in list(measured["sizes"].items()) + [("frontend", measured["frontend"])] if st.mismatch}
    assert not bad, bad


@pytest.mark.parametrize("stage", list(BOUNDS))
def test_stage_against_float64(measured, stage):
    print("\n" + table(measured))
    worst = {n: measured["sizes"][n].rel(stage) for n in measured["sizes"]}
    worst["frontend"] = measured["frontend"].rel(stage)
    assert max(worst.values()) <= BOUNDS[stage], (stage, worst)


# ---------------------------------------------------------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def full_size(synth_sd):
    """The 32 x 10 s batch of tests/test_gpu_fullsize.py (20,352 frames): one multi-chunk call of the shipping engine, and the
    same frames as three single-chunk debug_keep calls."""
    from sdfa_amd import synth
    from sdfa_amd.engine import Engine
    sd = synth_sd["dgrad"]
    L = 160000
    ship = Engine(sd, max_frames=FULL)
    pcms = [synth.make_pcm(c, L) for c in range(30)] + [synth.make_pcm(3, L), np.zeros(L, np.float32)]
    feat, _, _ = ship.mel_frontend(pcms, 16000)
    n = feat.shape[0]
    spk = torch.arange(n, device="cuda:0") % 8
    z, align = ship.encoder(feat)
    _, rows = ship.regress(z, spk)
    del ship
    keep = Engine(sd, max_frames=FULL, debug_keep=True)
    ref = StageRef64(sd, device="cuda:0")
    out = dict(n=n, equal=[], z=Stages(n), align=None)
    for f0 in range(0, n, FULL):
        sl = slice(f0, min(n, f0 + FULL))
        zk, ak = keep.encoder(feat[sl])
        _, rk = keep.regress(zk, spk[sl])
        out["equal"].append((torch.equal(zk, z[sl]), torch.equal(ak, align[sl]), torch.equal(rk, rows[sl])))
        del rk
        zr, ar = ref.attention(keep.tap(3, sl.stop - sl.start))
        out["z"].add("z", np.arange(sl.start, sl.stop), *frame_err(zk, zr))
        out["z"].add("align", np.arange(sl.start, sl.stop), *frame_err(ak, ar))
    return out


def test_full_size_single_chunk_calls_give_the_multi_chunk_bits(full_size):
    assert full_size["n"] == 20352
    assert full_size["equal"] == [(True, True, True)] * 3, full_size["equal"]


def test_full_size_one_launch_attention_against_float64(full_size):
    """All 20,352 frames' z and attention weights against the float64 attention of the BiLSTM output the kernel read."""
    st = full_size["z"]
    print(f"\nfull size: z {st.rel('z'):.2e}  align {st.rel('align'):.2e}  (peak device memory so far {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB)")
    assert st.rel("z") <= BOUNDS["z"] and st.rel("align") <= BOUNDS["align"]


# ------------------------------------------------------------------------------------------------------ sensitivity controls
def test_bounds_catch_a_stale_attention_tile(measured, synth_sd):
    """One 16-frame unit reading time step t+1 in place of t: the GPU's z misses that reference by more than the bound."""
    h = measured["host"]
    ref = StageRef64(synth_sd["dgrad"])
    good, _ = ref.attention(h["tap3"])
    bad, _ = ref.attention(h["tap3"], stale=(16, 40))
    scale = float(good.abs().max())
    miss = (h["z"].double() - bad).abs().amax(1) / scale
    assert float(miss[:16].max()) <= BOUNDS["z"] and float(miss[16:].max()) > BOUNDS["z"], miss


def test_bounds_catch_a_dropped_recurrent_term(measured, synth_sd):
    """One step of one direction of the time LSTM without its h feedback: the GPU's BiLSTM output misses it by more than the bound."""
    h = measured["host"]
    ref = StageRef64(synth_sd["dgrad"])
    good = ref.bilstm(h["tap2"])
    scale = float(good.abs().max())
    for drop in ((0, 0, 20), (1, 1, 50)):
        bad = ref.bilstm(h["tap2"], drop_h=drop)
        assert float((h["tap3"].double() - bad).abs().max()) / scale > BOUNDS["bilstm"], drop


def test_bounds_catch_a_missing_mean_term(measured, synth_sd):
    """One output column without its PCA mean: the GPU's rows miss that reference by more than the bound, in every frame."""
    h = measured["host"]
    ref = StageRef64(synth_sd["dgrad"])
    good = ref.expand(h["coef"])
    j = int(ref.row_means().abs().argmax())
    bad = ref.expand(h["coef"], drop_mean=j)
    miss = (h["rows"].double() - bad)[:, j].abs() / float(good.abs().max())
    assert float(miss.min()) > BOUNDS["rows"], miss


# ------------------------------------------------------------------------------------------------------------- offsets head
# The offsets regressor (BASELINE configs[4], bench.py --head offsets): three FCs to 59 coefficients, then the PCA expansion to
# Q = 15,069 columns through the generic GEMM -- a ragged last column tile (15,069 = 117 x 128 + 93: columns 14,976 .. 15,068 of
# 128-wide tiles, 14,848 .. of 256-wide ones) and a row stride of 15,069 floats (rows only 4-byte aligned).  Fed random z at every
# size of sizes_for(CUs); max|gpu - ref| / max|ref| per stage, each bound at most 4x the value measured on an MI355X, next to it.
BOUNDS_OFFSETS = {
    "coef": 3e-6,        # 8.4e-7
    "rows": 1.5e-6,      # 4.5e-7
    "rows_tail": 1.5e-6, # 3.9e-7: columns 14,848 .. 15,068 alone, normalised by their own max|ref|
}
OFF_Q = 15069
OFF_LD = 15104       # the basis' padded width, round_up(15069, 128) = 59 x 256: the expansion's Qpad
OFF_TAIL = 14848     # first column of the last 256-wide tile (and before the last 128-wide one, 14,976)
# The fp32 GEMM variants compared bitwise with the default (gemm.hip launch_any), and the sizes they run at.  The offsets head's
# GEMMs are the three FCs (Ppad 512, 256, 128; Qpad = Nc) and the expansion (Ppad = Nc, Qpad = 15,104, a bias per column).  2 and 6
# steer the LDS-tiled kernel's 64 x 64 tile choice at any size.  5 takes launch_big (256 x 256 tiles) only where Ppad and Qpad are
# multiples of 256: at Nc = 2048 on FC0, FC1 and the expansion, whose last 256-wide tile is the ragged one.  8 takes launch_fat
# where it fits (OUT_K4, no column bias, no speaker term, K % 64 == 0, Nc % 256 == 0): FC1 at Nc = 2048.  At 1025 frames
# (Nc = 1152) 5 and 8 launch the default kernels.  Variant 9 is left out: it only acts on tile-major operands, which no GEMM of
# this head has; 4 is split-bf16 and not bitwise.  (A kernel trace of the 2048-frame call on an MI355X shows gemm_big_kernel for
# FC0, FC1 and the expansion under 5 and gemm_fat_kernel for FC1 under 8; the default runs gemm_k4_kernel throughout.)
OFF_VARIANTS = (2, 5, 6, 8)
OFF_VARIANT_SIZES = (1025, 2048)


def regress_into(eng, z, spk, coef, rows):
    """sdfa_regress_forward into caller-owned coefficient and row buffers (NaN-filled by the caller, so that an element a kernel
    leaves unwritten cannot compare equal by holding bits an earlier call left in a recycled allocation)."""
    import ctypes as C
    from sdfa_amd._lib import lib, check
    n = z.shape[0]
    ws = eng.workspace(n)
    check(lib.sdfa_regress_forward(eng._m, C.c_void_p(z.data_ptr()), C.c_void_p(spk.data_ptr()), n, C.c_void_p(coef.data_ptr()),
                                   C.c_void_p(rows.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def nan_like(n, k):
    return torch.full((n, k), float("nan"), dtype=torch.float32, device="cuda:0")


def measure_offsets(sd):
    from sdfa_amd import _lib
    from sdfa_amd.engine import Engine
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ref = StageRef64(sd, device="cuda:0", head="offsets")
    eng = Engine(sd, max_frames=FULL)
    assert (eng.coef_dim, eng.out_dim) == (59, OFF_Q)
    out = dict(cus=cus, sizes={}, host=None, aligned={}, variants={})
    for n in sizes_for(cus):
        rs = np.random.RandomState(9000 + n)
        z = torch.from_numpy(rs.uniform(-0.9, 0.9, (n, 512)).astype(np.float32)).cuda()
        spk = torch.from_numpy(rs.permutation(np.arange(n) % 8)).cuda()
        coef, rows = nan_like(n, 59), nan_like(n, OFF_Q)
        regress_into(eng, z, spk, coef, rows)
        st = Stages(n)
        st.add("coef", np.arange(n), *frame_err(coef, ref.regress(z, spk)))
        tail_err, tail_ref = [], 0.0
        for f0 in range(0, n, 1024):
            sl = slice(f0, min(n, f0 + 1024))
            rr = ref.expand(coef[sl])
            st.add("rows", np.arange(sl.start, sl.stop), *frame_err(rows[sl], rr))
            tail_err.append((rows[sl, OFF_TAIL:].double() - rr[:, OFF_TAIL:]).abs().amax(1).cpu().numpy())
            tail_ref = max(tail_ref, float(rr[:, OFF_TAIL:].abs().max()))
            del rr
        st.add("rows_tail", np.arange(n), np.concatenate(tail_err), tail_ref)
        out["sizes"][n] = st
        if n == 1025:
            # rows written through output pointers 4 bytes past an aligned allocation: the regressor's epilogue and expand_coef
            # (guard elements on both sides, NaN: nothing may be written outside the rows)
            buf = torch.full((n * OFF_Q + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
            odd = buf[1:1 + n * OFF_Q].view(n, OFF_Q)
            eng.regress(z, spk, out=odd)
            buf2 = torch.full((n * OFF_Q + 4,), float("nan"), dtype=torch.float32, device="cuda:0")
            odd2 = buf2[3:3 + n * OFF_Q].view(n, OFF_Q)
            eng.expand_coef(coef, out=odd2)
            torch.cuda.synchronize()
            out["aligned"] = dict(ptr_mod16=(odd.data_ptr() % 16, odd2.data_ptr() % 16), regress=torch.equal(odd, rows),
                                  expand=torch.equal(odd2, rows), guard=bool(torch.isnan(buf[[0, -1]]).all()) and bool(torch.isnan(buf2[[0, 1, 2, -1]]).all()))
            del buf, buf2, odd, odd2
            out["host"] = dict(coef=coef[:32].cpu(), rows=rows[:32].cpu())
        if n in OFF_VARIANT_SIZES:
            for v in OFF_VARIANTS:
                cv, rv = nan_like(n, 59), nan_like(n, OFF_Q)
                try:
                    _lib.set_option("gemm_variant", v)
                    regress_into(eng, z, spk, cv, rv)
                finally:
                    _lib.set_option("gemm_variant", 0)
                out["variants"][(n, v)] = (torch.equal(cv, coef), torch.equal(rv, rows))
                del cv, rv
        del z, spk, coef, rows
    return out


@pytest.fixture(scope="module")
def offsets_measured(synth_sd):
    return measure_offsets(synth_sd["offsets"])


def offsets_table(out):
    lines = [f"offsets head, CUs {out['cus']}"]
    for n, st in out["sizes"].items():
        lines.append(f"{n:5d}  coef {st.rel('coef'):.2e}  rows {st.rel('rows'):.2e}  rows of columns {OFF_TAIL}.. {st.rel('rows_tail'):.2e}")
    lines.append(f"aligned {out['aligned']}  variants {out['variants']}")
    return "\n".join(lines)


def test_offsets_head_against_float64(offsets_measured):
    """Coefficients and rows at every size; the columns of the last (ragged) tile also on their own scale, so that an error
    confined to them is not hidden by the larger values elsewhere in the row."""
    print("\n" + offsets_table(offsets_measured))
    assert 1025 in offsets_measured["sizes"]
    for n, st in offsets_measured["sizes"].items():
        for stage in BOUNDS_OFFSETS:
            assert st.rel(stage) <= BOUNDS_OFFSETS[stage], (n, stage, st.rel(stage))


def test_offsets_rows_through_a_4_byte_aligned_pointer(offsets_measured):
    a = offsets_measured["aligned"]
    assert a["ptr_mod16"] == (4, 12), a
    assert a["regress"] and a["expand"] and a["guard"], a


def test_offsets_fp32_gemm_variants_are_bitwise(offsets_measured):
    """As tests/test_gpu_parity.py::test_gemm_variants_agree for dgrad: the fp32 GEMM choices contract k in the default kernel's
    order, so not a bit of the coefficients or the rows differs -- at 2048 frames through launch_big (the 256-wide ragged last
    column tile of the expansion) and launch_fat, which the host-side conditions below show those variants reach there."""
    for n in OFF_VARIANT_SIZES:
        assert n in offsets_measured["sizes"], n
    nc = round_up(2048)
    assert nc % 256 == 0 and OFF_LD % 256 == 0 and OFF_LD == round_up(OFF_Q) and OFF_TAIL == OFF_LD - 256
    want = {(n, v): (True, True) for n in OFF_VARIANT_SIZES for v in OFF_VARIANTS}
    assert offsets_measured["variants"] == want, offsets_measured["variants"]


def test_offsets_bound_catches_a_missing_mean_in_the_ragged_tile(offsets_measured, synth_sd):
    h = offsets_measured["host"]
    ref = StageRef64(synth_sd["offsets"], head="offsets")
    good = ref.expand(h["coef"])
    means = ref.row_means()
    j = 14976 + int(means[14976:].abs().argmax())
    miss = (h["rows"].double() - ref.expand(h["coef"], drop_mean=j))[:, j].abs() / float(good.abs().max())
    assert float(miss.min()) > BOUNDS_OFFSETS["rows"], (j, miss)


if __name__ == "__main__":
    from sdfa_amd import synth
    if sys.argv[1:] == ["offsets"]:
        print(offsets_table(measure_offsets(synth.make_state_dict("offsets", 1234))))
        sys.exit(0)
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    res = measure(synth.make_state_dict("dgrad", 1234))
    torch.cuda.synchronize()
    res["seconds"], res["peak_bytes"] = time.time() - t0, torch.cuda.max_memory_allocated()
    print(table(res))
    print(json.dumps({"forms": res["forms"], "mismatch": {str(n): st.mismatch for n, st in res["sizes"].items()},
                      "frontend_frames": res["frontend"].n, "frontend_mismatch": res["frontend"].mismatch}))
