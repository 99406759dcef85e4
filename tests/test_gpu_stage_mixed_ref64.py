"""Each stage of the mixed-precision modes (bf16x3, bf16x6, bf16x3_attention) against the float64 restatement of that stage alone
(tests/stage_ref64.py), fed the GPU's own input to the stage (the debug taps): what tests/test_gpu_stage_ref64.py does for fp32,
at the smallest frame count that reaches each launch form these modes pick (mixed_forms there restates the launch code).

The reference is the plain float64 operation, not a model of bf16 arithmetic; the bounds are measured against it.

  bf16x6            held to the fp32 BOUNDS / BOUNDS_OFFSETS of tests/test_gpu_stage_ref64.py, unchanged
  bf16x3            BOUNDS_MIXED["bf16x3"], each at most 4x the value measured on an MI355X and none above 1e-4
  bf16x3_attention  z and align only (the body is fp32: its BiLSTM tap is asserted bitwise the fp32 engine's)

A stage is compared at a size only where that size is the smallest that reaches one of the stage's launch forms (size_plan), and
at 1, 17 and 129 frames (ragged 16-frame units, the padded last 128-frame tile, the tile queue's second round); z, align, coef and
rows of the shipping engine must equal the debug_keep engine's bitwise at every size.  The regressor writes into NaN-filled
buffers, so an element a kernel skips cannot pass by holding an earlier call's value.

Sensitivity controls (bottom): plain bf16 -- single-term operands, what a split kernel computes once it loses its low-order terms --
misses the bf16x3 bound of a stage in every 16-frame unit; the bf16x3 rows miss a float64 expansion over the bf16-rounded basis in
every frame; and the stale-tile, dropped-recurrent-term and missing-mean controls of the fp32 test hold on the bf16x3 taps.

`python tests/test_gpu_stage_mixed_ref64.py` prints the measured errors per mode, stage and size (profiles/stage_mixed_ref64.txt:
how the bounds were set).  On an MI355X the module takes 14 s run alone, 8 s inside the suite; its slowest test, the first of
bf16x3 (all seven sizes of the mode), takes 2.4 s there and 6.7 s alone, where it also pays the process's first use of the device.
"""
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
from test_gpu_stage_ref64 import (BOUNDS, BOUNDS_OFFSETS, FULL, OFF_Q, OFF_TAIL, Stages, attention_form, edge_mask, frame_err,  # noqa: E402
                                  mixed_forms, nan_like, offsets_expand_form, random_batch, regress_into, round_up, sampled_frames)

pytestmark = pytest.mark.gpu

MODES = ("bf16x3", "bf16x6", "bf16x3_attention")
STAGES = ("conv3", "freq", "bilstm", "z", "align", "coef", "rows")
MODE_STAGES = {"bf16x3": STAGES, "bf16x6": STAGES, "bf16x3_attention": ("z", "align")}
SMALL = (1, 17, 129)         # every stage of the mode is compared at these

# max|gpu - ref| / max|ref| per stage over every size the stage is compared at; next to each bound the largest value measured on an
# MI355X (256 CUs, profiles/stage_mixed_ref64.txt), of which the bound is at most 4x.  bf16x6 is held to the fp32 bounds: the
# project's claim for that mode (measured: conv3 3.5e-7, freq 4.7e-6, bilstm 1.3e-6, z 7.1e-7, align 2.6e-6, coef 7.3e-7, rows 6.7e-7).
#
# Two split-bf16 stages measure above 2.5e-5, so 4x of them would pass the 1e-4 budget and their bound is the budget itself (2.8x and
# 3.0x what was measured): the BiLSTM and the attention weights.  Why they are that large: two bf16 terms carry 16 significand bits
# where fp32 carries 24, and the conv stack -- one contraction per layer, no recurrence -- already shows what that costs: 1.2e-5 against
# fp32's 5.7e-7, a factor of 20.  The BiLSTM's 3.6e-5 is the same factor of 20 over its fp32 error (1.8e-6): two layers of 64
# recurrent steps carry operand rounding forward exactly as they carry fp32's accumulation rounding.  The attention weights are
# softmax outputs of scores that the tanh of a 512-deep split projection feeds; 3.3e-5 is 6x fp32's 5.8e-6.  Neither error has a
# position: the edge / padded-tail frames are never more than 5 % above the rest, every 16-frame unit of the 129-frame run lies
# within a factor of 2.1 of the worst one (bilstm 2.1e-5 .. 3.1e-5, align 1.6e-5 .. 3.3e-5), and the maximum grows with the number of
# frames as the largest of more samples does (bilstm: 1.5e-5 at 1 frame, 3.1e-5 at 129, 3.6e-5 at 8,192).  Plain bf16 -- a lost low
# term -- is 50x to 230x above either bound in every unit.
BOUNDS_MIXED = {
    "bf16x3": {
        "conv3": 4e-5,       # 1.16e-5
        "freq": 3e-5,        # 8.83e-6
        "bilstm": 1e-4,      # 3.59e-5 (8,192 frames; 3.08e-5 at 129)
        "z": 1.5e-5,         # 4.57e-6 (8,192 frames)
        "align": 1e-4,       # 3.30e-5
        "coef": 4e-5,        # 1.26e-5
        "rows": 2.5e-5,      # 6.88e-6
    },
    "bf16x6": BOUNDS,
    "bf16x3_attention": {
        "z": 1.5e-5,         # 4.94e-6 (8,192 frames)
        "align": 1e-4,       # 2.78e-5
    },
}
BOUNDS_OFFSETS_MIXED = {
    "bf16x3": {
        "coef": 3e-5,        # 8.47e-6
        "rows": 2.5e-5,      # 7.20e-6
        "rows_tail": 2e-5,   # 6.16e-6: columns 14,848 .. 15,068 alone, normalised by their own max|ref|
    },
    "bf16x6": BOUNDS_OFFSETS,    # measured: coef 6.9e-7, rows 3.6e-7, rows_tail 3.2e-7
}
BF16X3_CEILING = 1e-4        # no bf16x3 bound may exceed the project's budget
OFF_SIZES = (129, 1024, 1025)


def size_plan(mode, cus):
    """{frames: stages compared there}.  1, 17 and 129 frames: every stage of the mode.  Then, for every launch form of a stage that
    some chunk size Nc in 128 .. 8192 reaches and a smaller size has not, the smallest frame count of that Nc (Nc - 127: one real frame
    in the padded last 128-frame tile; 8,192 itself for the full chunk) -- and only the stages whose form is new there."""
    own = lambda nc: mixed_forms(mode, nc, cus)      # keyed by stage; "z" stands for align too
    plan, seen = {}, set()
    for n in SMALL:
        plan[n] = set(MODE_STAGES[mode])
        seen |= set(own(round_up(n)).items())
    for nc in range(128, FULL + 1, 128):
        new = {s for s in own(nc).items() if s not in seen}
        if new:
            seen |= new
            stages = {s for s, _ in new}
            plan[FULL if nc == FULL else nc - 127] = (stages | ({"align"} if "z" in stages else set())) & set(MODE_STAGES[mode])
    return plan


def forms_reached(mode, sizes, cus):
    return {(s, f) for n in sizes for s, f in mixed_forms(mode, round_up(n), cus).items()}


def run_size(ref, keep, ship, feat, spk, stages, conv_ref=None, all_conv=False):
    """Both engines on `feat` (one chunk; `ship` may be None); the stages named of the debug_keep run, each against the float64
    stage fed the previous tap.  Returns the Stages and the first 32 frames of what the sensitivity controls read."""
    n = feat.shape[0]
    st = Stages(n)
    z, align = keep.encoder(feat)
    coef, rows = nan_like(n, keep.coef_dim), nan_like(n, keep.out_dim)
    regress_into(keep, z, spk, coef, rows)
    if ship is not None:
        z2, a2 = ship.encoder(feat)
        c2, r2 = nan_like(n, keep.coef_dim), nan_like(n, keep.out_dim)
        regress_into(ship, z2, spk, c2, r2)
        for what, a, b in (("z", z, z2), ("align", align, a2), ("coef", coef, c2), ("rows", rows, r2)):
            if not torch.equal(a, b):       # NaN (an unwritten element) never compares equal
                st.mismatch.append(what)
        del z2, a2, c2, r2
    every = np.arange(n)
    tap = {}

    def tapped(k):
        if k not in tap:
            tap[k] = keep.tap(k, n)
        return tap[k]
    if "conv3" in stages:
        fr = every if all_conv else sampled_frames(n)
        fi = torch.from_numpy(fr).to(feat.device)
        want = conv_ref(n, feat, fi) if conv_ref is not None else ref.conv_stack(feat[fi])
        st.add("conv3", fr, *frame_err(tapped(1)[fi], want))
        del want
    if "freq" in stages:
        st.add("freq", every, *frame_err(tapped(2), ref.freq(tapped(1))))
    tap.pop(1, None)
    if "bilstm" in stages:
        st.add("bilstm", every, *frame_err(tapped(3), ref.bilstm(tapped(2))))
    if "z" in stages or "align" in stages:
        zr, ar = ref.attention(tapped(3))
        st.add("z", every, *frame_err(z, zr))
        st.add("align", every, *frame_err(align, ar))
        del zr, ar
    if "coef" in stages:
        st.add("coef", every, *frame_err(coef, ref.regress(z, spk)))
    if "rows" in stages:
        for f0 in range(0, n, 1024):
            sl = slice(f0, min(n, f0 + 1024))
            st.add("rows", np.arange(sl.start, sl.stop), *frame_err(rows[sl], ref.expand(coef[sl])))
    host = dict(z=z[:32].cpu(), coef=coef[:32].cpu(), rows=rows[:32].cpu())
    for k in (2, 3):
        if k in tap:
            host[f"tap{k}"] = tap[k][:32].cpu()
    return st, host, (coef, rows)


class ConvRef:
    """The float64 conv stack of the sampled frames of a size: the same for every mode (it reads the features, not a tap)."""

    def __init__(self, ref):
        self.ref, self.got = ref, {}

    def __call__(self, n, feat, fi):
        if n not in self.got:
            self.got[n] = self.ref.conv_stack(feat[fi]).cpu()      # host: at most 32 frames x 1 MiB per size
        return self.got[n].to(feat.device)


def measure_mode(sd, mode, ref, conv_ref):
    from sdfa_amd.engine import Engine
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    keep = Engine(sd, max_frames=FULL, debug_keep=True, precision=mode)
    ship = Engine(sd, max_frames=FULL, precision=mode)
    plan = size_plan(mode, cus)
    out = dict(mode=mode, cus=cus, plan=plan, sizes={}, secs={}, host=None)
    for n, stages in plan.items():
        t1 = time.time()
        feat, spk = random_batch(n, 7000 + n)
        st, host, (coef, rows) = run_size(ref, keep, ship, feat, spk, stages, conv_ref)
        if n == 129:
            out["host"] = host
            if mode == "bf16x3":
                # lost low-order terms of the basis: the rows against the float64 expansion over the bf16-rounded basis, per frame
                good = ref.expand(coef)
                bad = ref.expand(coef, bf16_basis=True)
                out["rounded_basis_miss"] = ((rows.double() - bad).abs().amax(1) / float(good.abs().max())).cpu().numpy()
                del good, bad
            if mode == "bf16x3_attention":
                fp32 = Engine(sd, max_frames=FULL, debug_keep=True)
                fp32.encoder(feat)
                out["body_is_fp32"] = torch.equal(fp32.tap(3, n), keep.tap(3, n))
                del fp32
        del feat, spk, coef, rows
        torch.cuda.synchronize()
        out["sizes"][n] = st
        out["secs"][n] = time.time() - t1
    out["seconds"] = time.time() - t0
    return out


def measure_plain_bf16(sd, ref):
    """The lost-low-order-terms control: plain bf16 (one term per operand everywhere) at 129 frames, every stage on every frame."""
    from sdfa_amd.engine import Engine
    keep = Engine(sd, max_frames=FULL, debug_keep=True, precision="bf16")
    feat, spk = random_batch(129, 7000 + 129)
    st, _, _ = run_size(ref, keep, None, feat, spk, STAGES, None, all_conv=True)
    return st


def unit_worst(st, stage):
    """max|gpu - ref| / max|ref| of every 16-frame unit"""
    frames, err, refmax = st.err[stage]
    return np.array([err[frames // 16 == u].max() for u in np.unique(frames // 16)]) / refmax


def measure_offsets_mixed(sd, mode, ref):
    from sdfa_amd.engine import Engine
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    eng = Engine(sd, max_frames=FULL, precision=mode)
    assert (eng.coef_dim, eng.out_dim) == (59, OFF_Q)
    out = dict(mode=mode, cus=cus, sizes={}, forms={n: offsets_expand_form(mode, round_up(n), cus) for n in OFF_SIZES})
    for n in OFF_SIZES:
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
        del z, spk, coef, rows
    return out


# ------------------------------------------------------------------------------------------------------------------ tables
def mode_table(out):
    lines = [f"{out['mode']}  CUs {out['cus']}  ({out['seconds']:.1f} s: " + ", ".join(f"{n} {s:.1f}" for n, s in out["secs"].items()) + ")"]
    for stage in MODE_STAGES[out["mode"]]:
        for n, st in out["sizes"].items():
            if stage not in st.err:
                continue
            nn = st.n
            lines.append(f"{stage:7s} {n:5d}  all {st.rel(stage):.2e}  edge {st.rel(stage, lambda f: edge_mask(f, nn)):.2e}  "
                         f"rest {st.rel(stage, lambda f: ~edge_mask(f, nn)):.2e}")
    if 129 in out["sizes"]:
        for stage in MODE_STAGES[out["mode"]]:
            if out["sizes"][129].err[stage][0].size == 129:
                u = unit_worst(out["sizes"][129], stage)
                lines.append(f"{stage:7s}   129  per 16-frame unit: min {u.min():.2e}  max {u.max():.2e}")
    lines.append("shipping engine differs from the debug_keep engine: " + (str({n: st.mismatch for n, st in out["sizes"].items() if st.mismatch}) or "{}"))
    for n in out["sizes"]:
        lines.append(f"forms {n:5d}  " + "; ".join(f"{s}: {f}" for s, f in mixed_forms(out["mode"], round_up(n), out["cus"]).items()))
    return "\n".join(lines)


def plain_bf16_table(st):
    lines = ["plain bf16 at 129 frames, per 16-frame unit: min / max over units of the unit's max|gpu - ref| / max|ref|"]
    for stage in STAGES:
        u = unit_worst(st, stage)
        lines.append(f"{stage:7s}  min {u.min():.2e}  max {u.max():.2e}")
    return "\n".join(lines)


def offsets_mixed_table(out):
    lines = [f"offsets head, {out['mode']}, CUs {out['cus']}"]
    for n, st in out["sizes"].items():
        lines.append(f"{n:5d}  coef {st.rel('coef'):.2e}  rows {st.rel('rows'):.2e}  rows of columns {OFF_TAIL}.. {st.rel('rows_tail'):.2e}  {out['forms'][n]}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def ref64(synth_sd):
    ref = StageRef64(synth_sd["dgrad"], device="cuda:0")
    return ref, ConvRef(ref)


@pytest.fixture(scope="module")
def measured(synth_sd, ref64):
    """mode -> its measurement, made when a test first asks for it (both engines of a mode are gone before the next mode's are built)"""
    got = {}

    def get(mode):
        if mode not in got:
            got[mode] = measure_mode(synth_sd["dgrad"], mode, *ref64)
        return got[mode]
    return get


@pytest.fixture(scope="module")
def plain_bf16(synth_sd, ref64):
    return measure_plain_bf16(synth_sd["dgrad"], ref64[0])


@pytest.fixture(scope="module")
def ref64_cpu(synth_sd):
    return StageRef64(synth_sd["dgrad"])


@pytest.fixture(scope="module")
def offsets_measured(synth_sd):
    ref = StageRef64(synth_sd["offsets"], device="cuda:0", head="offsets")
    return {mode: measure_offsets_mixed(synth_sd["offsets"], mode, ref) for mode in BOUNDS_OFFSETS_MIXED}


# ------------------------------------------------------------------------------------------------------------------- tests
PINNED_256 = {"bf16x3": [1, 17, 129, 385, 1921, 3969, 8192], "bf16x6": [1, 17, 129, 385], "bf16x3_attention": [1, 17, 129, 1921, 3969, 8192]}


def test_sizes_hit_every_launch_form():
    """The sizes of size_plan reach every form any chunk size reaches on this device, and are these for 256 CUs:
      1, 17   Nc = 128: ragged 16-frame units; the persistent frequency LSTM with one tile per workgroup; 128-wide split GEMMs
      129     Nc = 256: the tile queue's second round, the padded last 128-frame tile
      385     Nc = 512: the 256 x 256 split GEMM of the frequency projection ((Mc / 256) * 2 >= 256 from Mc = 32,768), and an
              expansion whose work units are all whole
      1921, 3969, 8192   Nc = 2048, 4096, 8192: attn_key_score_kernel<3> + attn_kernel<true> at ts_shift 2, 1 and 0 (bf16x3,
              bf16x3_attention); 8192 also time_lstm_bf16_kernel<2,3> (bf16x3)
    The six-product mode keeps 32-frame tiles and runs the fp32 attention kernels: nothing of its own beyond 385."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for c in sorted({cus, 256}):
        for mode in MODES:
            plan = size_plan(mode, c)
            every = forms_reached(mode, range(128, FULL + 1, 128), c)
            assert forms_reached(mode, plan, c) == every, (mode, c)
            for s in MODE_STAGES[mode]:      # every form of a stage is also compared somewhere
                key = "z" if s == "align" else s
                assert {f for n, st in plan.items() if s in st for k, f in mixed_forms(mode, round_up(n), c).items() if k == key} == \
                       {f for k, f in every if k == key}, (mode, c, s)
            if c == 256:
                assert sorted(plan) == PINNED_256[mode], (mode, sorted(plan))
    f = lambda mode, n: mixed_forms(mode, round_up(n), 256)
    assert "one round" in f("bf16x3", 17)["freq"] and "several rounds" in f("bf16x3", 129)["freq"]
    assert "gemm_bf16_kernel<3>" in f("bf16x3", 129)["freq"] and "gemm_bf16_big_kernel<3>" in f("bf16x3", 385)["freq"]
    assert "gemm_bf16x6_kernel" in f("bf16x6", 129)["freq"] and "gemm_bf16x6_big_kernel" in f("bf16x6", 385)["freq"]
    assert [f("bf16x3_attention", n)["z"][-1] for n in (129, 1921, 3969, 8192)] == ["3", "2", "1", "0"]
    assert "<1,3>" in f("bf16x3", 8064)["bilstm"] and "<2,3>" in f("bf16x3", 8192)["bilstm"] and "<1,6>" in f("bf16x6", 8192)["bilstm"]
    # where the fp32 path has already handed over to the one-launch kernel, these modes still run attn_kernel<true>
    assert attention_form(4096, 256) == attention_form(8192, 256) == "attn_fused_f32_kernel"


@pytest.mark.parametrize("mode", MODES)
def test_debug_keep_engine_gives_the_shipping_bits(measured, mode):
    """z, align, coef and rows of the shipping engine (fused conv stack, columns shared by content) are bitwise the debug_keep
    engine's in every mode at every size: the taps are the arithmetic that ships."""
    out = measured(mode)
    print("\n" + mode_table(out))
    bad = {n: st.mismatch for n, st in out["sizes"].items() if st.mismatch}
    assert not bad, bad


@pytest.mark.parametrize("mode,stage", [(m, s) for m in MODES for s in MODE_STAGES[m]])
def test_stage_against_float64(measured, mode, stage):
    out = measured(mode)
    worst = {n: st.rel(stage) for n, st in out["sizes"].items() if stage in st.err}
    print(f"\n{mode} {stage}: {worst}")
    assert set(SMALL) <= set(worst)
    assert max(worst.values()) <= BOUNDS_MIXED[mode][stage], (mode, stage, worst)      # NaN (an unwritten element) fails too


def test_bounds_follow_the_rules():
    """bf16x6 is held to the fp32 bounds themselves; no bf16x3 bound exceeds the 1e-4 budget."""
    assert BOUNDS_MIXED["bf16x6"] is BOUNDS and BOUNDS_OFFSETS_MIXED["bf16x6"] is BOUNDS_OFFSETS
    for table in (BOUNDS_MIXED["bf16x3"], BOUNDS_MIXED["bf16x3_attention"], BOUNDS_OFFSETS_MIXED["bf16x3"]):
        assert all(0 < b <= BF16X3_CEILING for b in table.values()), table


def test_attention_only_mode_runs_the_fp32_body(measured):
    """bf16x3_attention: the BiLSTM tap is bitwise the fp32 engine's, so its body is what tests/test_gpu_stage_ref64.py covers."""
    assert measured("bf16x3_attention")["body_is_fp32"] is True


# ------------------------------------------------------------------------------------------------------ sensitivity controls
@pytest.mark.parametrize("stage", ["conv3", "freq", "bilstm", "z", "align", "coef"])
def test_bounds_catch_lost_low_order_terms(plain_bf16, stage):
    """Plain bf16 is the arithmetic a split kernel degenerates to when it drops its lo terms.  Every 16-frame unit of its stage --
    against float64 of its own tap -- misses the bf16x3 bound of that stage, so one unit with lost terms is caught wherever it sits."""
    print("\n" + plain_bf16_table(plain_bf16))
    u = unit_worst(plain_bf16, stage)
    assert len(u) == 9 and float(u.min()) > BOUNDS_MIXED["bf16x3"][stage], (stage, u)


def test_bounds_catch_a_bf16_rounded_basis(measured):
    """Plain bf16 keeps the dgrad expansion in fp32, so the expansion has a control of its own: the bf16x3 rows against the float64
    expansion over the basis rounded to bf16 miss by more than the rows bound in every frame."""
    miss = measured("bf16x3")["rounded_basis_miss"]
    assert miss.shape == (129,) and float(miss.min()) > BOUNDS_MIXED["bf16x3"]["rows"], miss


def test_bounds_catch_a_stale_attention_tile(measured, ref64_cpu):
    h = measured("bf16x3")["host"]
    bound = BOUNDS_MIXED["bf16x3"]["z"]
    good, _ = ref64_cpu.attention(h["tap3"])
    bad, _ = ref64_cpu.attention(h["tap3"], stale=(16, 40))
    miss = (h["z"].double() - bad).abs().amax(1) / float(good.abs().max())
    assert float(miss[:16].max()) <= bound and float(miss[16:].max()) > bound, miss


def test_bounds_catch_a_dropped_recurrent_term(measured, ref64_cpu):
    h = measured("bf16x3")["host"]
    scale = float(ref64_cpu.bilstm(h["tap2"]).abs().max())
    for drop in ((0, 0, 20), (1, 1, 50)):
        bad = ref64_cpu.bilstm(h["tap2"], drop_h=drop)
        assert float((h["tap3"].double() - bad).abs().max()) / scale > BOUNDS_MIXED["bf16x3"]["bilstm"], drop


def test_bounds_catch_a_missing_mean_term(measured, ref64_cpu):
    h = measured("bf16x3")["host"]
    good = ref64_cpu.expand(h["coef"])
    j = int(ref64_cpu.row_means().abs().argmax())
    miss = (h["rows"].double() - ref64_cpu.expand(h["coef"], drop_mean=j))[:, j].abs() / float(good.abs().max())
    assert float(miss.min()) > BOUNDS_MIXED["bf16x3"]["rows"], miss


# ------------------------------------------------------------------------------------------------------------- offsets head
@pytest.mark.parametrize("mode", list(BOUNDS_OFFSETS_MIXED))
def test_offsets_head_against_float64(offsets_measured, mode):
    """The offsets head on random z in the split modes: 129 frames (Nc = 256: the 128-wide split GEMM), 1024 (the 256 x 256 one,
    whose last column tile 14,848 .. 15,068 is the ragged one) and 1025 (Nc = 1152: the 128-wide kernel at scale).  Coefficients,
    rows, and the columns from 14,848 on their own scale."""
    out = offsets_measured[mode]
    print("\n" + offsets_mixed_table(out))
    if out["cus"] == 256:
        big = "gemm_bf16x6_big_kernel" if mode == "bf16x6" else "gemm_bf16_big_kernel<3>"
        assert [out["forms"][n] == big for n in OFF_SIZES] == [False, True, False], out["forms"]
    for n, st in out["sizes"].items():
        for stage, bound in BOUNDS_OFFSETS_MIXED[mode].items():
            assert st.rel(stage) <= bound, (mode, n, stage, st.rel(stage))


if __name__ == "__main__":
    from sdfa_amd import synth
    t0 = time.time()
    sd = synth.make_state_dict("dgrad", 1234)
    ref = StageRef64(sd, device="cuda:0")
    conv_ref = ConvRef(ref)
    for mode in MODES:
        res = measure_mode(sd, mode, ref, conv_ref)
        print(mode_table(res), flush=True)
        if mode == "bf16x3":
            miss = res["rounded_basis_miss"]
            print(f"bf16x3 rows against the expansion over the bf16-rounded basis, per frame: min {miss.min():.2e}  max {miss.max():.2e}")
        if mode == "bf16x3_attention":
            print(f"tap 3 bitwise the fp32 engine's: {res['body_is_fp32']}")
        del res
    print(plain_bf16_table(measure_plain_bf16(sd, ref)), flush=True)
    del ref, conv_ref
    sd_off = synth.make_state_dict("offsets", 1234)
    ref_off = StageRef64(sd_off, device="cuda:0", head="offsets")
    for mode in BOUNDS_OFFSETS_MIXED:
        print(offsets_mixed_table(measure_offsets_mixed(sd_off, mode, ref_off)), flush=True)
    print(f"total {time.time() - t0:.1f} s, peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
