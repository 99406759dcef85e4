"""Every launch form of the front end (csrc/frontend.hip, share.hip) against the float64 restatement of tests/frontend_ref64.py, on
every element of every frame, at 8 kHz (WIN = 512: the radix-4 stages and one radix-2 stage) and 16 kHz (WIN = 1024).

Metric: r = max |gpu - ref| / kappa, kappa being the per-element error scale of an exact-algorithm fp32 front end (tests/frontend_ref64.py
derives it from the float64 quantities alone).  A fixed tolerance would be too loose where the signal is strong or fail where it is
weak; kappa follows the log's magnification of the transform's rounding band by band.  The plain max abs error is reported beside it,
split into elements whose kappa is within 10x of its floor (2^-24) and the rest.

Inputs, at both rates: clip geometry (exactly one window, one sample more, a hop less one sample more, a clip whose last inner window
ends at its last sample, 1.9 s + 11 samples, 10 s, all zeros), signal dynamics (uniform noise, speechlike, sine sweep, full-scale
square wave, 1e-4 and 1e-3 noise, DC offset, one impulse, a tone on a bin centre), frame tables (the 60 fps enumeration, 25 and 30 fps, and a
hand-made table with frames before the clip, past its end, off the hop grid and out of order), a ragged batch (80 sentences of 3 - 6 s
at 8 kHz as BASELINE configs[4]; 24 at 16 kHz) and, at 16 kHz, the bench batch (32 x 10 s = 20,352 frames).  The shipping stream
(mel_stream_kernel<WIN, true>) runs all of them; on the ragged batch also the phase form, the repair pass (forced by a one-poll
hand-off bound), the two-kernel form, the t-major numbering, the radix-4 transform (16 kHz) and the per-window frontend_kernel, which
is not bitwise equal to the others and is checked here only.  One sdfa_mel_frontend_ring call per rate reads windows across the ring's
wrap point.

Exact assertions besides the bound: frames of an all-zero clip and frames whose window holds no sample are 0; every output is finite;
the status word is 0 except in the forced-repair case.  The sensitivity controls at the bottom show that the bound catches each
perturbation of tests/frontend_ref64.py on the GPU's own output, with a margin of at least 100.

`python tests/test_gpu_frontend_ref64.py` prints the table the bounds came from.  Measured on an MI355X (256 CUs): the measurement
takes 3 s (the whole module under pytest about 7 s), peak device memory 7.0 GiB; the float64 reference runs on the device in chunks
of 512 frames.
"""
import ctypes as C
import math
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
from frontend_ref64 import FrontendRef64, U, geometry                          # noqa: E402

pytestmark = pytest.mark.gpu

# max |gpu - ref| / kappa over every element of every input; at most 4x the largest value measured on an MI355X (256 CUs), written
# next to it.  The stream and the forms bitwise equal to it, the ring call and the radix-4 transform share one bound per rate; the
# per-window frontend_kernel (its own transform and arithmetic order) has its own.
BOUND_R = {
    8000: 8.0,       # 2.28 (ragged batch, every form; ring 1.74)
    16000: 8.0,      # 2.27 (radix-4 on the ragged batch; the stream 1.63, ring 1.25)
}
BOUND_R_PER_WINDOW = {
    8000: 10.0,      # 2.93
    16000: 16.0,     # 4.89
}

SRS = (8000, 16000)
FORMS = {
    "stream": {},
    "phases": {"frontend_stream_phases": 1},
    "repair": {"frontend_stream_spin_max": 1},
    "two_kernel": {"frontend_two_kernel": 1},
    "t_major": {"frontend_t_major": 1},
    "radix4": {"mel_fft_radix4": 1},
    "per_window": {},
}
OPTIONS = ("frontend_two_kernel", "frontend_stream_block", "frontend_stream_slots", "frontend_stream_phases", "frontend_stream_spin_max",
           "frontend_t_major", "mel_fft_radix4")
# The sensitivity controls: r of the GPU's output against the perturbed reference, measured at 8 / 16 kHz, next to each.  Every one
# must exceed SENS_MARGIN times the bound (the smallest measured is 676 times it).
PERTURBATIONS = {
    "preemph_col0": dict(preemph_col0=True),           # 8.5e3 / 5.4e3
    "stale_col": dict(stale_col=(150, 30)),            # 5.3e5 / 3.7e5
    "mel_shift": dict(mel_shift=60),                   # 8.2e5 / 5.6e5
    "delta_edge_zero": dict(delta_edge_zero=True),     # 2.2e6 / 2.0e6
    "pad_off_by_one": dict(pad_off_by_one=True),       # 3.2e5 / 9.1e4
    "periodic_hamming": dict(periodic_hamming=True),   # 2.4e4 / 9.5e3
}
SENS_MARGIN = 100
CHUNK = 512


def stream_blocks(n_frames, cus, slots=12):
    """(frames per block, blocks, blocks padded to 8) of the stream kernel's default geometry (frontend.hip stream_geometry)."""
    B = 144
    if -(-n_frames // B) * slots < 2 * cus:
        B = min(144, max(48, n_frames * slots // (2 * cus) // 12 * 12))
    nb = -(-n_frames // B)
    return B, nb, -(-nb // 8) * 8


# ------------------------------------------------------------------------------------------------------------------ inputs
def signals(sr, L):
    from sdfa_amd import synth
    win = geometry(sr)[0]
    n = np.arange(L)
    rs = np.random.RandomState(sr + 1)
    imp = np.zeros(L, np.float32)
    imp[L // 2 + 37] = 0.9
    return {
        "uniform": synth.make_pcm(30, L),
        "speechlike": synth.make_pcm(31, L, "speechlike"),
        "sweep": synth.make_pcm(32, L, "sweep"),
        "square_full_scale": np.where(np.sin(2 * np.pi * 210.0 * n / sr) >= 0, 1.0, -1.0).astype(np.float32),
        "noise_1e-4": (1e-4 * rs.uniform(-1, 1, L)).astype(np.float32),               # below the lower clamp throughout
        "noise_1e-3": (1e-3 * rs.uniform(-1, 1, L)).astype(np.float32),               # straddling it
        "dc_offset": (0.3 + 0.1 * synth.make_pcm(33, L, "speechlike")).astype(np.float32),
        "impulse": imp,
        "bin_centre_tone": (0.5 * np.sin(2 * np.pi * 37 * (n % win) / win)).astype(np.float32),
    }


def end_aligned_length(sr):
    """A clip length at which a window of the 60 fps enumeration ends exactly at the clip's last sample."""
    from sdfa_amd.engine import frame_index
    _, _, sliding = geometry(sr)
    L = int(np.floor(np.float32(100 * sr / 60.0))) + sliding // 2
    starts, _ = frame_index(L, sr)
    assert (starts + sliding == L).any()
    return L


def hand_table(sr, L):
    """Frames before the clip (one sample in, none in, partly in), past its end, ending at its end, off the hop grid, a hop chain,
    and the same frames again out of order."""
    _, hop, sliding = geometry(sr)
    rs = np.random.RandomState(sr)
    s = [-sliding + 1, -sliding, -sliding - 40, -700, -1, 0, 3, L - sliding, L - sliding + 1, L - 1, L, L + 50]
    s += list(1000 + hop * np.arange(40))                                     # a chain that shares columns
    s += list(rs.randint(-sliding, L, 40))                                    # off the grid
    s += list(2000 + 3 * hop * np.arange(20)[::-1])                           # descending
    s += list(rs.permutation(s))                                              # everything again, shuffled
    s = np.asarray(s, np.int64)
    return [(s, np.zeros(len(s), np.int64))]


def cases(sr):
    """[(name, clips, tables or None, forms)]: every input of this module at one rate."""
    from sdfa_amd import synth
    from sdfa_amd.engine import frame_index
    win, hop, sliding = geometry(sr)
    out = [
        ("one_window", [synth.make_pcm(22, sliding)], None),
        ("one_window+1", [synth.make_pcm(23, sliding + 1, "speechlike")], None),
        ("one_window+hop-1", [synth.make_pcm(24, sliding + hop - 1)], None),
        ("ends_at_clip_end", [synth.make_pcm(25, end_aligned_length(sr), "sweep")], None),
        ("1.9s+11", [synth.make_pcm(21, int(1.9 * sr) + 11, "speechlike")], None),
        ("10s", [synth.make_pcm(0, 10 * sr)], None),
        ("zeros", [np.zeros(int(1.5 * sr), np.float32)], None),
    ]
    out += [(k, [v], None) for k, v in signals(sr, 2 * sr).items()]
    clip = synth.make_pcm(9, 3 * sr, "speechlike")
    for fps in (25, 30):
        out.append((f"{fps}fps", [clip], [frame_index(len(clip), sr, fps=fps)]))
    out.append(("hand_table", [clip], hand_table(sr, len(clip))))
    rs = np.random.RandomState(80 + sr)
    kinds = ("speechlike", "uniform", "sweep")
    nsent = 80 if sr == 8000 else 24
    ragged = [synth.make_pcm(100 + i, int(rs.uniform(3, 6) * sr), kinds[i % 3]) for i in range(nsent)]
    forms = [f for f in FORMS if f != "radix4" or sr == 16000]
    out = [(name, clips, tables, ["stream"]) for name, clips, tables in out]
    out.append(("ragged", ragged, None, forms))
    if sr == 16000:
        out.append(("bench_batch", [synth.make_pcm(c, 10 * sr) for c in range(32)], None, ["stream"]))
    return out


# ------------------------------------------------------------------------------------------------------------------ compare
def empty_frames(clips, fc, fs, sliding):
    """Frames that must be exactly 0: the window holds no sample, or the clip is all zeros."""
    lens = np.array([len(c) for c in clips])[fc]
    silent = np.array([not np.any(c) for c in clips])[fc]
    return (fs + sliding <= 0) | (fs >= lens) | silent


def compare(ref, clips, fc, fs, got, **pert):
    """r, max abs error where kappa <= 10 u, max abs error elsewhere: all frames, in chunks."""
    r, a_floor, a_rest = 0.0, 0.0, 0.0
    for f0, f1, feat, kappa in ref.chunks(clips, fc, fs, chunk=CHUNK, **pert):
        e = (got[f0:f1].to(feat.device).double() - feat).abs()
        r = max(r, float((e / kappa).max()))
        near = kappa <= 10 * U
        if near.any():
            a_floor = max(a_floor, float(e[near].max()))
        if (~near).any():
            a_rest = max(a_rest, float(e[~near].max()))
        del e, feat, kappa, near
    return r, a_floor, a_rest


def run_form(fe, clips, sr, tables, form):
    from sdfa_amd import _lib
    try:
        for k, v in FORMS[form].items():
            _lib.set_option(k, v)
        got, _, _ = fe.mel_frontend(clips, sr, tables=tables, gather=form != "per_window")
        torch.cuda.synchronize()
        status = None if form == "per_window" else fe.frontend_status()
    finally:
        for k in OPTIONS:
            _lib.set_option(k, 0)
    fc, fs, _ = fe.last_frame_table
    return got, fc.cpu().numpy(), fs.cpu().numpy(), status


def ring_case(sr, ref):
    """sdfa_mel_frontend_ring on one stream whose frames straddle the ring's wrap point and its valid end (as
    tests/test_live_gpu.py::test_frontend_ring_equals_gather), against float64 of the same frames cut from the signal."""
    from sdfa_amd import synth, live
    from sdfa_amd._lib import lib, check
    win, hop, sliding = geometry(sr)
    r = int(np.ceil(np.log2(sliding + 1)))
    R = 1 << r
    L = 3 * R + 1234
    sig = synth.make_pcm(40 + sr, L, "speechlike")
    hi = L - 37
    lo = L - R + 1
    starts = list(range(lo, hi - 40, hop * 7)) + list(range(hi - sliding - 3 * hop, hi + 9, hop)) + [3 * R - 500, 3 * R - sliding // 2]
    starts = np.array(sorted(set(s for s in starts if s >= lo)), np.int64)
    S = R + live.RING_MIRROR
    buf = np.zeros(S, np.float32)
    for p in range(L - R, L):
        buf[p & (R - 1)] = sig[p]
    buf[R:] = buf[:live.RING_MIRROR]
    rings = torch.zeros(2 * S, dtype=torch.float32, device="cuda")
    rings[S:] = torch.from_numpy(buf).cuda()                                  # the stream lives in ring 1
    n = len(starts)
    vring = torch.tensor([1], dtype=torch.int64, device="cuda")
    vhi = torch.tensor([hi], dtype=torch.int64, device="cuda")
    d_fv = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_fs = torch.from_numpy(starts).cuda()
    out = torch.empty((n, 64, 128, 3), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(check(lib.sdfa_frontend_workspace_bytes(n))), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.sdfa_mel_frontend_ring(C.c_void_p(rings.data_ptr()), r, 2, C.c_void_p(vring.data_ptr()), C.c_void_p(vhi.data_ptr()), 1,
                                     C.c_void_p(d_fv.data_ptr()), C.c_void_p(d_fs.data_ptr()), n, sr, C.c_void_p(out.data_ptr()),
                                     C.c_void_p(ws.data_ptr()), ws.numel(), st))
    status = int(check(lib.sdfa_debug_frontend_status(C.c_void_p(ws.data_ptr()), st)))
    torch.cuda.synchronize()
    clips = [sig[:hi]]
    fc = np.zeros(n, np.int32)
    res = compare(ref, clips, fc, starts, out)
    wraps = int(((starts // R) != ((starts + sliding - 1) // R)).sum())
    past_hi = int((starts + sliding > hi).sum())
    return dict(res=res, status=status, finite=bool(torch.isfinite(out).all()), frames=n, wraps=wraps, past_hi=past_hi,
                zeros_ok=bool((out[torch.from_numpy(empty_frames(clips, fc, starts, sliding)).cuda()] == 0).all()))


# ------------------------------------------------------------------------------------------------------------------ measure
def measure():
    from sdfa_amd.engine import FrontendOnly
    fe = FrontendOnly()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = dict(cus=cus, rows=[], ring={}, host={}, geometry={})
    for sr in SRS:
        ref = FrontendRef64(sr, device="cuda")
        sliding = geometry(sr)[2]
        for name, clips, tables, forms in cases(sr):
            for form in forms:
                t0 = time.time()
                got, fc, fs, status = run_form(fe, clips, sr, tables, form)
                t_gpu = time.time() - t0
                res = compare(ref, clips, fc, fs, got)
                empty = torch.from_numpy(empty_frames(clips, fc, fs, sliding)).cuda()
                out["rows"].append(dict(sr=sr, form=form, case=name, frames=len(fs), r=res[0], abs_floor=res[1], abs_rest=res[2],
                                        seconds=time.time() - t0, gpu_seconds=t_gpu, status=status, finite=bool(torch.isfinite(got).all()),
                                        empty=int(empty.sum()), zeros_ok=bool((got[empty] == 0).all())))
                if form == "stream" and name in ("ragged", "bench_batch"):
                    out["geometry"][(sr, name)] = stream_blocks(len(fs), cus)
                if form == "stream" and name == "10s":
                    k = 300
                    out["host"][sr] = dict(clips=[clips[0]], fc=fc[:k], fs=fs[:k], got=got[:k].cpu())
                del got
        out["ring"][sr] = ring_case(sr, ref)
    return out


@pytest.fixture(scope="module")
def measured():
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    out = measure()
    torch.cuda.synchronize()
    out["seconds"] = time.time() - t0
    out["peak_bytes"] = torch.cuda.max_memory_allocated()
    return out


def table(out):
    lines = [f"CUs {out['cus']}  ({out.get('seconds', 0):.0f} s, peak {out.get('peak_bytes', 0) / 2**30:.1f} GiB)",
             f"{'sr':>5s} {'form':10s} {'input':18s} {'frames':>6s} {'r':>6s} {'abs@floor':>9s} {'abs rest':>9s} {'s':>6s}"]
    for x in out["rows"]:
        lines.append(f"{x['sr']:5d} {x['form']:10s} {x['case']:18s} {x['frames']:6d} {x['r']:6.2f} {x['abs_floor']:9.1e} "
                     f"{x['abs_rest']:9.1e} {x['seconds']:6.2f}")
    for sr, x in out["ring"].items():
        r, af, ar = x["res"]
        lines.append(f"{sr:5d} {'ring':10s} {'wrap':18s} {x['frames']:6d} {r:6.2f} {af:9.1e} {ar:9.1e}")
    for sr, h in out.get("sens", {}).items():
        lines.append(f"{sr:5d} sensitivity  " + "  ".join(f"{k} {v:.3g}" for k, v in h.items()))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("sr", SRS)
def test_every_form_against_float64(measured, sr):
    print("\n" + table(measured))
    rows = [x for x in measured["rows"] if x["sr"] == sr and x["form"] != "per_window"]
    worst = max(rows, key=lambda x: x["r"])
    assert worst["r"] <= BOUND_R[sr], worst
    pw = [x for x in measured["rows"] if x["sr"] == sr and x["form"] == "per_window"]
    assert pw and max(x["r"] for x in pw) <= BOUND_R_PER_WINDOW[sr], pw
    assert measured["ring"][sr]["res"][0] <= BOUND_R[sr], measured["ring"][sr]


def test_exact_zeros_finite_and_status(measured):
    for x in measured["rows"]:
        assert x["finite"] and x["zeros_ok"], x
        if x["form"] == "repair":
            assert x["status"] > 0, x                       # the forced bound expired waits: the repair pass ran
        elif x["status"] is not None:
            assert x["status"] == 0, x
    assert any(x["case"] == "zeros" and x["empty"] == x["frames"] for x in measured["rows"])
    assert any(x["case"] == "hand_table" and 0 < x["empty"] < x["frames"] for x in measured["rows"])
    for sr, x in measured["ring"].items():
        assert x["finite"] and x["zeros_ok"] and x["status"] == 0, (sr, x)


def test_inputs_reach_every_form(measured):
    """What the inputs should reach, by the launch rules as this module restates them -- not a record of what the kernels
    launched: every form ran at each rate; by stream_blocks (a copy of frontend.hip stream_geometry, to be kept in step with
    it) the stream's grid has more than 8 blocks, a partial last block and an nb8 pad; the ring frames cross the wrap point
    and the valid end; WIN = 512 at 8 kHz, whose transform has a radix-2 stage after the radix-4 ones (log2 512 is odd).
    The forced repair is the one reach the kernels report themselves: its status word counts expired waits
    (test_exact_zeros_finite_and_status)."""
    for sr in SRS:
        forms = {x["form"] for x in measured["rows"] if x["sr"] == sr}
        assert forms == {f for f in FORMS if f != "radix4" or sr == 16000}, (sr, forms)
        ring = measured["ring"][sr]
        assert ring["wraps"] > 0 and ring["past_hi"] > 0, ring
    g = measured["geometry"]
    for key, (B, nb, nb8) in g.items():
        assert nb > 8, (key, B, nb)
    assert any(nb8 > nb for _, nb, nb8 in g.values()), g
    rows = {(x["sr"], x["case"]): x["frames"] for x in measured["rows"] if x["form"] == "stream"}
    assert any(rows[k] % g[k][0] for k in g), (rows, g)
    assert rows[(16000, "bench_batch")] == 20352
    win = geometry(8000)[0]
    assert win == 512 and int(math.log2(win)) % 2 == 1


@pytest.mark.parametrize("name", list(PERTURBATIONS))
def test_bound_catches(measured, name):
    """The GPU's output of the first 300 frames of the 10 s clip (frames before the clip, long chains) misses the perturbed
    reference by more than SENS_MARGIN times the bound, at both rates; against the unperturbed reference it is within the bound."""
    for sr in SRS:
        h = measured["host"][sr]
        ref = FrontendRef64(sr, device="cuda")
        good = compare(ref, h["clips"], h["fc"], h["fs"], h["got"])[0]
        bad = compare(ref, h["clips"], h["fc"], h["fs"], h["got"], **PERTURBATIONS[name])[0]
        measured.setdefault("sens", {}).setdefault(sr, {})[name] = bad
        assert good <= BOUND_R[sr] and bad > SENS_MARGIN * BOUND_R[sr], (sr, name, good, bad)


if __name__ == "__main__":
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    res = measure()
    for sr in SRS:
        h = res["host"][sr]
        ref = FrontendRef64(sr, device="cuda")
        res.setdefault("sens", {})[sr] = {k: compare(ref, h["clips"], h["fc"], h["fs"], h["got"], **kw)[0] for k, kw in PERTURBATIONS.items()}
    torch.cuda.synchronize()
    res["seconds"], res["peak_bytes"] = time.time() - t0, torch.cuda.max_memory_allocated()
    print(table(res))
    for sr in SRS:
        rows = [x for x in res["rows"] if x["sr"] == sr]
        print(sr, "max r", max(x["r"] for x in rows), "ring", res["ring"][sr]["res"][0],
              {f: max(x["r"] for x in rows if x["form"] == f) for f in {x["form"] for x in rows}})
    print("status", [(x["sr"], x["form"], x["case"], x["status"]) for x in res["rows"] if x["status"]], "geometry", res["geometry"])
