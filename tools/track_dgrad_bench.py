"""Temporal track filters and the offsets -> dgrad dataset step on the MI355X.  bench.py (the headline
workload) is not involved.

  python tools/track_dgrad_bench.py --out profiles/track_dgrad_bench.json

Filters   sdfa_amd.tfilter on 600 x 15,069 (one offsets clip, dword form) and on --frames (20,352) x 89,784 (the headline
          batch's dgrad rows in 32 clips, float4 form): the FIR with scipy's sigma = 1 taps (radius 4) and the bilateral filter at
          the reference's radius 5, each in the register-window and in the generic form.  Device events around --launches
          back-to-back launches after a warm-up launch; --rounds rounds with the forms alternating; median and minimum per launch.
Floor     every element read once and written once, F W 8 bytes, at the rate of a device-to-device copy of the same rows measured
          the same way in the same process.
Host      scipy.ndimage.gaussian_filter1d(x, 1, axis=0) on the 600 x 15,069 clip, wall clock, best of 3.
Dataset   speech_anime.datasets.dgrad.generate_dgrad on a synthetic tree of --clips (40) clips x --clip_frames (240) frames of one
          speaker (the FLAME template of tests/golden/mesh_flame.npz) in a temporary directory: wall clock, clips per second."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))


def timed(fn, launches):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def bench_shape(F, W, n_clips, launches, rounds, seed):
    import torch
    from sdfa_amd import tfilter
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(F, W, device="cuda", generator=g) * 2e-3
    out = torch.empty_like(x)
    off = (np.arange(n_clips + 1, dtype=np.int64) * F) // n_clips
    taps = tfilter.gaussian_taps(1.0)
    arms = {
        "copy": lambda: out.copy_(x),
        "fir_window": lambda: tfilter.correlate_symmetric(x, taps, off, out=out),
        "fir_generic": lambda: tfilter.correlate_symmetric(x, taps, off, out=out, generic=True),
        "bilateral_window": lambda: tfilter.bilateral(x, 1.0, 2e-3, 5, clip_frame_off=off, out=out),
        "bilateral_generic": lambda: tfilter.bilateral(x, 1.0, 2e-3, 5, clip_frame_off=off, out=out, generic=True),
    }
    ms = {k: [] for k in arms}
    for fn in arms.values():                                  # warm-up: code objects, first touch of out
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn, launches))
    byts = 8.0 * F * W
    copy_rate = byts / (statistics.median(ms["copy"]) / 1e3)
    rep = {"frames": F, "row_width": W, "clips": n_clips, "form": "float4" if W % 4 == 0 else "dword", "launches_per_timing": launches,
           "rounds": rounds, "bytes_read_once_written_once": byts, "copy_ms": ms["copy"], "copy_rate_bytes_per_s": copy_rate}
    for k in list(arms)[1:]:
        med = statistics.median(ms[k])
        rep[k] = {"ms": ms[k], "ms_median": med, "ms_min": min(ms[k]), "ratio_to_copy_floor": med / statistics.median(ms["copy"]),
                  "achieved_bytes_per_s": byts / (med / 1e3)}
    rep["fir_window_over_generic"] = rep["fir_window"]["ms_median"] / rep["fir_generic"]["ms_median"]
    rep["bilateral_window_over_generic"] = rep["bilateral_window"]["ms_median"] / rep["bilateral_generic"]["ms_median"]
    del x, out
    torch.cuda.empty_cache()
    return rep


def host_scipy(F, W):
    from scipy.ndimage import gaussian_filter1d
    x = (np.random.RandomState(0).normal(0, 2e-3, (F, W))).astype(np.float32)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        gaussian_filter1d(x, 1, axis=0)
        best = min(best, time.perf_counter() - t0)
    return {"frames": F, "row_width": W, "ms_best_of_3": 1e3 * best}


def dataset_step(clips, clip_frames):
    import torch
    from speech_anime.datasets.dgrad import generate_dgrad
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_flame.npz"))
    V, faces = g["verts"].astype(np.float32), g["faces"]
    tmp = tempfile.mkdtemp(prefix="track_dgrad_bench_")
    try:
        src, dst = os.path.join(tmp, "offsets"), os.path.join(tmp, "dgrad")
        rs = np.random.RandomState(1)
        k = rs.normal(0, 1, (3, 3)) * 20.0
        base = np.sin(V.astype(np.float64) @ k)
        for c in range(clips):
            d = os.path.join(src, "data", "m0", "neutral", f"{c:03d}")
            os.makedirs(d)
            ph = rs.uniform(0, 6.28)
            for f in range(clip_frames):
                np.save(os.path.join(d, f"{f:06d}.npy"), (2e-3 * np.sin(0.2 * f + ph) * base).astype(np.float32).reshape(-1))
            np.save(os.path.join(d, "000000_lips_dist.npy"), np.float32(0.004))
            with open(d + "_audio", "wb") as fp:
                fp.write(b"\0" * 1024)
        for name in ("train.csv", "valid.csv"):
            with open(os.path.join(src, name), "w") as fp:
                fp.write("npy_data_path:path\n")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = generate_dgrad(src, dst, {"m0": (V, faces)})
        wall = time.perf_counter() - t0
        assert len(done) == clips
        return {"clips": clips, "frames_per_clip": clip_frames, "wall_s": wall, "clips_per_s": clips / wall,
                "frames_per_s": clips * clip_frames / wall, "note": "reads 60 KB and writes 359 KB .npy files per frame on the host"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=20352)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=40)
    ap.add_argument("--clip_frames", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_dgrad_bench.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "track_dgrad_bench needs the MI355X"
    report = {"device": torch.cuda.get_device_name(0)}
    report["offsets_clip"] = bench_shape(600, 15069, 1, max(args.launches, 50), args.rounds, 0)
    report["dgrad_batch"] = bench_shape(args.frames, 89784, 32, args.launches, args.rounds, 1)
    report["scipy_host"] = host_scipy(600, 15069)
    report["scipy_host"]["speedup_of_fir_window"] = report["scipy_host"]["ms_best_of_3"] / report["offsets_clip"]["fir_window"]["ms_median"]
    report["generate_dgrad"] = dataset_step(args.clips, args.clip_frames)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
