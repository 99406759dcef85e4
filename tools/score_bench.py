"""Validation losses on the MI355X: sdfa_amd.score.score_rows on the headline batch's dgrad rows against
its byte floor, and the same scalars from the reference's criterion written as torch operations on the same device tensors in
the same process.  bench.py (the headline workload) is not involved.

  python tools/score_bench.py --out profiles/score_bench.json

Rows      --frames (20,352) x 89,784 float32 prediction rows (7.3 GB) in --clips (32) clips, built on the device from the
          synthetic head as tools/pca_fit_bench.py builds rows; a 60 fps track of the same width, one more row than frames per
          clip, built the same way from another seed.  Frame f of a clip blends track rows f and f + 1 with a per-clip fraction.
Timed     score_rows (marking, the scoring kernel, the sum of its partials) by device events after a warm-up call; median of --reps.
Floor     (prediction bytes + track bytes, each once) / 6.29 TB/s, the measured float4 copy rate of the part.
Baseline  PLoss and MLoss as criterion.py writes them -- blend, view as triangles, exp of the rotat part, mse_loss, sum over the
          last dimension, means, the weighted batch mean -- on the collated batch [a; b] of each clip, clip by clip (the whole
          batch's temporaries, several times 7.3 GB, are not attempted), by device events after a warm-up on the first clip."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_RATE = 6.29e12          # bytes/s, float4 copy measured on the MI355X


def torch_criterion(pred, track, src, w, off):
    """The reference's scalars per clip with torch operations (float32, as the reference computes them)."""
    import torch
    import torch.nn.functional as Fn
    out = []
    for c in range(len(off) - 1):
        f0, f1 = int(off[c]), int(off[c + 1])
        fc = f1 - f0
        truth = track[src[f0:f1, 0]] * w[f0:f1, 0:1] + track[src[f0:f1, 1]] * w[f0:f1, 1:2]
        a = torch.cat((torch.arange(fc - 1), torch.tensor([fc - 2]))).to(pred.device)
        b = torch.cat((torch.arange(1, fc), torch.tensor([fc - 1]))).to(pred.device)
        idx = torch.cat((a, b))
        P = pred[f0:f1][idx].view(2 * fc, 1, -1, 9)
        T = truth[idx].view(2 * fc, 1, -1, 9)
        weights = torch.ones(2 * fc, device=pred.device)
        res = {}
        for tag, sl in (("s", slice(0, 6)), ("r", slice(6, 9))):
            x, y = P[..., sl], T[..., sl]
            if x.size(-1) == 3:
                x, y = torch.exp(x), torch.exp(y)
            loss = Fn.mse_loss(x, y, reduction="none").sum(-1)
            while loss.dim() > 1:
                loss = loss.mean(-1)
            res["scalar_p" + tag] = (loss * weights).mean(dim=0)
            m = Fn.mse_loss(x[fc:] - x[:fc], y[fc:] - y[:fc], reduction="none").sum(-1)
            while m.dim() > 1:
                m = m.mean(-1)
            res["scalar_m" + tag] = (m * (weights[fc:] + weights[:fc])).mean(dim=0)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=20352)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    args = ap.parse_args()
    import torch
    from sdfa_amd import score
    from pca_fit_bench import build_rows
    assert torch.cuda.is_available(), "score_bench needs the MI355X"
    assert args.frames % args.clips == 0
    fc = args.frames // args.clips
    pred = build_rows(args.frames, seed=0)
    track = build_rows(args.frames + args.clips, seed=1)
    F, W = pred.shape
    off = np.arange(args.clips + 1, dtype=np.int64) * fc
    src = np.zeros((F, 2), np.int64)
    wts = np.zeros((F, 2), np.float32)
    for c in range(args.clips):
        src[off[c]:off[c + 1], 0] = off[c] + c + np.arange(fc)
        a = np.float32((0.37 + 0.017 * c) % 1.0)
        wts[off[c]:off[c + 1]] = (np.float32(1.0 - float(a)), a)
    src[:, 1] = src[:, 0] + 1
    d_src, d_w = torch.from_numpy(src).cuda(), torch.from_numpy(wts).cuda()
    torch.cuda.synchronize()

    score.score_rows(pred[:2 * fc], track, d_src[:2 * fc], d_w[:2 * fc], off[:3], score.LAYOUT_DGRAD)      # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rec = score.score_rows(pred, track, d_src, d_w, off, score.LAYOUT_DGRAD)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ours = score.clip_scalars(rec, off, W // 9)
    bytes_once = 4.0 * W * (F + track.shape[0])
    floor_ms = 1e3 * bytes_once / COPY_RATE
    report = {"frames": F, "clips": args.clips, "row_width": W, "track_rows": int(track.shape[0]), "reps": args.reps, "score_rows_ms": ms,
              "score_rows_ms_median": statistics.median(ms), "bytes_each_once": bytes_once, "copy_rate_bytes_per_s": COPY_RATE,
              "floor_ms": floor_ms, "ratio_to_floor": statistics.median(ms) / floor_ms,
              "achieved_bytes_per_s": bytes_once / (statistics.median(ms) / 1e3), "corpus": ours["corpus"]}

    torch_criterion(pred, track, d_src, d_w, off[:2])                                                      # warm-up
    torch.cuda.synchronize()
    tms = []
    for _ in range(max(1, min(args.reps, 3))):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        base = torch_criterion(pred, track, d_src, d_w, off)
        e1.record()
        torch.cuda.synchronize()
        tms.append(e0.elapsed_time(e1))
    worst = 0.0
    for b, o in zip(base, ours["clips"]):
        for k, v in b.items():
            worst = max(worst, abs(float(v) / o[k] - 1))
    report["torch_baseline"] = {"ms": tms, "ms_median": statistics.median(tms), "how": "per clip (the collated batch [a; b] of one clip at a time)",
                                "speedup": statistics.median(tms) / statistics.median(ms), "max_relative_gap_to_score_rows": worst}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
