"""PCA fit on the MI355X: `sdfa_amd.pca.fit_dgrad` end to end on dgrad rows of the headline batch, and
what each pass over the rows costs against its floor.  bench.py (the headline workload) is not involved.

  python tools/pca_fit_bench.py --out profiles/pca_fit_bench.json

Rows     --frames (20,352) x 89,784 float32 (7.3 GB), built on the device from the synthetic head: means + coef compT^T per
         branch, interleaved as the regressor writes them, coef_i ~ N(0, decay^i), plus seeded noise worth about 1 % of the
         variance, so that 0.97 is a real threshold.
Timed    fit_dgrad (two fits, scale then rotat) by device events and by a host clock around the synchronising call, after a
         warm-up fit on the first 256 rows (code objects, allocator); median of --reps.
Passes   a sweep reads the rows twice: Z = Xc Q and Y = Xc^T Z.  The library times both on the device in the last sweep
         (PcaFit.z_pass_ms / y_pass_ms).  Bytes and FLOPs per pass are computed from the shapes here; the floor of a pass is the
         larger of bytes / HBM peak and FLOPs / fp32-MFMA peak, and the report says which one binds.
Host     numpy's float64 SVD of the centred scale columns of the largest leading subset of frames (256, 512, ...) that
         finishes inside --host_budget seconds (40, recorded in the report): the reference's route (sklearn's full PCA is this SVD) at that size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

HBM_PEAK = 8.0e12            # bytes/s, specification
MFMA_F32_PEAK = 157.3e12     # FLOP/s, v_mfma_f32_32x32x2_f32, specification
N_TRI = 9976


def build_rows(frames, seed=0, decay=0.93, noise_share=0.01, step=1024):
    import torch
    from sdfa_amd import synth
    sd = synth.make_state_dict("dgrad", 1234)
    rows = torch.empty(frames, N_TRI, 9, dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    for name, per, lo in (("scale", 6, 0), ("rotat", 3, 6)):
        compT = torch.from_numpy(next(v for k, v in sd.items() if k.endswith(f"_{name}_pca.compT"))).cuda()
        means = torch.from_numpy(next(v for k, v in sd.items() if k.endswith(f"_{name}_pca.means"))).cuda()
        nc = compT.shape[1]
        scale = decay ** torch.arange(nc, dtype=torch.float32, device="cuda")
        # signal variance per entry: sum_i scale_i^2 * 0.02^2 (compT ~ N(0, 0.02)); the noise gets noise_share of the total
        signal = float((scale ** 2).sum()) * 0.02 ** 2
        sigma = (signal * noise_share / (1.0 - noise_share)) ** 0.5
        for r0 in range(0, frames, step):
            n = min(step, frames - r0)
            coef = torch.randn(n, nc, generator=g, device="cuda") * scale
            part = means + coef @ compT.t() + sigma * torch.randn(n, N_TRI * per, generator=g, device="cuda")
            rows[r0:r0 + n, :, lo:lo + per] = part.reshape(n, N_TRI, per)
    return rows.reshape(frames, N_TRI * 9)


def pass_model(F, D, W, b, ms, which):
    """Bytes and FLOPs of one pass from its shapes, and its time against the larger floor."""
    flops = 2.0 * F * D * b
    rows_bytes = 4.0 * F * D                       # the selected columns, each read once
    small_bytes = 4.0 * (F * b + D * b)            # Z and Q (pass Z) or Z and Y (pass Y), each once
    t_hbm, t_mfma = (rows_bytes + small_bytes) / HBM_PEAK, flops / MFMA_F32_PEAK
    floor = max(t_hbm, t_mfma)
    return {"pass": which, "block": b, "ms": ms, "flops": flops, "bytes": rows_bytes + small_bytes, "row_bytes_at_line_granularity": 4.0 * F * W,
            "floor_ms_hbm": 1e3 * t_hbm, "floor_ms_mfma_f32": 1e3 * t_mfma, "binds": "fp32 MFMA" if t_mfma >= t_hbm else "HBM",
            "share_of_floor": (1e3 * floor / ms) if ms > 0 else None, "tflops": flops / ms / 1e9 if ms > 0 else None}


def host_baseline(rows, budget_s):
    """numpy float64 SVD of the centred scale columns of the first n frames, n doubling while the next size is expected to fit."""
    cols = (np.arange(N_TRI * 6) // 6) * 9 + np.arange(N_TRI * 6) % 6
    out, n, spent = None, 256, 0.0
    while n <= rows.shape[0]:
        x = rows[:n].cpu().numpy()[:, cols].astype(np.float64)
        t0 = time.perf_counter()
        xc = x - x.mean(axis=0)
        s = np.linalg.svd(xc, full_matrices=False)[1]
        dt = time.perf_counter() - t0
        spent += dt
        ratio = np.cumsum(s * s) / (s * s).sum()
        out = {"frames": n, "columns": int(x.shape[1]), "seconds": dt, "k_at_0.97": int(np.searchsorted(ratio, 0.97, side="right") + 1),
               "label": "the reference's route (numpy float64 SVD of the centred rows, as sklearn's full PCA) at this size"}
        if spent + 4.5 * dt > budget_s:          # the SVD of an n x D matrix, n << D, costs ~ n^2 D: four times per doubling
            break
        n *= 2
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=20352)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--n_components", type=float, default=0.97)
    ap.add_argument("--host_budget", type=float, default=40.0, help="seconds the host baseline may take in all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_fit_bench.json"))
    args = ap.parse_args()
    import torch
    from sdfa_amd import pca
    assert torch.cuda.is_available(), "pca_fit_bench needs the MI355X"
    rows = build_rows(args.frames)
    torch.cuda.synchronize()
    F, W = rows.shape
    pca.fit_dgrad(rows[:256])                      # warm-up
    runs = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fits = pca.fit_dgrad(rows, args.n_components)
        e1.record()
        torch.cuda.synchronize()
        runs.append({"host_s": time.perf_counter() - t0, "device_event_s": e0.elapsed_time(e1) / 1e3})
    report = {"frames": F, "row_width": W, "row_bytes": 4.0 * F * W, "n_components": args.n_components, "reps": args.reps, "runs": runs,
              "fit_dgrad_host_s_median": statistics.median(r["host_s"] for r in runs),
              "fit_dgrad_event_s_median": statistics.median(r["device_event_s"] for r in runs),
              "peaks": {"hbm_bytes_per_s": HBM_PEAK, "mfma_f32_flop_per_s": MFMA_F32_PEAK}, "fits": {}}
    for name, fit in zip(("scale", "rotat"), fits):
        D = pca.selected_dim(W, fit.select)
        report["fits"][name] = {"D": D, "k": fit.k, "block": fit.block, "sweeps": fit.sweeps, "max_residual": fit.max_residual,
                                "explained": float(fit.explained_variance_ratio.double().sum()),
                                "passes": [pass_model(F, D, W, fit.block, fit.z_pass_ms, "Z = Xc Q"), pass_model(F, D, W, fit.block, fit.y_pass_ms, "Y = Xc^T Z")]}
    report["host_baseline"] = dict(host_baseline(rows, args.host_budget), budget_s=args.host_budget)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
