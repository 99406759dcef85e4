"""Timing of mesh -> dgrad (sdfa_mesh_deform_grad) at FLAME size: the kernel on 600 frames (10 s at 60 fps) in float32 and float64
output, the offsets-head retarget route of one 10 s clip (deform_grad of the offsets rows + the template's solve), and -- where
oracle/_ref holds the reference's compiled module -- its get_deform_grad for one frame on the host.  Prints one JSON line.

    python tools/deform_grad_bench.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
from sdfa_amd.mesh import DeformGrad, MeshSolver  # noqa: E402
from speech_anime.datasets.vocaset_mask import non_face_tris, non_face_verts  # noqa: E402


def _time(fn, reps=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_flame.npz"))
    V, F = g["verts"], g["faces"]
    frames = 600
    rs = np.random.RandomState(0)
    offs = torch.from_numpy((rs.normal(0, 1e-3, (frames, len(V), 3))).astype(np.float32)).cuda()
    dg = DeformGrad(V, F, tri_mask=non_face_tris(F))
    out32 = torch.empty((frames, len(F) * 9), device="cuda")
    out64 = torch.empty((frames, len(F) * 9), device="cuda", dtype=torch.float64)
    res = {"frames": frames, "tris": int(len(F))}
    res["kernel_f32_ms"] = _time(lambda: dg(offs, offsets=True, out=out32))
    res["kernel_f64_ms"] = _time(lambda: dg(offs, offsets=True, dtype=torch.float64, out=out64))
    solver = MeshSolver(V, F, non_face_verts())
    res["retarget_10s_ms"] = _time(lambda: solver.get_mesh(dg(offs, offsets=True, out=out32)), reps=5)
    ref = os.path.join(ROOT, "oracle", "_ref")
    if os.path.isdir(ref):
        sys.path.insert(0, ref)
        try:
            import deformation as D
            tgt = (V + offs[0].cpu().numpy()).astype(np.float32)
            D.get_deform_grad(V, tgt, F, 1e-6)
            t0 = time.perf_counter()
            for _ in range(5):
                D.get_deform_grad(V, tgt, F, 1e-6)
            res["reference_host_ms_per_frame"] = (time.perf_counter() - t0) / 5 * 1e3
        except ImportError as e:
            res["reference_host_ms_per_frame"] = f"unavailable: {e}"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
