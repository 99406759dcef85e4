"""Generates tests/golden/deform_grad.npz: mesh -> dgrad cases computed by the REFERENCE'S OWN compiled module
(deformation.get_deform_grad, built into oracle/_ref by oracle/build_ref.sh).  Build container only:

    python tests/gen_golden_deform_grad.py

The vendored pybind11 of that module predates NumPy 2: the float64 array it returns carries a zero stride although its buffer
holds the n_tris*9 values in order, so the values are read back through the buffer's real stride (`_ref_dgrad`).

Cases (every target float32, as the binding casts its inputs):
  flame_*     the FLAME template of mesh_flame.npz: smooth speech-sized (1 mm) and 1 cm offset fields, rigid rotations by 10, 90 and
              179.9 degrees; reference rows kept for every 10th triangle (the file stays small)
  preload     preload.py:768-779: float32 template + offsets, then the non-face triangles zeroed
  small_*     small random meshes with collinear and coincident-vertex (zero-area) triangles, mirrored targets (det < 0), rotations
              near both 1e-6 branches of rotation_log_exp::log, at eps 1e-6 and 1e-2
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
FLAME_STRIDE = 10


def _ref_module():
    subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
    import deformation
    return deformation


def _ref_dgrad(D, a, b, faces, eps):
    r = D.get_deform_grad(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32),
                          np.ascontiguousarray(faces, np.uint32), eps)
    return np.lib.stride_tricks.as_strided(r, r.shape, (r.itemsize,)).copy()


def rotation(deg, axis):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    th = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rotation_rad(rad, axis):
    return rotation(np.rad2deg(rad), axis)


def smooth_field(V, amp, seed):
    rs = np.random.RandomState(seed)
    k = rs.normal(0, 1, (3, 3)) * 20.0
    ph = rs.uniform(0, 2 * np.pi, 3)
    return (amp * np.sin(V.astype(np.float64) @ k + ph)).astype(np.float32)


def small_mesh(rs, n_verts=48, n_tris=80):
    V = rs.normal(0, 1, (n_verts, 3)).astype(np.float32)
    F = np.stack([rs.choice(n_verts, 3, replace=False) for _ in range(n_tris)]).astype(np.uint32)
    # collinear: vertex c on the segment a-b (exact in float32: the midpoint of integers)
    for t in range(0, 6):
        a, b, c = 3 * t, 3 * t + 1, 3 * t + 2
        V[a] = rs.randint(-4, 5, 3); V[b] = rs.randint(-4, 5, 3)
        V[b] += (V[a] == V[b]).astype(np.float32)
        V[c] = (V[a] + V[b]) / 2
        F[t] = (a, b, c)
    F[6] = (18, 19, 20)
    V[20] = V[18]                                            # coincident vertices: zero area, zero-length edge
    F[7] = (21, 22, 23)                                      # sliver: |cos| ~ 0.995, degenerate at eps 1e-2 only
    V[21] = (0, 0, 0); V[22] = (1, 0, 0); V[23] = (1, 0.1, 0)
    return V, F


def main():
    D = _ref_module()
    from speech_anime.datasets.vocaset_mask import non_face_verts
    g = np.load(os.path.join(HERE, "golden", "mesh_flame.npz"))
    V, F = g["verts"], g["faces"]
    out = {"flame_faces_stride": np.int64(FLAME_STRIDE)}
    meta = {}
    tgts, names = [], []
    for name, amp, seed in (("speech", 1e-3, 1), ("1cm", 1e-2, 2)):
        tgts.append(V + smooth_field(V, amp, seed)); names.append(name)
    for deg in (10.0, 90.0, 179.9):
        tgts.append((V.astype(np.float64) @ rotation(deg, [0.3, 1.0, 0.2]).T).astype(np.float32)); names.append(f"rot{deg:g}")
    out["flame_targets"] = np.stack(tgts)
    out["flame_names"] = np.array(names)
    out["flame_dgrad"] = np.stack([_ref_dgrad(D, V, t, F, 1e-6).reshape(-1, 9)[::FLAME_STRIDE] for t in tgts])

    # preload.py:768-779 -- template + offsets in float32, get_deform_grad, non-face triangles zeroed, float32 rows
    nf = np.zeros(len(V), bool); nf[non_face_verts()] = True
    mask = nf[F].all(1)
    meta["non_face_tris"] = int(mask.sum())
    offs = smooth_field(V, 2e-3, 3)
    dg = _ref_dgrad(D, V, V + offs, F, 1e-6).reshape(-1, 9)
    dg[mask] = 0
    out["preload_offsets"] = offs
    out["preload_dgrad"] = dg[::FLAME_STRIDE]
    out["preload_rows_f32"] = dg.flatten(order="C").astype(np.float32)[: 9 * 997]      # the first 997 triangles as preload saves them

    rs = np.random.RandomState(7)
    Vs, Fs = small_mesh(rs)
    frames = []
    frames.append(Vs + rs.normal(0, 0.05, Vs.shape).astype(np.float32))                     # general
    frames.append((Vs * np.array([-1, 1, 1], np.float32)))                                  # mirrored: det < 0, equal singular values
    frames.append((Vs.astype(np.float64) @ (np.diag([-1.0, 1.0, 1.0]) @ np.diag([1.5, 1.2, 0.7])).T).astype(np.float32))   # mirrored stretch
    for ang in (1e-6 * 0.999, 1e-6 * 1.001, 1e-6 * 5, np.pi - 1e-6 * 0.999, np.pi - 1e-6 * 1.001, np.pi - 1e-5, 3.0):
        frames.append((Vs.astype(np.float64) @ rotation_rad(ang, [0.2, -0.5, 1.0]).T).astype(np.float32))
    frames.append(Vs.copy())                                                                # identity
    out["small_src"] = Vs
    out["small_faces"] = Fs
    out["small_targets"] = np.stack(frames)
    out["small_eps"] = np.array([1e-6, 1e-2])
    out["small_dgrad"] = np.stack([np.stack([_ref_dgrad(D, Vs, t, Fs, e) for t in frames]) for e in (1e-6, 1e-2)])
    path = os.path.join(HERE, "golden", "deform_grad.npz")
    np.savez_compressed(path, **out)
    meta["bytes"] = os.path.getsize(path)
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
