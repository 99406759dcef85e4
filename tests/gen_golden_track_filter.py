"""Generates tests/golden/track_filter.npz and META_track_filter.json.  Build container only (it reads the reference):

    python -B tests/gen_golden_track_filter.py

(a) bilateral_*  the reference's BilateralFilter1D (saber/utils/bilateral.py, loaded from its file by path: it needs only numpy,
    math and tqdm) on float32 signals of F in {1, 2, 5, 6, 11, 23} frames x 7 columns, amplitudes 1 and 1e-3, with the two
    parameter sets of preload.py:151-152, (distance_sigma, range_sigma, radius) = (1, 1, 5) and (5, 2, 10).  Run on float64
    copies of the signals -- the exact double evaluation, `bilateral_out64` -- and on the float32 signals themselves
    (`bilateral_out32`: under NumPy 2 that run accumulates in float32).
(b) dgrad_*      the literal preload.py:768-779,819 recipe -- scipy.ndimage.gaussian_filter1d(frames, sigma=1, axis=0), float32
    template + offsets, the reference's compiled get_deform_grad (oracle/_ref, built by oracle/build_ref.sh), non-face triangles
    zeroed, float32 rows -- on one FLAME clip (tests/golden/mesh_flame.npz) of 6 frames of smooth 2 mm offsets.  Kept: the
    offsets and every 10th triangle of the float32 rows.
(c) META: the largest |float32 run - float64 run| / max|signal| seen in (a)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
REFERENCE_ROOT = os.environ.get("SDFA_REFERENCE_ROOT", "/root/reference")
STRIDE = 10
FRAMES = (1, 2, 5, 6, 11, 23)
COLUMNS = 7
PARAMS = ((1.0, 1.0, 5), (5.0, 2.0, 10))            # distance_sigma, range_sigma, radius (preload.py:151-152)
AMPS = (1.0, 1e-3)


def _bilateral_class():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_bilateral", os.path.join(REFERENCE_ROOT, "saber", "utils", "bilateral.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BilateralFilter1D


def _ref_module():
    subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
    import deformation
    return deformation


def _ref_dgrad(D, a, b, faces, eps):
    """The vendored pybind11 predates NumPy 2: the returned array carries a zero stride (tests/gen_golden_deform_grad.py)."""
    r = D.get_deform_grad(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32),
                          np.ascontiguousarray(faces, np.uint32), eps)
    return np.lib.stride_tricks.as_strided(r, r.shape, (r.itemsize,)).copy()


def signal(F, amp, seed):
    """A speech-like column set: a slow wave plus jitter and one step, float32 (F, COLUMNS)."""
    rs = np.random.RandomState(seed)
    t = np.arange(F)[:, None]
    x = np.sin(0.45 * t + rs.uniform(0, 6.28, COLUMNS)) + 0.3 * rs.normal(0, 1, (F, COLUMNS)) + (t >= F // 2) * rs.normal(0, 1, COLUMNS)
    return (amp * x).astype(np.float32)


def smooth_field(V, amp, seed):
    rs = np.random.RandomState(seed)
    k = rs.normal(0, 1, (3, 3)) * 20.0
    ph = rs.uniform(0, 2 * np.pi, 3)
    return amp * np.sin(V.astype(np.float64) @ k + ph)


def main():
    out, meta = {}, {}
    B = _bilateral_class()
    worst = 0.0
    sigs, o64, o32, index = [], [], [], []
    for pi, (ds, rs_, r) in enumerate(PARAMS):
        filt = B(-0.5, ds, rs_, r)
        for ai, amp in enumerate(AMPS):
            for F in FRAMES:
                x = signal(F, amp, 100 * pi + 10 * ai + F)
                a = np.asarray(filt(x.astype(np.float64)), np.float64)
                b = np.asarray(filt(x), np.float32)
                worst = max(worst, float(np.abs(b.astype(np.float64) - a).max() / np.abs(x).max()))
                index.append((pi, ai, F))
                sigs.append(x); o64.append(a); o32.append(b)
    out["bilateral_params"] = np.asarray(PARAMS, np.float64)
    out["bilateral_amps"] = np.asarray(AMPS, np.float64)
    out["bilateral_index"] = np.asarray(index, np.int64)                 # (parameter set, amplitude, frames) per case
    out["bilateral_signal"] = np.concatenate(sigs)                       # the cases one after the other
    out["bilateral_out64"] = np.concatenate(o64)
    out["bilateral_out32"] = np.concatenate(o32)
    meta["bilateral_f32_vs_f64_rel"] = worst

    from scipy.ndimage import gaussian_filter1d
    from speech_anime.datasets.vocaset_mask import non_face_verts
    D = _ref_module()
    g = np.load(os.path.join(HERE, "golden", "mesh_flame.npz"))
    V, faces = g["verts"], g["faces"]
    nf = np.zeros(len(V), bool); nf[non_face_verts()] = True
    mask = nf[faces].all(1)
    f0, f1 = smooth_field(V, 2e-3, 11), smooth_field(V, 2e-3, 12)
    frames = [(np.sin(0.9 * t) * f0 + np.cos(0.6 * t + 0.4) * f1).astype(np.float32).reshape(-1) for t in range(6)]
    template = V.astype(np.float32)
    smoothed = gaussian_filter1d(frames, sigma=1, axis=0)                # preload.py:819
    rows = []
    for offsets in smoothed:                                             # preload.py:768-779
        offsets = np.reshape(offsets, (-1, 3))
        verts = template + offsets
        dg = _ref_dgrad(D, template, verts, faces, 1e-6)
        dg = np.reshape(dg, (-1, 9))
        dg[mask] = 0
        rows.append(dg.flatten(order="C").astype(np.float32))
    rows = np.stack(rows)
    out["dgrad_offsets"] = np.stack(frames)
    out["dgrad_stride"] = np.int64(STRIDE)
    out["dgrad_rows"] = rows.reshape(len(rows), -1, 9)[:, ::STRIDE]
    meta["dgrad_frames"] = len(rows)
    meta["non_face_tris"] = int(mask.sum())

    path = os.path.join(HERE, "golden", "track_filter.npz")
    np.savez_compressed(path, **out)
    meta["bytes"] = os.path.getsize(path)
    import scipy
    meta["numpy"], meta["scipy"] = np.__version__, scipy.__version__
    with open(os.path.join(HERE, "golden", "META_track_filter.json"), "w") as fp:
        json.dump(meta, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
