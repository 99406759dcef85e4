"""numpy float32 restatement of the rasterizer in sdfa-2019_amd/csrc/render.hip (contract: include/sdfa_render.h).

The vertex stage and the raster / depth stage are written with explicit element-wise float32 operations in the kernel's
order (no BLAS, no fused multiply-add), so snapped screen positions and the visibility buffer are reproduced bit for
bit; the shading stage follows the same formulas (the GPU tests allow +-1 per channel there).

A restatement agrees with the kernel on a wrong rule, so this file is itself held to an independent float64 ray caster
(tests/render_ref64.py: no edge functions, no snapping, no fp32) by tests/test_render_ref64_cpu.py: visibility of every sample
outside 1/256 pixel of a projected edge, colour within a per-pixel bound formed from the reference alone, and seven patched
copies of this source (winding, y flip, aspect, depth order, affine interpolation, channel order, normals mode) that the
comparison must reject."""
import math

import numpy as np

F32 = np.float32
INT_MAX = 2 ** 31 - 1
GUARD_PX = 32768.0

# the reference's rig (speech_anime/viewer/render_py.py:13-23) and pyrender's camera defaults
DEFAULT_PARAMS = dict(
    cam_pose=np.array([[9.84561989e-01, -1.14640632e-02, 1.74657155e-01, 7.99997887e-02],
                       [-2.63421926e-08, 9.97852584e-01, 6.54966148e-02, 3.00000020e-02],
                       [-1.75033820e-01, -6.44855109e-02, 9.82448868e-01, 4.49999897e-01],
                       [0.0, 0.0, 0.0, 1.0]], np.float32),
    yfov=F32(math.pi / 4.0), znear=F32(0.05), ambient=F32(0.02), dir_intensity=F32(3.5), point_intensity=F32(0.5),
    albedo=np.full(3, 0.4, np.float32), background=np.ones(3, np.float32))

# sample offsets in 1/16 pixel
SAMPLES = {1: [(0, 0)], 4: [(-2, -6), (6, -2), (-6, 2), (2, 6)]}


def consts(template_verts, width, height, params=None):
    """The per-renderer constants sdfa_render_create derives (scale, view transform, projection, shading)."""
    p = dict(DEFAULT_PARAMS, **(params or {}))
    vmax = np.abs(np.asarray(template_verts, np.float32)).max()
    pose = np.asarray(p["cam_pose"], np.float32).astype(np.float64)
    R, t = pose[:3, :3], pose[:3, 3]
    m = np.zeros(12, np.float32)
    for i in range(3):                                   # rigid inverse (R^T, -R^T t) in fp64, rounded to fp32
        for j in range(3):
            m[4 * i + j] = F32(R[j, i])
        m[4 * i + 3] = F32(-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]))
    fy = 1.0 / math.tan(float(F32(p["yfov"])) * 0.5)
    albedo = np.asarray(p["albedo"], np.float32)
    return dict(s=F32(0.15) / F32(vmax), m=m, fy=F32(fy), fx=F32(fy / (float(width) / float(height))),
                hw=F32(0.5) * F32(width), hh=F32(0.5) * F32(height), znear=F32(p["znear"]), W=int(width), H=int(height),
                ka=albedo * F32(p["ambient"]), kd=(albedo.astype(np.float64) / math.pi).astype(np.float32),
                dir_i=F32(p["dir_intensity"]), pt_i=F32(p["point_intensity"]), bg=np.asarray(p["background"], np.float32))


def vertex_stage(verts, k):
    """(V, 3) -> screen (V, 4) int32 {x, y in 1/256 pixel, bits of 1/w, valid} and camera-space positions (V, 3)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    m, s = k["m"], k["s"]
    px, py, pz = s * v[:, 0], s * v[:, 1], s * v[:, 2]
    cx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
    cy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
    cz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
    with np.errstate(all="ignore"):
        w = -cz
        iw = F32(1.0) / w
        X = ((cx * k["fx"]) * iw + F32(1.0)) * k["hw"]
        Y = (F32(1.0) - (cy * k["fy"]) * iw) * k["hh"]
        ok = (np.isfinite(cx) & np.isfinite(cy) & np.isfinite(cz) & (w > k["znear"])
              & (np.abs(X) <= F32(GUARD_PX)) & (np.abs(Y) <= F32(GUARD_PX)))
        scr = np.zeros((len(v), 4), np.int32)
        scr[ok, 0] = np.rint(X[ok] * F32(256.0)).astype(np.int32)
        scr[ok, 1] = np.rint(Y[ok] * F32(256.0)).astype(np.int32)
    scr[ok, 2] = iw[ok].view(np.int32)
    scr[ok, 3] = 1
    return scr, np.stack([cx, cy, cz], 1)


def vertex_normals(verts, faces, s):
    """Area-weighted unit vertex normals in world space: sum over incident faces in ascending face order."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = [s * v[f[:, i]] for i in range(3)]
    e1, e2 = p[1] - p[0], p[2] - p[0]
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    flat_v = f.reshape(-1)
    flat_f = np.repeat(np.arange(len(f)), 3)
    order = np.argsort(flat_v, kind="stable")          # per vertex, ascending face order
    fv, ff = flat_v[order], flat_f[order]
    start = np.searchsorted(fv, np.arange(len(v)))
    deg = np.bincount(flat_v, minlength=len(v))
    n = np.zeros((len(v), 3), np.float32)
    for j in range(int(deg.max()) if len(deg) else 0):
        has = deg > j
        idx = ff[np.minimum(start + j, len(ff) - 1)]
        n = np.where(has[:, None], n + cr[idx], n)
    l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    pos = l2 > 0
    with np.errstate(all="ignore"):
        inv = F32(1.0) / np.sqrt(l2)
    n[pos] = n[pos] * inv[pos, None]
    return n


def to_camera(n, k):
    m = k["m"]
    return np.stack([(m[0] * n[:, 0] + m[1] * n[:, 1]) + m[2] * n[:, 2], (m[4] * n[:, 0] + m[5] * n[:, 1]) + m[6] * n[:, 2],
                     (m[8] * n[:, 0] + m[9] * n[:, 1]) + m[10] * n[:, 2]], 1)


def edge(ax, ay, bx, by, px, py):
    return (np.int64(by) - ay) * (np.asarray(px, np.int64) - ax) - (np.int64(bx) - ax) * (np.asarray(py, np.int64) - ay)


def raster(scr, faces, width, height, samples=1):
    """Visibility of every sample: (H, W, S) int64 triangle index (INT_MAX = background) and (H, W, S) float32 1/w."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    best = np.full((height, width, samples), -np.inf, np.float32)
    btri = np.full((height, width, samples), INT_MAX, np.int64)
    offs = SAMPLES[samples]
    for t in range(len(f)):
        p = [scr[f[t, i]].astype(np.int64) for i in range(3)]
        if not (p[0][3] and p[1][3] and p[2][3]):
            continue
        D = edge(p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1])
        if D <= 0:
            continue
        xs, ys = [q[0] for q in p], [q[1] for q in p]
        x0, x1 = max((min(xs) >> 8) - 1, 0), min(max(xs) >> 8, width - 1)
        y0, y1 = max((min(ys) >> 8) - 1, 0), min(max(ys) >> 8, height - 1)
        if x0 > x1 or y0 > y1:
            continue
        gy, gx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        rD = F32(1.0) / F32(D)
        for si, (ox, oy) in enumerate(offs):
            sx, sy = gx * 256 + 128 + 16 * ox, gy * 256 + 128 + 16 * oy
            cov = np.ones(sx.shape, bool)
            Fs = []
            for e in range(3):
                u, v = p[(e + 1) % 3], p[(e + 2) % 3]
                Fe = edge(u[0], u[1], v[0], v[1], sx, sy)
                dy, dx = v[1] - u[1], v[0] - u[0]
                bias = 0 if (dy > 0 or (dy == 0 and dx < 0)) else 1
                cov &= Fe >= bias
                Fs.append(Fe)
            if not cov.any():
                continue
            iw = [np.int32(q[2]).view(np.float32) for q in p]
            z = ((Fs[0].astype(np.float32) * rD) * iw[0] + (Fs[1].astype(np.float32) * rD) * iw[1]) + (Fs[2].astype(np.float32) * rD) * iw[2]
            bz, bt = best[y0:y1 + 1, x0:x1 + 1, si], btri[y0:y1 + 1, x0:x1 + 1, si]
            win = cov & ((z > bz) | ((z == bz) & (t < bt)))
            bz[win] = z[win]
            bt[win] = t
    return btri, best


def shade(btri, scr, pos, nrm_cam, faces, k, samples):
    """(H, W, 3) uint8 from the visibility of every sample."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    H, W, S = btri.shape
    gy, gx = np.mgrid[0:H, 0:W]
    acc = None
    for si, (ox, oy) in enumerate(SAMPLES[samples]):
        col = np.broadcast_to(k["bg"], (H, W, 3)).astype(np.float32).copy()
        hit = btri[:, :, si] != INT_MAX
        t = btri[:, :, si][hit]
        sx, sy = (gx * 256 + 128 + 16 * ox)[hit], (gy * 256 + 128 + 16 * oy)[hit]
        i0, i1, i2 = f[t, 0], f[t, 1], f[t, 2]
        a, b, d = scr[i0].astype(np.int64), scr[i1].astype(np.int64), scr[i2].astype(np.int64)
        with np.errstate(all="ignore"):
            rD = F32(1.0) / edge(a[:, 0], a[:, 1], b[:, 0], b[:, 1], d[:, 0], d[:, 1]).astype(np.float32)
            w0 = edge(b[:, 0], b[:, 1], d[:, 0], d[:, 1], sx, sy).astype(np.float32) * rD
            w1 = edge(d[:, 0], d[:, 1], a[:, 0], a[:, 1], sx, sy).astype(np.float32) * rD
            w2 = edge(a[:, 0], a[:, 1], b[:, 0], b[:, 1], sx, sy).astype(np.float32) * rD
            q0, q1, q2 = w0 * a[:, 2].astype(np.int32).view(np.float32), w1 * b[:, 2].astype(np.int32).view(np.float32), w2 * d[:, 2].astype(np.int32).view(np.float32)
            iz = F32(1.0) / ((q0 + q1) + q2)
            c0, c1, c2 = q0 * iz, q1 * iz, q2 * iz
            n = [(c0 * nrm_cam[i0, j] + c1 * nrm_cam[i1, j]) + c2 * nrm_cam[i2, j] for j in range(3)]
            P = [(c0 * pos[i0, j] + c1 * pos[i1, j]) + c2 * pos[i2, j] for j in range(3)]
            l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            inv = np.where(l2 > 0, F32(1.0) / np.sqrt(l2), F32(1.0)).astype(np.float32)
            n = [np.where(l2 > 0, x * inv, x) for x in n]
            d2 = (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]
            ndl_dir = np.fmax(n[2], F32(0.0))
            ndl_pt = np.fmax(-((n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]) * (F32(1.0) / np.sqrt(d2)), F32(0.0))
            e = k["dir_i"] * ndl_dir + (k["pt_i"] * ndl_pt) / d2
            for c in range(3):
                col[:, :, c][hit] = np.fmin(np.fmax(k["ka"][c] + k["kd"][c] * e, F32(0.0)), F32(1.0))
        acc = col if acc is None else acc + col
    if samples > 1:
        acc = acc * F32(1.0 / samples)
    return np.rint(acc * F32(255.0)).astype(np.uint8)


def render(template_verts, faces, verts, width, height, samples=1, normals="template", params=None):
    """One frame: (rgb (H, W, 3) uint8, tri ids of the first sample (H, W) int32, screen (V, 4) int32)."""
    k = consts(template_verts, width, height, params)
    scr, pos = vertex_stage(verts, k)
    n_world = vertex_normals(template_verts if normals == "template" else verts, faces, k["s"])
    btri, _ = raster(scr, faces, width, height, samples)
    rgb = shade(btri, scr, pos, to_camera(n_world, k), faces, k, samples)
    ids = np.where(btri[:, :, 0] == INT_MAX, -1, btri[:, :, 0]).astype(np.int32)
    return rgb, ids, scr
