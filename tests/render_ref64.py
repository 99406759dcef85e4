"""Independent float64 reference of the rendering contract (include/sdfa_render.h): a ray caster.

It shares nothing with the formulation of csrc/render.hip and tests/render_oracle.py: no edge functions, no snapping, no
fp32, no clip space.  Camera-space points are R^T (s v - t); one ray runs from the origin through every sample position,
direction (x_ndc tan(yfov/2) W/H, y_ndc tan(yfov/2), -1); it is intersected with every triangle by scalar triple products;
the nearest hit among front faces (n . a < 0 with the camera at the origin) whose three vertices lie beyond znear wins.
Projected pixel positions of vertices are formed only for what is measured in pixels: the guard-band drop rule of the
contract and the distance of a sample to the nearest projected edge.

Only the rig's data (DEFAULT_PARAMS) comes from render_oracle."""
import math

import numpy as np

from render_oracle import DEFAULT_PARAMS

OFFSETS = {1: [(0.0, 0.0)], 4: [(-2 / 16, -6 / 16), (6 / 16, -2 / 16), (-6 / 16, 2 / 16), (2 / 16, 6 / 16)]}   # pixels
GUARD_PX = 32768.0
FAR_EDGE = 0.5          # edge distances are exact below this many pixels and reported as this value where no edge is that near
CHUNK = 1 << 19         # (triangle, pixel) pairs per pass


class Rig:
    def __init__(self, template_verts, width, height, params=None):
        p = dict(DEFAULT_PARAMS, **(params or {}))
        pose = np.asarray(p["cam_pose"], np.float64)
        self.R, self.t = pose[:3, :3], pose[:3, 3]
        self.s = 0.15 / float(np.abs(np.asarray(template_verts, np.float64)).max())
        self.W, self.H = int(width), int(height)
        self.ty = math.tan(float(p["yfov"]) * 0.5)
        self.tx = self.ty * self.W / self.H
        self.znear = float(p["znear"])
        self.ambient, self.dir_i, self.pt_i = float(p["ambient"]), float(p["dir_intensity"]), float(p["point_intensity"])
        self.albedo, self.bg = np.asarray(p["albedo"], np.float64), np.asarray(p["background"], np.float64)

    def camera(self, verts):
        return (self.s * np.asarray(verts, np.float64).reshape(-1, 3) - self.t) @ self.R          # rows of R^T (s v - t)

    def pixels(self, cam):
        """Pixel position (x right, y down, pixel (0, 0) spans [0, 1)^2) of camera-space points in front of the camera."""
        d = -cam[:, 2]
        return np.stack([(cam[:, 0] / d / self.tx + 1.0) * 0.5 * self.W, (1.0 - cam[:, 1] / d / self.ty) * 0.5 * self.H], 1)

    def rays(self, sx, sy):
        """Directions (..., 3) through pixel positions sx, sy."""
        return np.stack([(2.0 * sx / self.W - 1.0) * self.tx, (1.0 - 2.0 * sy / self.H) * self.ty, -np.ones_like(sx)], -1)


def _drawn(rig, cam, faces):
    """Indices of the triangles the contract draws: every vertex beyond znear and inside the guard band, front facing."""
    with np.errstate(all="ignore"):
        px = rig.pixels(cam)
        ok_v = np.isfinite(cam).all(1) & (-cam[:, 2] > rig.znear) & (np.abs(px) <= GUARD_PX).all(1)
    a, b, c = cam[faces[:, 0]], cam[faces[:, 1]], cam[faces[:, 2]]
    with np.errstate(all="ignore"):
        front = np.einsum("ij,ij->i", np.cross(b - a, c - a), a) < 0.0
    return np.flatnonzero(ok_v[faces].all(1) & front), px


def _pairs(x0, x1, y0, y1):
    """All (triangle slot, pixel x, pixel y) of inclusive pixel boxes."""
    w, h = x1 - x0 + 1, y1 - y0 + 1
    cnt = w * h
    slot = np.repeat(np.arange(len(cnt)), cnt)
    k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return slot, x0[slot] + k % w[slot], y0[slot] + k // w[slot]


def _seg_dist(px, py, ax, ay, bx, by):
    ex, ey = bx - ax, by - ay
    l2 = ex * ex + ey * ey
    with np.errstate(all="ignore"):
        u = np.where(l2 > 0, ((px - ax) * ex + (py - ay) * ey) / l2, 0.0)
    u = np.clip(u, 0.0, 1.0)
    return np.hypot(px - (ax + u * ex), py - (ay + u * ey))


def visibility(rig, verts, faces, samples):
    """Per sample, (H, W, S): id of the nearest triangle hit (-1 = none), its depth (distance along the camera's -Z), the depth of
    the second-nearest hit (inf = none) and the distance in pixels to the nearest projected edge of any drawn triangle."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cam = rig.camera(verts)
    H, W, offs = rig.H, rig.W, OFFSETS[samples]
    S = len(offs)
    tid = np.full(H * W * S, -1, np.int64)
    d1 = np.full(H * W * S, np.inf)
    d2 = np.full(H * W * S, np.inf)
    edge = np.full(H * W * S, FAR_EDGE)
    drawn, px = _drawn(rig, cam, faces)
    if len(drawn):
        P = px[faces[drawn]]                                                   # (n, 3, 2)
        x0 = np.clip(np.floor(P[:, :, 0].min(1) - 1.0), 0, W - 1).astype(np.int64)
        x1 = np.clip(np.ceil(P[:, :, 0].max(1) + 1.0), -1, W - 1).astype(np.int64)
        y0 = np.clip(np.floor(P[:, :, 1].min(1) - 1.0), 0, H - 1).astype(np.int64)
        y1 = np.clip(np.ceil(P[:, :, 1].max(1) + 1.0), -1, H - 1).astype(np.int64)
        keep = (x0 <= x1) & (y0 <= y1)
        drawn, P, x0, x1, y0, y1 = drawn[keep], P[keep], x0[keep], x1[keep], y0[keep], y1[keep]
    area = (x1 - x0 + 1) * (y1 - y0 + 1) if len(drawn) else np.zeros(0, np.int64)
    start = 0
    while start < len(drawn):                                                  # runs of triangles of at most CHUNK pairs
        stop = start + max(1, int(np.searchsorted(np.cumsum(area[start:]), CHUNK, side="right")))
        sl = slice(start, stop)
        slot, gx, gy = _pairs(x0[sl], x1[sl], y0[sl], y1[sl])
        t = drawn[sl][slot]
        a, b, c = cam[faces[t, 0]], cam[faces[t, 1]], cam[faces[t, 2]]
        bc, ca, ab = np.cross(b, c), np.cross(c, a), np.cross(a, b)
        det = np.einsum("ij,ij->i", a, bc)                                     # a . (b x c): negative for a front face
        Pp = P[sl][slot]
        for si, (ox, oy) in enumerate(offs):
            sx, sy = gx + 0.5 + ox, gy + 0.5 + oy
            key = (gy * W + gx) * S + si
            e = np.minimum(np.minimum(_seg_dist(sx, sy, Pp[:, 0, 0], Pp[:, 0, 1], Pp[:, 1, 0], Pp[:, 1, 1]),
                                      _seg_dist(sx, sy, Pp[:, 1, 0], Pp[:, 1, 1], Pp[:, 2, 0], Pp[:, 2, 1])),
                           _seg_dist(sx, sy, Pp[:, 2, 0], Pp[:, 2, 1], Pp[:, 0, 0], Pp[:, 0, 1]))
            near = e < FAR_EDGE
            np.minimum.at(edge, key[near], e[near])
            d = rig.rays(sx, sy)
            u, v, w = (np.einsum("ij,ij->i", d, m) for m in (bc, ca, ab))     # signed volumes: all of det's sign inside
            hit = (u <= 0) & (v <= 0) & (w <= 0) & (u + v + w < 0)
            depth = det[hit] / (u + v + w)[hit]                                # the hit is depth * d, and d_z = -1
            kh, th = key[hit], t[hit]
            order = np.lexsort((th, depth, kh))
            kh, th, depth = kh[order], th[order], depth[order]
            first = np.r_[True, kh[1:] != kh[:-1]] if len(kh) else np.zeros(0, bool)
            rank = np.arange(len(kh)) - np.maximum.accumulate(np.where(first, np.arange(len(kh)), 0)) if len(kh) else first
            for r in (0, 1):                                                   # a chunk's two nearest per sample into the running two
                m = rank == r
                k_, t_, z_ = kh[m], th[m], depth[m]
                nearer = (z_ < d1[k_]) | ((z_ == d1[k_]) & (t_ < tid[k_]))
                kn, ko = k_[nearer], k_[~nearer]
                d2[kn] = d1[kn]
                d1[kn], tid[kn] = z_[nearer], t_[nearer]
                d2[ko] = np.minimum(d2[ko], z_[~nearer])
        start = stop
    shape = (H, W, S)
    return tid.reshape(shape), d1.reshape(shape), d2.reshape(shape), edge.reshape(shape)


def vertex_normals(rig, verts, faces):
    """Area-weighted unit vertex normals in camera space (zero where the incident areas cancel or there is no face)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p = rig.s * np.asarray(verts, np.float64).reshape(-1, 3)
    cr = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    n = np.zeros_like(p)
    np.add.at(n, faces.reshape(-1), np.repeat(cr, 3, axis=0))                 # unbuffered, in face order
    l = np.linalg.norm(n, axis=1)
    n[l > 0] /= l[l > 0, None]
    return n @ rig.R


def _shade_samples(rig, cam, nrm, faces, tid, sx, sy):
    """Colour (N, 3) in [0, 1] of the rays through (sx, sy) on the planes of triangles tid (N,): Lambert of DESIGN.md section 8."""
    a, b, c = cam[faces[tid, 0]], cam[faces[tid, 1]], cam[faces[tid, 2]]
    d = rig.rays(sx, sy)
    bc, ca, ab = np.cross(b, c), np.cross(c, a), np.cross(a, b)
    u, v, w = (np.einsum("ij,ij->i", d, m) for m in (bc, ca, ab))
    tot = u + v + w
    bu, bv, bw = u / tot, v / tot, w / tot                                     # barycentrics of the 3-D hit point
    Ppt = bu[:, None] * a + bv[:, None] * b + bw[:, None] * c
    n = bu[:, None] * nrm[faces[tid, 0]] + bv[:, None] * nrm[faces[tid, 1]] + bw[:, None] * nrm[faces[tid, 2]]
    l = np.linalg.norm(n, axis=1)
    n = np.where(l[:, None] > 0, n / np.where(l > 0, l, 1.0)[:, None], n)
    dist = np.linalg.norm(Ppt, axis=1)
    e = rig.dir_i * np.maximum(n[:, 2], 0.0) + rig.pt_i * np.maximum(-np.einsum("ij,ij->i", n, Ppt) / dist, 0.0) / dist ** 2
    return np.clip(rig.albedo[None] * rig.ambient + rig.albedo[None] / math.pi * e[:, None], 0.0, 1.0)


def shade(rig, verts, normal_verts, faces, tid, shift=(0.0, 0.0)):
    """(H, W, 3) float64 levels (0 .. 255, not rounded): every sample shaded, clamped, the samples averaged.  `shift` displaces
    every sample (pixels) while keeping its triangle: the ray meets the triangle's plane."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cam, nrm = rig.camera(verts), vertex_normals(rig, normal_verts, faces)
    H, W, S = tid.shape
    gy, gx = np.mgrid[0:H, 0:W]
    acc = np.zeros((H, W, 3))
    for si, (ox, oy) in enumerate(OFFSETS[S]):
        col = np.broadcast_to(rig.bg, (H, W, 3)).copy()
        hit = tid[:, :, si] >= 0
        col[hit] = _shade_samples(rig, cam, nrm, faces, tid[:, :, si][hit], gx[hit] + 0.5 + ox + shift[0], gy[hit] + 0.5 + oy + shift[1])
        acc += col
    return acc * (255.0 / S)


def colour_and_bound(rig, verts, normal_verts, faces, tid, step=1.0 / 256.0):
    """The image and, per pixel, 0.75 + 2 max|c(sample displaced by +-step in x or y on its triangle's plane) - c| levels:
    0.5 for the final rounding, 0.25 for fp32 shading, the rest the first-order effect of snapping vertices to 1/256 pixel."""
    c = shade(rig, verts, normal_verts, faces, tid)
    dev = np.zeros(c.shape[:2])
    for sh in ((step, 0.0), (-step, 0.0), (0.0, step), (0.0, -step)):
        dev = np.maximum(dev, np.abs(shade(rig, verts, normal_verts, faces, tid, sh) - c).max(2))
    return c, 0.75 + 2.0 * dev
