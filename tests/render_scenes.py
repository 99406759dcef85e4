"""Small synthetic scenes for the rasterizer tests (tests/test_render_ref64_cpu.py, tests/test_render_edges_gpu.py).

Every scene is built in world units with max|v| = 0.15f exactly (the anchor vertex below), so the renderer's scale
0.15f / max|template| is 1 and a scene's numbers are the numbers the kernels see.  A scene is a dict:
    verts (V, 3) float32, faces (T, 3) uint32, params (dict over render_oracle.DEFAULT_PARAMS, {} = the default rig),
    normals ("template" / "frame"), and a few scene-specific entries.
Each builder says which path of csrc/render.hip it is there for."""
import math

import numpy as np

from render_oracle import DEFAULT_PARAMS

ANCHOR = (np.float32(0.15), 0.0, 0.0)        # the one vertex no face references: it fixes max|v| = 0.15f (vertex_normal: no incident face)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """Camera-to-world pose (4, 4) float32 of a camera at `eye` looking down its -Z at `target`."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose.astype(np.float32)


def cam_to_world(p_cam, pose=None):
    pose = np.asarray(DEFAULT_PARAMS["cam_pose"] if pose is None else pose, np.float64)
    return np.asarray(p_cam, np.float64) @ pose[:3, :3].T + pose[:3, 3]


def _scene(world, faces, params=None, normals="template", **extra):
    world = np.asarray(world, np.float64).reshape(-1, 3)
    assert np.abs(world).max() < 0.15, "a scene must fit the 0.15 box the anchor vertex spans"
    verts = np.concatenate([world.astype(np.float32), np.asarray([ANCHOR], np.float32)])
    faces = np.asarray(faces, np.uint32).reshape(-1, 3)
    assert faces.max() < len(verts) - 1, "no face references the anchor"
    assert np.abs(verts).max() == np.float32(0.15)
    return dict(verts=verts, faces=faces, params=dict(params or {}), normals=normals, **extra)


# the second rig of the float64 comparison: another pose, field of view and near plane
CAMERA2 = dict(cam_pose=look_at((-0.20, 0.12, 0.40)), yfov=np.float32(0.6), znear=np.float32(0.1))
# albedo and background that differ per channel: a swap of R and B anywhere changes the image
COLOURED = dict(albedo=np.array([0.8, 0.4, 0.15], np.float32), background=np.array([0.1, 0.5, 0.9], np.float32))
AMBIENT_ONLY = dict(ambient=np.float32(0.6), dir_intensity=np.float32(0.0), point_intensity=np.float32(0.0), **COLOURED)
SATURATING = dict(dir_intensity=np.float32(9.0), point_intensity=np.float32(2.0), **COLOURED)       # most of the lit side clamps at 1.0
# the close rig: 0.13 from the origin, 0.03 above the ellipsoid and looking along it, narrow field of view, lights turned
# down so that the image does not clamp to white
CLOSE = dict(cam_pose=look_at(0.13 * np.array([0.25, 0.15, 1.0]) / np.linalg.norm([0.25, 0.15, 1.0]), (0.0, -0.08, 0.03)), yfov=np.float32(0.3),
             znear=np.float32(0.01), dir_intensity=np.float32(2.0), point_intensity=np.float32(0.001), **COLOURED)


def ellipsoid_wall_blade(params=None):
    """A 12 x 8 ellipsoid with single pole vertices (fans of 12 triangles at the poles, vertices of degree 12 and 6), a tilted
    two-triangle wall behind it (large triangles: boxes that span many tiles), a blade that cuts through the ellipsoid (depth
    order changes along a line inside triangles) present in both windings, each face directly followed by its reverse, so that
    its vertices' normals cancel to exactly zero (vertex_normal and shade: the l2 == 0 branch), and the anchor (a vertex without
    faces: the empty gather)."""
    seg, stacks, rad = 12, 8, np.array([0.10, 0.12, 0.10])
    pts = [(0.0, rad[1], 0.0)]
    for j in range(1, stacks):
        th = math.pi * j / stacks
        for i in range(seg):
            ph = 2.0 * math.pi * i / seg
            pts.append((rad[0] * math.sin(th) * math.sin(ph), rad[1] * math.cos(th), rad[2] * math.sin(th) * math.cos(ph)))
    pts.append((0.0, -rad[1], 0.0))
    south = len(pts) - 1
    ring = lambda j, i: 1 + (j - 1) * seg + i % seg
    faces = []
    for i in range(seg):
        faces.append((0, ring(1, i), ring(1, i + 1)))
        faces.append((south, ring(stacks - 1, i + 1), ring(stacks - 1, i)))
    for j in range(1, stacks - 1):
        for i in range(seg):
            a, b, c, d = ring(j, i), ring(j, i + 1), ring(j + 1, i), ring(j + 1, i + 1)
            faces += [(a, c, d), (a, d, b)]
    n0 = len(pts)                                               # wall: behind the ellipsoid, tilted, facing +Z
    pts += [(-0.14, -0.14, -0.135), (0.14, -0.14, -0.105), (0.14, 0.14, -0.125), (-0.14, 0.14, -0.145)]
    faces += [(n0, n0 + 1, n0 + 2), (n0, n0 + 2, n0 + 3)]
    b0 = len(pts)                                               # blade: the plane 0.8 y + 0.6 z = 0.03, wider than the ellipsoid
    nrm, u, v = np.array([0.0, 0.8, 0.6]), np.array([1.0, 0.0, 0.0]), np.array([0.0, -0.6, 0.8])
    for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        pts.append(tuple(0.03 * nrm + su * 0.14 * u + sv * 0.115 * v))
    for tri in ((b0, b0 + 1, b0 + 2), (b0, b0 + 2, b0 + 3)):
        faces += [tri, (tri[0], tri[2], tri[1])]
    return _scene(pts, faces, params, blade_verts=np.arange(b0, b0 + 4), blade_faces=np.arange(len(faces) - 4, len(faces)))


def close():
    """ellipsoid_wall_blade under the CLOSE rig: a handful of triangles cover whole images, their vertices lie a thousand and more
    pixels outside on every side (negative coordinates: >> 8 of a negative value, every clamp of render_setup_kernel's box), and
    the edge values and the doubled area are far above 2^24, so (float)F and 1.0f / (float)D round.  Perspective matters here:
    1/w varies several-fold across a triangle."""
    return ellipsoid_wall_blade(CLOSE)


GUARD = dict(yfov=np.float32(0.002))           # 2.8e5 pixels per world unit at 256 rows: the guard band is +-0.118 in camera x, y


def guard_band(size=(256, 256)):
    """A field of view so narrow that vertices 0.13 off the axis project beyond the +-2^15-pixel guard band.  Nearest to the camera
    two triangles that would cover the whole image but have such a vertex (valid == 0 with w > znear: dropped), behind them a
    triangle that covers part of the image with all vertices inside the band (drawn), and behind that a quad that fills the image.
    Two slivers (faces 5, 6) reach from the image to a vertex in the last pixel inside the band, X (Y) in [-32768, -32767): the
    only place where render_setup_kernel's x0 (y0) = (min >> 8) - 1 does not fit an int16 before its clamp to 0."""
    z = -0.45
    W, H = size
    t = math.tan(float(GUARD["yfov"]) * 0.5)
    edge_x = (-32767.5 / (0.5 * W) - 1.0) * t * (W / H) * -(z + 0.010)          # camera x of pixel X = -32767.5 at that depth
    edge_y = (1.0 - -32767.5 / (0.5 * H)) * t * -(z + 0.012)
    cam = [(-0.13, -0.05, z + 0.02), (0.10, -0.06, z + 0.02), (0.0, 0.11, z + 0.02),           # 0: x beyond the band
           (-0.06, -0.10, z + 0.03), (0.09, 0.02, z + 0.03), (-0.05, 0.135, z + 0.03),          # 1: y beyond the band
           (-0.0004, -0.020, z), (0.024, 0.0003, z + 0.004), (-0.0003, 0.018, z - 0.004),       # 2: drawn, one edge through the image
           (-0.02, -0.02, z - 0.02), (0.02, -0.02, z - 0.02), (0.02, 0.02, z - 0.02), (-0.02, 0.02, z - 0.02),
           (edge_x, 0.0, z + 0.010), (-0.0001, -0.0003, z + 0.010), (-0.0001, 0.0002, z + 0.010),
           (0.0, edge_y, z + 0.012), (-0.0002, 0.0001, z + 0.012), (0.0003, 0.0001, z + 0.012)]
    faces = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (9, 11, 12), (13, 14, 15), (16, 17, 18)]
    return _scene(cam_to_world(cam), faces, GUARD, dropped_faces=np.array([0, 1]), edge_verts=(13, 16), edge_faces=np.array([5, 6]))


TIES = dict(yfov=np.float32(0.3))              # narrow enough that the filler triangles lie outside the image


def ties():
    """A fan of 20 triangles; the same 20 again in the same block of 256 (same vertex indices), 300 small filler triangles outside
    the image, and the 20 a third time from duplicated vertices, more than 256 indices later.  Every covered sample meets the exact
    tie z == best twice, within one block and across blocks: the first copy must own it."""
    n, zc = 20, -0.46
    cam = [(0.0, 0.0, zc + 0.01)] + [(0.05 * math.cos(2 * math.pi * i / n), 0.05 * math.sin(2 * math.pi * i / n), zc - 0.01 * math.cos(3 * i))
                                      for i in range(n)]
    fan = [(0, 1 + i, 1 + (i + 1) % n) for i in range(n)]
    faces = fan + fan
    for i in range(300):                                        # fillers: a ring far off the axis, front facing
        a = 2 * math.pi * i / 300
        cx, cy, k = 0.125 * math.cos(a), 0.125 * math.sin(a), len(cam)
        cam += [(cx, cy, zc), (cx + 0.004, cy, zc), (cx, cy + 0.004, zc)]
        faces.append((k, k + 1, k + 2))
    k = len(cam)
    cam += cam[:n + 1]
    faces += [(k + a, k + b, k + c) for a, b, c in fan]
    return _scene(cam_to_world(cam), faces, TIES, n_fan=n)


def stack(n=600, size=(256, 256)):
    """600 triangles of 40 to 60 pixels that all contain the centre of the 32 x 32 tile at pixels (96..127, 96..127), at depths
    in random order: in every block of 256 triangles every lane hits that tile, so the compaction list is full (slot 255) and
    the last block (88) is partial."""
    rs = np.random.RandomState(5)
    W, H = size
    depth = 0.36 + 3e-4 * rs.permutation(n)
    t = math.tan(math.pi / 8)
    cam, faces = [], []
    for i in range(n):
        ang = rs.uniform(0, 2 * math.pi) + np.array([0.0, 2.1, 4.2]) + rs.uniform(-0.3, 0.3, 3)
        r = rs.uniform(20.0, 30.0, 3)
        px, py = 112.0 + r * np.cos(ang), 112.0 - r * np.sin(ang)              # counter-clockwise with y up
        x = (2 * px / W - 1) * t * (W / H) * depth[i]
        y = (1 - 2 * py / H) * t * depth[i]
        cam += [(x[k], y[k], -depth[i] - 0.004 * k) for k in range(3)]
        faces.append((3 * i, 3 * i + 1, 3 * i + 2))
    return _scene(cam_to_world(cam), faces)


def grid(T, n=128):
    """The camera-facing plane of test_watertight_camera_facing_grid (2 n^2 triangles of ~1.4 pixels at 256^2), cut to its first T
    triangles: T = 1, 255, 256, 257, 513 are one partial block, one full block, and a block boundary with one triangle behind it."""
    rows = -(-T // (2 * n))
    u = np.linspace(-0.12, 0.12, n + 1)
    gx, gy = np.meshgrid(u, u[:rows + 1])
    cam = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -0.4)], 1)
    faces = []
    for j in range(rows):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            faces += [(a, b, d), (a, d, c)]
    return _scene(cam_to_world(cam), faces[:T])


def facets(n=20):
    """n^2 disjoint triangles of about 8 pixels (at 256^2) on a lattice, each with three private vertices and a random tilt, rendered
    with normals="frame": flat shading, so neighbours differ by tens of levels and the wrong triangle at any one of the four samples
    moves the pixel by more than one level (samples 1 to 3 of render_raster_kernel<4>)."""
    rs = np.random.RandomState(9)
    cam, faces = [], []
    step = 0.24 / n
    for j in range(n):
        for i in range(n):
            c = np.array([-0.12 + (i + 0.5) * step, -0.12 + (j + 0.5) * step, -0.40])
            ang = rs.uniform(0, 2 * math.pi) + np.array([0.0, 2.1, 4.2])
            tilt = rs.uniform(-1.2, 1.2, 2)
            for k in range(3):
                dx, dy = 0.45 * step * math.cos(ang[k]), 0.45 * step * math.sin(ang[k])
                cam.append((c[0] + dx, c[1] + dy, c[2] + tilt[0] * dx + tilt[1] * dy))
            faces.append((len(cam) - 3, len(cam) - 2, len(cam) - 1))
    return _scene(cam_to_world(cam), faces, normals="frame")
