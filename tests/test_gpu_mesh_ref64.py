"""The dgrad -> mesh stage (mesh_rhs_kernel, the fp32 GEMM with the template's inverse, mesh_scatter_kernel, the fused
saber.stream.seek blend) against a float64 restatement of the stage (tests/mesh_ref64.py), at a frame count on each side of every
change of launch form.

Launch forms.  mesh_solve() hands the GEMM Ppad = K = free_pad and Qpad = ld = round_up(3 * frames, 128); gemm.hip launch_any /
small_tile_pays pick the kernel from those and the CU count (gemm_form below).  For FLAME (1261 free vertices, free_pad 1280, a
40-stage contraction) on 256 CUs: the 64 x 64 tile form of gemm_k4_kernel up to 512 frames, its 128 x 128 form from 513, the
persistent gemm_fat_kernel at 8747 .. 8789 frames (Qpad 26,368 = 103 x 256: 5 x 103 tiles >= 512), the 128 x 128 form again at 8790
(Qpad an odd multiple of 128).  The small meshes run the sizes at which ld changes (42 | 43, 85 | 86) and 130.

Inputs.  Rows at the fixtures' sigma, a zero row, a rotation-only row, a scale-only row and a row whose rotation vectors have norms
from 1e-12 to 4 (the identity branch of transform_minus_identity, the half-angle form of (1 - cos a) / a^2, angles at and beyond
pi).  The large FLAME sizes go through get_mesh_seek with a plan over four clips of 8 .. 12 irregularly stamped frames, fps chosen
so that the plan has exactly the wanted number of queries, with queries before a clip's first timestamp, after its last and
exactly on one; the blends scale the rotation-edge row's vectors continuously between its neighbours'.

Errors are max|gpu - ref| per frame (`abs`) and that over max|ref - template| of the frames it is taken over (`rel`), for the
frames that blend the rotation-edge row (`edge_*`) and for all the others; every frame of every size is under one of the two pairs.
The sensitivity controls at the bottom show that the bounds catch a dropped incidence, a stale frame and a skipped K block.

`python tests/test_gpu_mesh_ref64.py` prints every measured value (how the bounds below were set).  The fixture takes about
8 s and 4.3 GiB of device memory on an MI355X run on its own, 5.9 GiB of peak within the whole suite (3.2 GB are the two-step
form's rows at 8789 frames).
"""
import ctypes as C
import json
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
from mesh_ref64 import MeshRef64                                                 # noqa: E402

pytestmark = pytest.mark.gpu

# Over every mesh and size; each bound is at most 4x the largest value measured on an MI355X (256 CUs), written next to it.  The
# float32 rounding of the output alone is 7.5e-9 on FLAME's coordinates (below 0.25) and 1.5e-8 on the 43 x 3 patch's (up to 0.44);
# the largest `rel` is the one-frame FLAME call, a sigma 0.02 row that moves no vertex by more than 4.6e-4.  Per form at FLAME size
# (abs / edge_abs): 64 x 64 2.9e-8 / 7.5e-8, 128 x 128 4.9e-8 / 8.6e-8, gemm_fat_kernel 4.3e-8 / 9.2e-8 -- no form stands out, and
# all are some 40x below the 2e-6 that tests/test_next_rows.py allows against the float32 fixtures.
BOUNDS = {
    "abs": 1.5e-7,       # 4.86e-8 (FLAME, 8790 frames)
    "rel": 5e-5,         # 1.54e-5 (FLAME, 1 frame)
    "edge_abs": 3e-7,    # 9.18e-8 (FLAME, 8789 frames)
    "edge_rel": 1e-5,    # 2.83e-6 (FLAME, 8789 frames)
}
REST_POSE = 1e-9         # zero-dgrad frames: the template, up to the regulariser's reg * Inv * x_template (~1e-16)
SMALL_SIZES = (1, 2, 42, 43, 85, 86, 130)
FLAME_LIMIT = 9000
EDGE_NORMS = (1e-12, 1e-10, 1e-9, 1e-7, 1e-3, 1.0, math.pi - 1e-3, math.pi, 4.0)
VARIANTS = (2, 5, 6, 8)          # fp32 GEMM choices compared bitwise with the default at 512 FLAME frames (Qpad 1536 = 6 x 256):
                                 # 2 / 6 the 128 x 128 / 64 x 64 form, 5 gemm_big_kernel, 8 gemm_fat_kernel
VARIANT_SIZE = 512
SMALL, TILE, FAT = "gemm_k4_kernel 64x64", "gemm_k4_kernel 128x128", "gemm_fat_kernel"


def round_up(n, m=128):
    return -(-n // m) * m


# ---------------------------------------------------------------------------------------------------------------- launch forms
def gemm_form(ppad, qpad, k, cus):
    """The kernel gemm.hip launch_any runs for mesh_solve()'s call (OUT_K4, no bias, seg_k = K, Pstore = Ppad, ldp = Ppad,
    ldq = ldd = Qpad, row-major operands, default gemm_variant, no CUs reserved)."""
    fits = (ppad % 256 == 0 and qpad % 256 == 0 and k % 64 == 0 and qpad * 32 < 1 << 32
            and (k // 4) * ppad * 16 < 0x7fffffff and (k // 4) * qpad * 16 < 0x7fffffff)
    if fits and (ppad // 256) * (qpad // 256) >= 512:
        return FAT
    n128 = (ppad // 128) * (qpad // 128)                 # small_tile_pays
    if n128 * 2 < cus or (n128 <= 2 * cus and k <= 512):
        return SMALL
    return TILE


def flame_sizes(cus):
    """sizes_for(cus), and the size at which the GEMM variants are compared if it is not among them."""
    return sorted(set(sizes_for(cus)) | {VARIANT_SIZE})


def mesh_form(free_pad, frames, cus):
    return gemm_form(free_pad, round_up(3 * frames), free_pad, cus)


def sizes_for(cus, free_pad=1280, limit=FLAME_LIMIT):
    """1, and for each edge between forms that depends on the CU count the largest frame count on either side of it: the edges are
    the largest Qpad that still takes the 64 x 64 form and the smallest that takes gemm_fat_kernel; the sizes are the largest frame
    count with that Qpad (the most real columns in its last tile) and one more frame, the first with the next Qpad.  After the
    fat kernel's first Qpad the next is an odd multiple of 128: the 128 x 128 form again, on a problem larger than any it ran
    below the edge (so the largest 128 x 128 size below it, one Qpad down, is bracketed from both sides)."""
    qpads = range(128, round_up(3 * limit) + 1, 128)
    forms = {q: gemm_form(free_pad, q, free_pad, cus) for q in qpads}
    edges = [max((q for q in qpads if forms[q] == SMALL), default=None), min((q for q in qpads if forms[q] == FAT), default=None)]
    out = {1}
    for e in edges:
        if e is not None and e // 3 + 1 < limit:
            out |= {e // 3, e // 3 + 1}
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- meshes, rows
def grid_patch(nx, ny, seed=5):
    """An open grid patch with an nx x ny interior and the border constrained, as tests/test_mesh.py builds its 40 x 30 one."""
    rs = np.random.RandomState(seed)
    gx, gy = nx + 2, ny + 2
    x, y = np.meshgrid(np.arange(gx) * 0.01, np.arange(gy) * 0.01, indexing="ij")
    V = np.stack([x, y, 0.02 * np.sin(7 * x) * np.cos(5 * y)], -1).reshape(-1, 3).astype(np.float32)
    V += rs.normal(0, 1e-3, V.shape).astype(np.float32)
    idx = lambda i, j: i * gy + j
    F = np.asarray([[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(gx - 1) for j in range(gy - 1)] +
                   [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(gx - 1) for j in range(gy - 1)], np.uint32)
    cn = np.asarray([idx(i, j) for i in range(gx) for j in range(gy) if i in (0, gx - 1) or j in (0, gy - 1)], np.uint32)
    return V, F, cn


def meshes(golden):
    """name -> dict(verts, faces, cnsts, corr (kwargs for both MeshSolver and MeshRef64), n_src, sigmas)."""
    out = {}
    g = golden["mesh_flame"]
    out["flame"] = dict(verts=g["verts"], faces=g["faces"], cnsts=g["cnsts"], corr={}, n_src=len(g["faces"]),
                        sigmas=[float(s) for s in g["dgrad_sigma"] if s > 0])
    g = golden["mesh_corres"]
    out["corres"] = dict(verts=g["verts"], faces=g["faces"], cnsts=g["cnsts"], corr=dict(corr_count=g["corr_count"], corr_faces=g["corr_faces"]),
                         n_src=int(g["n_src_tris"]), sigmas=[float(np.asarray(g["dgrad"])[1:].std())])
    for name, (nx, ny) in (("grid16x8", (16, 8)), ("grid43x3", (43, 3))):
        V, F, cn = grid_patch(nx, ny)
        out[name] = dict(verts=V, faces=F, cnsts=cn, corr={}, n_src=len(F), sigmas=[0.08])       # sigma of tests/test_mesh.py
    return out


def make_solver(m):
    from sdfa_amd.mesh import MeshSolver
    kw = dict(m["corr"], n_src_tris=m["n_src"]) if m["corr"] else {}
    return MeshSolver(m["verts"], m["faces"], m["cnsts"], **kw)


def make_ref(m, device):
    return MeshRef64(m["verts"], m["faces"], m["cnsts"], device=device, **m["corr"])


def edge_row(n_src, rs):
    """Rotation vectors of random direction whose norms cycle through EDGE_NORMS, no scale part."""
    v = rs.normal(0, 1, (n_src, 3))
    v *= (np.asarray(EDGE_NORMS)[np.arange(n_src) % len(EDGE_NORMS)] / np.linalg.norm(v, axis=1))[:, None]
    d = np.zeros((n_src, 9), np.float32)
    d[:, 6:] = v.astype(np.float32)
    return d


def draw_rows(n, n_src, sigmas, seed, special):
    """(n, n_src * 9) float32: normal rows cycling through `sigmas`, with the rows `special` = {index: kind} replaced."""
    rs = np.random.RandomState(seed)
    rows = np.stack([rs.normal(0, sigmas[i % len(sigmas)], (n_src, 9)).astype(np.float32) for i in range(n)])
    for i, kind in special.items():
        if i >= n:
            continue
        if kind == "zero":
            rows[i] = 0.0
        elif kind == "rot_only":
            rows[i, :, :6] = 0.0
        elif kind == "scale_only":
            rows[i, :, 6:] = 0.0
        elif kind == "edge":
            rows[i] = edge_row(n_src, rs)
    return rows.reshape(n, -1)


SMALL_SPECIAL = {1: "edge", 2: "zero", 3: "rot_only", 4: "scale_only"}       # frame 0 (the 1-frame call) is a plain row

# FLAME animation rows: four clips, first timestamps 0 (query 0 lies exactly on it), 117, 40 and 250 ms; steps as irregular as the
# front end's rounded hops.  Clip 1 starts with the zero row and clip 2 with the rotation-edge row: the queries before a clip's
# first timestamp copy them unblended.  Clips 1 and 3 are planned a few queries past their last timestamp (rot_only, scale_only).
CLIP_FRAMES = (8, 12, 10, 9)
CLIP_START = (0, 117, 40, 250)
CLIP_EXTRA = (0, 3, 0, 2)
FLAME_SPECIAL = {8: "zero", 19: "rot_only", 20: "edge", 38: "scale_only"}
FLAME_EDGE_ROW, FLAME_ZERO_ROW = 20, 8


def flame_clips():
    rs = np.random.RandomState(77)
    return [[int(t) for t in t0 + np.concatenate([[0], np.cumsum(rs.choice([16, 17, 17, 33, 34, 50], n - 1))])]
            for n, t0 in zip(CLIP_FRAMES, CLIP_START)]


def plan_for(n):
    """(tslists, fps, query_counts) of a plan over flame_clips() with exactly n queries: model.py's count per clip at an fps found
    by bisection (the count is a step function of fps) plus CLIP_EXTRA."""
    ts = flame_clips()
    target = n - sum(CLIP_EXTRA)
    count = lambda fps: [MeshRef64.query_count(t[-1], fps) for t in ts]
    lo, hi = 1e-3, 1e7
    for _ in range(400):
        mid = math.sqrt(lo * hi)
        c = sum(count(mid))
        if c == target:
            return ts, mid, [a + b for a, b in zip(count(mid), CLIP_EXTRA)]
        lo, hi = (mid, hi) if c < target else (lo, mid)
    raise AssertionError(f"no fps gives {target} queries: two clips step together")


def plan_cases(ts, fps, counts):
    """How many queries lie before their clip's first timestamp, after its last, exactly on one."""
    before = after = on = 0
    for t, nq in zip(ts, counts):
        q = np.arange(nq, dtype=np.float64) * 1000.0 / fps
        before += int((q < t[0]).sum())
        after += int((q > t[-1]).sum())
        on += int(np.isin(q, np.asarray(t, np.float64)).sum())
    return dict(before=before, after=after, on=on)


# ---------------------------------------------------------------------------------------------------------------- measuring
def nan_out(n, n_verts):
    return torch.full((n, n_verts, 3), float("nan"), dtype=torch.float32, device="cuda:0")


def poison_workspace(ms, n):
    """NaN in every byte of the workspace a call of n frames will use: what the kernels do not write cannot look right."""
    ms._workspace(n).view(torch.float32).fill_(float("nan"))


def mesh_into(ms, d, out, poison=True):
    """sdfa_mesh_from_dgrad into a caller-owned (NaN-filled) vertex buffer."""
    from sdfa_amd._lib import lib, check
    n = d.shape[0]
    if poison:
        poison_workspace(ms, n)
    ws = ms._workspace(n)
    check(lib.sdfa_mesh_from_dgrad(ms._m, C.c_void_p(d.data_ptr()), n, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Size:
    """One mesh at one frame count: per-frame errors against float64 and the exact checks."""

    def __init__(self, n, form):
        self.n, self.form = n, form
        self.err = np.zeros(n)            # max|gpu - ref| per frame
        self.disp = np.zeros(n)           # max|ref - template| per frame
        self.edge = np.zeros(n, bool)     # frames that blend the rotation-edge row
        self.zero = np.zeros(n, bool)     # frames whose dgrad is all zero
        self.rest_err = 0.0               # max|gpu - template| over the zero frames
        self.finite = self.pinned = True
        self.plan_equal = self.cases = None

    def stat(self, key):
        m = self.edge if key.startswith("edge") else ~self.edge
        if not m.any():
            return 0.0
        a = float(self.err[m].max())
        return a if key.endswith("abs") else a / float(self.disp[m].max())


def compare(st, ref, out, rows_of, edge_of, tmpl32, cn):
    """Fill st from the GPU's vertices `out` and the float64 reference of the float32 rows rows_of(slice)."""
    n = st.n
    step = ref.frames_per_chunk()
    st.finite = bool(torch.isfinite(out).all())
    st.pinned = same_bits(out[:, cn], tmpl32[cn].unsqueeze(0).expand(n, -1, -1))
    for f0 in range(0, n, step):
        sl = slice(f0, min(n, f0 + step))
        d = rows_of(sl)
        want = ref.get_mesh(d)
        st.err[sl] = (out[sl].double() - want).abs().flatten(1).amax(1).cpu().numpy()
        st.disp[sl] = (want - ref.V64).abs().flatten(1).amax(1).cpu().numpy()
        st.zero[sl] = (d == 0).all(1).cpu().numpy()
        st.edge[sl] = edge_of(sl)
        del d, want
    if st.zero.any():
        z = torch.from_numpy(np.nonzero(st.zero)[0]).to(out.device)
        st.rest_err = float((out[z] - tmpl32).abs().max())
    return st


def pick_host_frames(st):
    """A zero frame, a rotation-edge frame and six others spread over the batch, for the controls."""
    plain = np.nonzero(~st.edge & ~st.zero)[0]
    pick = [int(np.nonzero(st.zero)[0][0]), int(np.nonzero(st.edge)[0][0])] + [int(plain[i]) for i in np.linspace(0, len(plain) - 1, 6).astype(int)]
    return np.asarray(pick, np.int64)


def measure(golden):
    from sdfa_amd import _lib
    from sdfa_amd import seek as S
    from sdfa_amd._lib import lib, check
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ms_all = meshes(golden)
    out = dict(cus=cus, sizes={}, bits={}, host=None)
    dev = "cuda:0"
    # ------------------------------------------------------------ small meshes: plain get_mesh at the sizes where ld changes
    for name in ("corres", "grid16x8", "grid43x3"):
        m = ms_all[name]
        ms, ref = make_solver(m), make_ref(m, dev)
        free_pad = round_up(ref.n_free)
        tmpl32 = torch.from_numpy(np.asarray(m["verts"], np.float32)).to(dev)
        cn = torch.from_numpy(np.asarray(m["cnsts"], np.int64)).to(dev)
        for n in SMALL_SIZES:
            rows = torch.from_numpy(draw_rows(n, m["n_src"], m["sigmas"], 4000 + n, SMALL_SPECIAL)).to(dev)
            got = mesh_into(ms, rows, nan_out(n, ref.n_verts))
            st = Size(n, mesh_form(free_pad, n, cus))
            edge = np.arange(n) == 1
            out["sizes"][(name, n)] = compare(st, ref, got, lambda sl: rows[sl], lambda sl: edge[sl], tmpl32, cn)
            del rows, got
        del ms, ref
    # ------------------------------------------------------------ FLAME
    m = ms_all["flame"]
    ms, ref = make_solver(m), make_ref(m, dev)
    assert (ref.n_free, round_up(ref.n_free)) == (1261, 1280)
    tmpl32 = torch.from_numpy(np.asarray(m["verts"], np.float32)).to(dev)
    cn = torch.from_numpy(np.asarray(m["cnsts"], np.int64)).to(dev)
    rows = torch.from_numpy(draw_rows(sum(CLIP_FRAMES), m["n_src"], m["sigmas"], 4100, FLAME_SPECIAL)).to(dev)
    width = rows.shape[1]
    sizes = sizes_for(cus)
    plans = {}
    for n in flame_sizes(cus):
        st = Size(n, mesh_form(1280, n, cus))
        if n < 16:           # fewer queries than four clips and the extras give: the plain call, one sigma row per frame
            got = mesh_into(ms, rows[:n], nan_out(n, ref.n_verts))
            compare(st, ref, got, lambda sl: rows[:n][sl], lambda sl: np.zeros(sl.stop - sl.start, bool), tmpl32, cn)
            out["sizes"][("flame", n)] = st
            del got
            continue
        ts, fps, counts = plan_for(n)
        plan = S.SeekPlan(ts, fps, query_counts=counts)
        assert plan.n_queries == n and plan.n_frames == rows.shape[0]
        src, w = MeshRef64.seek_plan(ts, fps, query_counts=counts)
        st.plan_equal = bool(np.array_equal(plan.src.cpu().numpy(), src) and np.array_equal(plan.w.cpu().numpy().view(np.uint32), w.view(np.uint32)))
        st.cases = plan_cases(ts, fps, counts)
        assert st.plan_equal, f"{n} queries: seek_plan_kernel's plan differs from the host restatement"     # not run on a wrong plan
        d_src, d_w = torch.from_numpy(src).to(dev), torch.from_numpy(w).to(dev)
        poison_workspace(ms, n)
        got = ms.get_mesh_seek(rows, plan, out=nan_out(n, ref.n_verts))
        edge = ((src[:, 0] == FLAME_EDGE_ROW) & (w[:, 0] != 0)) | ((src[:, 1] == FLAME_EDGE_ROW) & (w[:, 1] != 0))
        blended = lambda sl: MeshRef64.blend(rows, d_src[sl], d_w[sl])
        compare(st, ref, got, blended, lambda sl: edge[sl], tmpl32, cn)
        out["sizes"][("flame", n)] = st
        plans[n] = (plan, d_src, d_w)
        if n == sizes[2]:    # the smallest 128 x 128 size (513 on 256 CUs): the two-step form, the controls' frames
            two = plan.rows(rows)
            out["bits"][f"two_step_{n}"] = same_bits(ms.get_mesh(two), got)
            fr = pick_host_frames(st)
            fi = torch.from_numpy(fr).to(dev)
            out["host"] = dict(n=n, frames=fr, d=MeshRef64.blend(rows, d_src[fi], d_w[fi]).cpu(), verts=got[fi].cpu(), edge=st.edge[fr], zero=st.zero[fr])
            del two
        if n == VARIANT_SIZE:    # 512 queries, Qpad 1536 = 6 x 256 (the largest 64 x 64 size on 256 CUs)
            # seek_rows against the three rounded operations: past 93 queries of 89,784 columns the grid-stride loop runs
            want = MeshRef64.blend(rows, d_src, d_w)
            two = plan.rows(rows)
            out["bits"]["seek_rows_89784"] = width == 89784 and two.data_ptr() % 16 == 0 and rows.data_ptr() % 16 == 0 and same_bits(two, want)
            del two
            narrow = rows[:, :15069].contiguous()
            out["bits"]["seek_rows_15069"] = same_bits(plan.rows(narrow), want[:, :15069])
            del narrow
            # input and output 4 bytes past an aligned allocation, through the C ABI; NaN guard elements on both sides
            src_buf = torch.full((rows.numel() + 2,), float("nan"), dtype=torch.float32, device=dev)
            src_buf[1:-1] = rows.reshape(-1)
            dst_buf = torch.full((n * width + 2,), float("nan"), dtype=torch.float32, device=dev)
            p = lambda t: C.c_void_p(t.data_ptr())
            check(lib.sdfa_seek_rows(p(src_buf[1:]), width, p(plan.src), p(plan.w), n, p(dst_buf[1:]), None))
            torch.cuda.synchronize()
            out["bits"]["seek_rows_offset4"] = (src_buf[1:].data_ptr() % 16 == 4 and dst_buf[1:].data_ptr() % 16 == 4
                                                and same_bits(dst_buf[1:-1].view(n, width), want) and bool(torch.isnan(dst_buf[[0, -1]]).all())
                                                and bool(torch.isnan(src_buf[[0, -1]]).all()))
            del src_buf, dst_buf, want
            # the fp32 GEMM variants, bitwise
            out["bits"]["variant_qpad"] = round_up(3 * n)
            for v in VARIANTS:
                try:
                    _lib.set_option("gemm_variant", v)
                    poison_workspace(ms, n)
                    gv = ms.get_mesh_seek(rows, plan, out=nan_out(n, ref.n_verts))
                    torch.cuda.synchronize()
                finally:
                    _lib.set_option("gemm_variant", 0)
                out["bits"][f"variant_{v}"] = same_bits(gv, got)
                del gv
        if n == sizes[3]:    # the fat kernel's size (8789): the two-step form materialises 3.2 GB of rows: freed at once
            two = plan.rows(rows)
            got2 = ms.get_mesh(two)
            del two
            out["bits"][f"two_step_{n}"] = same_bits(got2, got)
            del got2
        del got
    # ------------------------------------------------------------ workspace reuse: 8789, then 1, then 43 frames on one solver
    big = sizes[3]
    plan = plans[big][0]
    ms.get_mesh_seek(rows, plan)                                     # leaves its rhs / sol in the workspace
    r43 = torch.cat([rows, 0.5 * rows[:43 - rows.shape[0]]])
    used1, used43 = ms.get_mesh(rows[:1]), ms.get_mesh(r43)
    fresh = make_solver(m)
    out["bits"]["reuse_1"] = same_bits(mesh_into(fresh, rows[:1], nan_out(1, ref.n_verts)), used1)
    out["bits"]["reuse_43"] = same_bits(mesh_into(fresh, r43, nan_out(43, ref.n_verts)), used43)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def measured(golden):
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    out = measure(golden)
    torch.cuda.synchronize()
    out["seconds"] = time.time() - t0
    out["peak_bytes"] = torch.cuda.max_memory_allocated()
    return out


@pytest.fixture(scope="module")
def flame_ref_cpu(golden):
    return make_ref(meshes(golden)["flame"], "cpu")


def worst(out, key):
    return max(st.stat(key) for st in out["sizes"].values())


def table(out):
    lines = [f"CUs {out['cus']}  ({out.get('seconds', 0):.0f} s, peak {out.get('peak_bytes', 0) / 2**30:.1f} GiB)"]
    for (name, n), st in out["sizes"].items():
        lines.append(f"{name:9s} {n:5d}  {st.form:23s} abs {st.stat('abs'):.2e} rel {st.stat('rel'):.2e}  edge abs {st.stat('edge_abs'):.2e} rel {st.stat('edge_rel'):.2e}"
                     f"  rest {st.rest_err:.1e} ({int(st.zero.sum())} frames)  finite {st.finite} pinned {st.pinned} plan {st.plan_equal} {st.cases or ''}")
    lines.append("worst  " + "  ".join(f"{k} {worst(out, k):.2e}" for k in BOUNDS))
    lines.append("bits   " + json.dumps(out["bits"]))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- tests
def test_sizes_hit_every_launch_form(measured):
    cus = measured["cus"]
    sizes = sizes_for(cus)
    if cus == 256:
        assert sizes == [1, 512, 513, 8789, 8790]
        assert [mesh_form(1280, n, cus) for n in sizes] == [SMALL, SMALL, TILE, FAT, TILE]
    assert len(sizes) == 5, sizes
    ran = {st.form for (name, n), st in measured["sizes"].items() if name == "flame"}
    assert ran == {mesh_form(1280, n, cus) for n in range(1, FLAME_LIMIT)} == {SMALL, TILE, FAT}
    assert [n for (name, n) in measured["sizes"] if name == "flame"] == flame_sizes(cus)
    for name in ("corres", "grid16x8", "grid43x3"):
        assert [n for (nm, n) in measured["sizes"] if nm == name] == list(SMALL_SIZES)
    # ld = round_up(3 * frames, 128): 128 up to 42 frames, 256 from 43, 384 from 86, 512 at 130 (390 columns, 122 of padding)
    assert [round_up(3 * n) for n in SMALL_SIZES] == [128, 128, 128, 256, 256, 384, 512]
    print("\n" + table(measured))


def test_seek_plan_kernel_equals_the_host_restatement(measured):
    """Indices and weights of the four-clip plan at every size, bit for bit; each plan has queries before a clip's first timestamp,
    after its last and exactly on one."""
    planned = {k: st for k, st in measured["sizes"].items() if st.plan_equal is not None}
    assert len(planned) == len(flame_sizes(measured["cus"])) - 1, list(planned)
    for k, st in planned.items():
        assert st.plan_equal, k
        assert min(st.cases.values()) > 0, (k, st.cases)
        assert st.edge.any() and st.zero.any() and not st.edge.all(), k


def test_every_element_written_constraints_pinned_rest_pose(measured):
    for k, st in measured["sizes"].items():
        assert st.finite, k                                   # output and workspace were NaN before the call
        assert st.pinned, k                                   # constrained vertices: the template's bits
        assert st.rest_err <= REST_POSE, (k, st.rest_err)
        assert st.zero.any() or st.n < 3, k


@pytest.mark.parametrize("key", list(BOUNDS))
def test_mesh_against_float64(measured, key):
    print("\n" + table(measured))
    got = {k: st.stat(key) for k, st in measured["sizes"].items()}
    assert max(got.values()) <= BOUNDS[key], (key, got)


def test_fused_seek_gives_the_two_step_bits(measured):
    """get_mesh(plan.rows(rows)) == get_mesh_seek(rows, plan) at the smallest 128 x 128 size and at the fat kernel's."""
    sizes = sizes_for(measured["cus"])
    assert measured["bits"][f"two_step_{sizes[2]}"] and measured["bits"][f"two_step_{sizes[3]}"], measured["bits"]


def test_seek_rows_is_the_three_rounded_operations(measured):
    """plan.rows against blend() bit for bit, 512 queries (the grid-stride loop runs): 16-byte accesses at width 89,784,
    seek_rows_kernel<1> at width 15,069 and for rows 4 bytes past an aligned allocation, nothing written outside them."""
    b = measured["bits"]
    assert b["seek_rows_89784"] and b["seek_rows_15069"] and b["seek_rows_offset4"], b


def test_fp32_gemm_variants_are_bitwise_at_flame_depth(measured):
    """gemm_variant 2, 5, 6 and 8 at K = 1280: the 128 x 128 and 64 x 64 forms, gemm_big_kernel and gemm_fat_kernel give the
    default's vertices, so all of them stand under the float64 bound the default is held to."""
    b = measured["bits"]
    assert b["variant_qpad"] % 256 == 0 and 1280 % 256 == 0, b
    assert all(b[f"variant_{v}"] for v in VARIANTS), b


def test_small_call_after_a_large_one_gives_a_fresh_solvers_bits(measured):
    b = measured["bits"]
    assert b["reuse_1"] and b["reuse_43"], b


# ------------------------------------------------------------------------------------------------------ sensitivity controls
def control_miss(measured, ref, **inject):
    """Per kept frame and vertex, |gpu - failing reference|, and each frame's bound."""
    h = measured["host"]
    bad = ref.get_mesh(h["d"], **inject)
    miss = (h["verts"].double() - bad).abs().amax(2).numpy()                      # (frames, vertices)
    bound = np.where(h["edge"], BOUNDS["edge_abs"], BOUNDS["abs"])
    return h, miss, bound


def test_good_reference_passes_on_the_kept_frames(measured, flame_ref_cpu):
    h, miss, bound = control_miss(measured, flame_ref_cpu)
    assert (miss.max(1) <= bound).all(), (miss.max(1), bound)
    assert h["zero"][0] and h["edge"][1] and not h["edge"][2:].any() and not h["zero"][1:].any()


def test_bounds_catch_a_dropped_incidence(measured, flame_ref_cpu):
    """One incidence of one free vertex without its (T - I) c term: every deformed frame misses at that vertex; the rest pose, where
    the term is zero, stays within the bound."""
    ref = flame_ref_cpu
    v = int(ref.free[len(ref.free) // 2])
    hits = np.nonzero(ref.a_vert == v)[0]            # an incidence whose triangle turns by 1 or more in the rotation-edge row, so that
    k = next(i for i, e in enumerate(hits) if EDGE_NORMS[ref.eq_src[ref.a_eq[e]] % len(EDGE_NORMS)] >= 1.0)      # its term is not ~0 there
    h, miss, bound = control_miss(measured, ref, drop_incidence=(v, k))
    deformed = ~h["zero"]
    assert (miss[deformed, v] > bound[deformed]).all(), (miss[:, v], bound)
    assert miss[~deformed].max() <= BOUNDS["abs"]


def test_bounds_catch_a_stale_frame(measured, flame_ref_cpu):
    """Frame 3 solved from frame 6's transforms: that frame misses, the others stay within their bounds."""
    h, miss, bound = control_miss(measured, flame_ref_cpu, stale_frame=(3, 6))
    worst_of = miss.max(1)
    others = np.arange(len(worst_of)) != 3
    assert worst_of[3] > bound[3] and (worst_of[others] <= bound[others]).all(), (worst_of, bound)


def test_bounds_catch_a_skipped_k_block(measured, flame_ref_cpu):
    """Row tile 4 (unknowns 512 .. 639) without K block 17 (unknowns 544 .. 575): the vertices of that tile miss in every deformed
    frame, every other vertex stays within the bound."""
    ref = flame_ref_cpu
    h, miss, bound = control_miss(measured, ref, skip_k_block=(4, 17))
    in_tile = np.zeros(ref.n_verts, bool)
    in_tile[ref.free[512:640]] = True
    deformed = ~h["zero"]
    assert (miss[deformed][:, in_tile].max(1) > bound[deformed]).all(), (miss[:, in_tile].max(1), bound)
    assert (miss[:, ~in_tile].max(1) <= bound).all(), (miss[:, ~in_tile].max(1), bound)
    assert miss[~deformed].max() <= BOUNDS["abs"]


if __name__ == "__main__":
    class _Golden:
        def __getitem__(self, name):
            return np.load(os.path.join(_HERE, "golden", name + ".npz"))
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    res = measure(_Golden())
    torch.cuda.synchronize()
    res["seconds"], res["peak_bytes"] = time.time() - t0, torch.cuda.max_memory_allocated()
    print(table(res))
