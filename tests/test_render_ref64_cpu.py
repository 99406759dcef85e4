"""The numpy restatement of the rasterizer (tests/render_oracle.py, which the GPU tests compare the kernels with bit for bit)
against an independent float64 ray caster (tests/render_ref64.py), on the CPU.

Visibility: the ids of every sample must be equal wherever the sample is farther than 1/256 pixel from every projected edge
of a drawn triangle and the two nearest depths differ by more than 1e-5 relative.  The band is derived: snapping moves a vertex
at most 1/512 pixel per axis, the fp32 projection error at |X| <= 8192 is below 2^-10 pixel, together an edge moves less than
1/256 pixel.  Colour: on pixels whose samples all agree, |oracle - ref64| <= 0.75 + 2 max|c64(sample displaced by +-1/256 pixel,
same triangle's plane) - c64| levels (0.5 final rounding, 0.25 fp32 shading, the rest snapping to first order); a pixel whose
bound exceeds 3 levels is excluded.  Excluded samples (band, depth tie, colour bound) must be at most 3 % of the covered samples
in every case: the cap is a condition on the cases chosen, not a measurement.

Seven controls (patched copies of the oracle's source) must turn the comparison red."""
import os
import types

import numpy as np
import pytest

import render_oracle as R
import render_ref64 as R64
import render_scenes as SC

BAND_PX = 1.0 / 256.0
DEPTH_TIE = 1e-5
MAX_BOUND = 3.0
CAP = 0.03
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rotated(verts, seed):                      # as in test_render_gpu.py
    rs = np.random.RandomState(seed)
    axis = rs.randn(3)
    axis /= np.linalg.norm(axis)
    ang = rs.uniform(0.3, 0.8)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    c = verts.mean(0)
    return ((verts - c) @ Rm.T + c).astype(np.float32)


def _case(name, template, faces, verts, size, params):
    return dict(name=name, template=template, faces=np.asarray(faces, np.uint32), verts=verts, size=size, params=params)


def _build_cases():
    g = np.load(os.path.join(GOLDEN, "mesh_flame.npz"))
    tv, tf = g["verts"].astype(np.float32), g["faces"].astype(np.uint32)
    frames = dict(template=tv, deformed=g["mesh"][2].astype(np.float32), rotated=_rotated(tv, 7))
    cases = []
    for fname, v in frames.items():
        for size in ((512, 512), (301, 170)):
            cases.append(_case(f"flame-{fname}-{size[0]}x{size[1]}", tv, tf, v, size, {}))
    cases.append(_case("flame-rotated-512x512-camera2-coloured", tv, tf, frames["rotated"], (512, 512), dict(SC.CAMERA2, **SC.COLOURED)))
    cases.append(_case("flame-deformed-301x170-coloured", tv, tf, frames["deformed"], (301, 170), SC.COLOURED))

    def synth(name, sc, size, params=None):
        rs = np.random.RandomState(len(cases))
        verts = sc["verts"] + rs.normal(0, 2e-3, sc["verts"].shape).astype(np.float32) if name.endswith("-moved") else sc["verts"]
        cases.append(_case(f"{name}-{size[0]}x{size[1]}", sc["verts"], sc["faces"], verts, size, sc["params"] if params is None else params))
    ewb = SC.ellipsoid_wall_blade()
    for size in ((256, 256), (301, 170), (33, 31)):
        synth("ellipsoid", ewb, size)
        synth("close", SC.close(), size)
    synth("ellipsoid-moved", ewb, (256, 256))                                   # frame normals differ from template normals
    synth("ellipsoid-camera2-coloured", ewb, (301, 170), dict(SC.CAMERA2, **SC.COLOURED))
    synth("ellipsoid-coloured", ewb, (256, 256), SC.COLOURED)
    synth("grid513", SC.grid(513), (256, 256))
    synth("facets", SC.facets(), (256, 256))
    synth("guard_band", SC.guard_band(), (256, 256))
    return cases


CASES = _build_cases()
BY_NAME = {c["name"]: c for c in CASES}


class _Cache:
    """Reference and unpatched-oracle results, computed once per (case, samples[, normals]) and never changed."""

    def __init__(self):
        self.vis, self.col, self.raster = {}, {}, {}

    def visibility(self, case, S):
        key = (case["name"], S)
        if key not in self.vis:
            rig = R64.Rig(case["template"], *case["size"], case["params"])
            self.vis[key] = (rig,) + R64.visibility(rig, case["verts"], case["faces"], S)
        return self.vis[key]

    def colour(self, case, S, normals):
        key = (case["name"], S, normals)
        if key not in self.col:
            rig, tid = self.visibility(case, S)[:2]
            nv = case["template"] if normals == "template" else case["verts"]
            self.col[key] = R64.colour_and_bound(rig, case["verts"], nv, case["faces"], tid)
        return self.col[key]


@pytest.fixture(scope="module")
def cache():
    return _Cache()


def _oracle(O, case, S, normals, memo=None):
    """O.render of the case, with the raster stage's answer for all S samples caught on the way (and, for the unpatched
    oracle, kept: it does not depend on the normals mode)."""
    orig, box = O.raster, {}

    def raster(scr, faces, w, h, s):
        key = (case["name"], S)
        if memo is not None and key in memo:
            box["v"] = memo[key]
        else:
            box["v"] = orig(scr, faces, w, h, s)
            if memo is not None:
                memo[key] = box["v"]
        return box["v"]
    O.raster = raster
    try:
        rgb, _, scr = O.render(case["template"], case["faces"], case["verts"], case["size"][0], case["size"][1], S, normals, case["params"])
    finally:
        O.raster = orig
    btri = box["v"][0]
    return rgb, np.where(btri == R.INT_MAX, -1, btri), scr


def compare(O, case, S, normals, cache, memo=None):
    """Figures of one comparison; check() asserts on them."""
    rgb, ids, _ = _oracle(O, case, S, normals, memo)
    rig, tid, d1, d2, edge = cache.visibility(case, S)
    c64, bound = cache.colour(case, S, normals)
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(d2) & (d2 - d1 <= DEPTH_TIE * d1)
    excl_vis = (edge < BAND_PX) | tie
    differ = ids != tid
    agree_px = ~differ.any(2)
    excl_col = bound > MAX_BOUND
    err = np.abs(rgb.astype(np.float64) - c64).max(2)
    judged = agree_px & ~excl_col
    ratio = float((err[judged] / bound[judged]).max()) if judged.any() else 0.0
    counts = (tid >= 0) | (ids >= 0)
    covered = int((tid >= 0).sum())
    excluded = int(((excl_vis | excl_col[:, :, None]) & counts).sum())
    return dict(case=case["name"], samples=S, normals=normals, covered=covered, differ=int(differ.sum()),
                bad_ids=int((differ & ~excl_vis).sum()), where=np.argwhere(differ & ~excl_vis)[:5].tolist(),
                share=excluded / max(covered, 1), ratio=ratio, raw=float(err[judged].max()) if judged.any() else 0.0,
                white=float((rgb[tid.max(2) >= 0] == 255).all(1).mean()) if covered else 0.0)


def check(st):
    print(f"{st['case']:42s} S={st['samples']} {st['normals']:8s} covered {st['covered']:7d}  ids differing {st['differ']:4d} "
          f"(outside the band {st['bad_ids']})  excluded {100 * st['share']:5.2f} %  |oracle-ref64| max {st['raw']:5.2f} levels, "
          f"{st['ratio']:4.2f} of the bound")
    assert st["covered"] > 0, "an empty image proves nothing"
    assert st["bad_ids"] == 0, f"{st['case']}: visibility differs outside the band at (y, x, sample) {st['where']}"
    assert st["ratio"] <= 1.0, f"{st['case']}: colour is {st['ratio']:.2f} of the bound"
    assert st["share"] <= CAP, f"{st['case']}: {100 * st['share']:.2f} % of the covered samples excluded"


def red(st):
    return st["bad_ids"] > 0 or st["ratio"] > 1.0


@pytest.fixture(scope="module")
def memo():
    return {}


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_oracle_against_float64_ray_caster(name, samples, cache, memo):
    case = BY_NAME[name]
    for normals in ("template", "frame"):
        st = compare(R, case, samples, normals, cache, memo)
        check(st)
        if name.startswith("close"):
            assert st["white"] < 0.2, "the close scene must not saturate: a white image proves nothing for colour"


def test_guard_band_scene_drops_what_it_is_there_for():
    sc = SC.guard_band()
    k = R.consts(sc["verts"], 256, 256, sc["params"])
    scr, pos = R.vertex_stage(sc["verts"], k)
    out = (scr[:-1, 3] == 0) & (-pos[:-1, 2] > k["znear"])
    assert out.sum() >= 2, "no vertex beyond the guard band in front of the near plane"
    faces = sc["faces"].astype(np.int64)
    assert out[faces[sc["dropped_faces"]]].any(1).all()
    _, ids, _ = R.render(sc["verts"], sc["faces"], sc["verts"], 256, 256, 1, "template", sc["params"])
    assert not np.isin(ids, sc["dropped_faces"]).any() and (ids == 2).sum() > 1000 and (ids >= 3).sum() > 1000
    # the slivers: drawn, with a vertex in the last pixel of the band on the negative side
    vx, vy = sc["edge_verts"]
    assert scr[vx, 3] == 1 and -32768 * 256 <= scr[vx, 0] < -32767 * 256
    assert scr[vy, 3] == 1 and -32768 * 256 <= scr[vy, 1] < -32767 * 256
    assert all((ids == f).sum() > 1000 for f in sc["edge_faces"])
    # without the guard band both would cover the image centre: the rule is what removes them
    rig = R64.Rig(sc["verts"], 256, 256, sc["params"])
    cam = rig.camera(sc["verts"])
    for f in sc["dropped_faces"]:
        a, b, c = cam[faces[f]]
        vol = [np.dot((0.0, 0.0, -1.0), np.cross(p, q)) for p, q in ((b, c), (c, a), (a, b))]
        assert max(vol) < 0, "the dropped triangle does not cross the image centre"


def test_ties_scene_first_copy_owns_every_sample():
    """Every covered sample of this scene is an exact depth tie, which the float64 comparison excludes by definition: the
    tie rule (smaller index) is checked on the oracle directly."""
    sc = SC.ties()
    n = sc["n_fan"]
    for S in (1, 4):
        k = R.consts(sc["verts"], 256, 256, sc["params"])
        scr, _ = R.vertex_stage(sc["verts"], k)
        btri, z = R.raster(scr, sc["faces"], 256, 256, S)
        alone, z1 = R.raster(scr, sc["faces"][:n], 256, 256, S)
        far, z3 = R.raster(scr, sc["faces"][-n:], 256, 256, S)
        assert (alone != R.INT_MAX).sum() > 10000
        assert np.array_equal(btri, alone) and np.array_equal(z, z1), "a later copy or a filler owns a sample"
        assert np.array_equal(z3, z1) and np.array_equal(far != R.INT_MAX, alone != R.INT_MAX), "the third copy is not an exact tie"
        assert len(sc["faces"]) - n > 256 + n


def test_scenes_are_what_they_claim():
    for sc in (SC.ellipsoid_wall_blade(), SC.close(), SC.guard_band(), SC.ties(), SC.stack(), SC.grid(257), SC.facets()):
        assert np.abs(sc["verts"]).max() == np.float32(0.15) and R.consts(sc["verts"], 256, 256, sc["params"])["s"] == np.float32(1.0)
    # blade vertices and the anchor have zero normals, bit for bit, in the oracle and in the reference
    sc = SC.ellipsoid_wall_blade()
    zero = list(sc["blade_verts"]) + [len(sc["verts"]) - 1]
    assert not R.vertex_normals(sc["verts"], sc["faces"], np.float32(1.0))[zero].any()
    assert not R64.vertex_normals(R64.Rig(sc["verts"], 256, 256), sc["verts"], sc["faces"])[zero].any()
    # close: vertices of drawn triangles lie a thousand pixels outside on every side, the doubled area is far above 2^24
    sc = SC.close()
    scr, _ = R.vertex_stage(sc["verts"], R.consts(sc["verts"], 256, 256, sc["params"]))
    btri, _ = R.raster(scr, sc["faces"], 256, 256, 1)
    seen = np.unique(btri[btri != R.INT_MAX])
    p = scr[sc["faces"].astype(np.int64)[seen]].astype(np.int64)
    assert p[:, :, 3].all()
    assert p[:, :, 0].min() < -1000 * 256 and p[:, :, 0].max() > (256 + 1000) * 256
    assert p[:, :, 1].min() < -1000 * 256 and p[:, :, 1].max() > (256 + 1000) * 256
    D = R.edge(p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1], p[:, 2, 0], p[:, 2, 1])
    assert D.max() > 2 ** 36 and (D.astype(np.float32).astype(np.int64) != D).any(), "(float)D must round"
    # stack: every triangle's box contains the tile (96..127)^2 's centre pixel
    sc = SC.stack()
    scr, _ = R.vertex_stage(sc["verts"], R.consts(sc["verts"], 256, 256))
    p = scr[sc["faces"].astype(np.int64)]
    assert len(p) == 600 and (p[:, :, 0].min(1) < 112 * 256).all() and (p[:, :, 0].max(1) > 112 * 256).all()
    assert (p[:, :, 1].min(1) < 112 * 256).all() and (p[:, :, 1].max(1) > 112 * 256).all()
    btri, _ = R.raster(scr, sc["faces"], 256, 256, 1)
    assert len(np.unique(btri[btri != R.INT_MAX])) > 20 and btri[112, 112, 0] != R.INT_MAX


# ---- controls: a patched copy of the oracle must be caught ----

def _patched(*edits):
    src = open(R.__file__.replace(".pyc", ".py")).read()
    for old, new, count in edits:
        assert src.count(old) == count, (old, src.count(old))
        src = src.replace(old, new)
    mod = types.ModuleType("render_oracle_control")
    exec(compile(src, "render_oracle_control", "exec"), mod.__dict__)
    return mod


CONTROLS = {
    "affine": ([("c0, c1, c2 = q0 * iz, q1 * iz, q2 * iz", "c0, c1, c2 = w0, w1, w2", 1)], "close-256x256", 4, "template"),
    "y_not_flipped": ([('Y = (F32(1.0) - (cy * k["fy"]) * iw) * k["hh"]', 'Y = (F32(1.0) + (cy * k["fy"]) * iw) * k["hh"]', 1)],
                      "ellipsoid-256x256", 1, "template"),
    "clockwise_front": ([("f = np.asarray(faces, np.int64).reshape(-1, 3)\n", "f = np.asarray(faces, np.int64).reshape(-1, 3)[:, ::-1]\n", 3)],
                        "ellipsoid-256x256", 1, "template"),
    "fx_with_h_over_w": ([("fy / (float(width) / float(height))", "fy / (float(height) / float(width))", 1)], "ellipsoid-301x170", 1, "template"),
    "smaller_iw_nearer": ([("samples), -np.inf, np.float32)", "samples), np.inf, np.float32)", 1), ("(z > bz)", "(z < bz)", 1)],
                          "ellipsoid-256x256", 4, "template"),
    "r_b_swapped": ([("return np.rint(acc * F32(255.0)).astype(np.uint8)", "return np.rint(acc * F32(255.0)).astype(np.uint8)[:, :, ::-1]", 1)],
                    "ellipsoid-coloured-256x256", 4, "template"),
    "frame_normals_for_template": ([('template_verts if normals == "template" else verts, faces', "verts, faces", 1)],
                                   "ellipsoid-moved-256x256", 4, "template"),
}


@pytest.mark.parametrize("control", sorted(CONTROLS))
def test_control_turns_the_comparison_red(control, cache, memo):
    edits, name, S, normals = CONTROLS[control]
    case = BY_NAME[name]
    assert not red(compare(R, case, S, normals, cache, memo)), "the unpatched oracle must be green on the control's case"
    st = compare(_patched(*edits), case, S, normals, cache)
    print(f"control {control}: ids differing outside the band {st['bad_ids']}, colour {st['ratio']:.2f} of the bound")
    assert red(st), f"the comparison does not notice {control}"
