"""The GPU rasterizer (csrc/render.hip via sdfa_amd.render) against its numpy restatement (tests/render_oracle.py, itself held to
the float64 ray caster by tests/test_render_ref64_cpu.py) on the synthetic scenes of tests/render_scenes.py: the launch forms,
store paths, drop rules, tie rule and parameters that the FLAME renders of test_render_gpu.py never reach.  Every comparison is
the one made there: snapped screen positions and visibility bitwise, colour within +-1 per channel."""
import numpy as np
import pytest
import torch

import render_oracle as R
import render_scenes as SC

pytestmark = pytest.mark.gpu

SCENES = {"ellipsoid_wall_blade": SC.ellipsoid_wall_blade, "close": SC.close, "guard_band": SC.guard_band, "ties": SC.ties,
          "stack": SC.stack, "facets": SC.facets}
SCENES.update({f"grid{T}": (lambda T=T: SC.grid(T)) for T in (1, 255, 256, 257, 513)})
SMALL_SIZES = [(301, 170), (33, 31), (31, 33), (5, 3), (1, 1), (2048, 8)]
MATRIX = [(name, (256, 256)) for name in SCENES] + [(name, size) for name in ("ellipsoid_wall_blade", "close") for size in SMALL_SIZES]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _params(d):
    """A dict over render_oracle.DEFAULT_PARAMS -> sdfa_render_params."""
    from sdfa_amd.render import Params
    full = dict(R.DEFAULT_PARAMS, **d)
    p = Params()
    p.cam_pose[:] = [float(x) for x in np.asarray(full["cam_pose"], np.float32).reshape(-1)]
    for name in ("yfov", "znear", "ambient", "dir_intensity", "point_intensity"):
        setattr(p, name, float(np.float32(full[name])))
    p.albedo[:] = [float(x) for x in np.asarray(full["albedo"], np.float32)]
    p.background[:] = [float(x) for x in np.asarray(full["background"], np.float32)]
    return p


def _renderer(sc, size, samples, params=None, normals=None):
    from sdfa_amd.render import Renderer
    return Renderer(sc["verts"], sc["faces"], size, samples=samples, normals=normals or sc["normals"],
                    params=_params(sc["params"] if params is None else params))


@pytest.fixture(scope="module")
def scenes():
    built = {}

    def get(name):
        if name not in built:
            built[name] = SCENES[name]()
        return built[name]
    return get


@pytest.fixture(scope="module")
def oracle(scenes):
    """(rgb, ids, scr) of the oracle, once per (scene, size, samples, rig)."""
    done = {}

    def get(name, size, samples, rig=None, verts=None, key=None):
        k = (name, size, samples, rig, key)
        if k not in done:
            sc = scenes(name)
            params = sc["params"] if rig is None else getattr(SC, rig)
            done[k] = R.render(sc["verts"], sc["faces"], sc["verts"] if verts is None else verts, size[0], size[1], samples, sc["normals"], params)
        return done[k]
    return get


def _same(rgb, ids, scr, o, what):
    o_rgb, o_ids, o_scr = o
    if scr is not None:
        assert np.array_equal(scr, o_scr), f"{what}: snapped screen positions differ"
    assert np.array_equal(ids, o_ids), f"{what}: visibility differs at {np.argwhere(ids != o_ids)[:5].tolist()}"
    d = int(np.abs(rgb.astype(np.int32) - o_rgb.astype(np.int32)).max())
    assert d <= 1, f"{what}: colour differs by {d}"


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name,size", MATRIX, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in MATRIX])
def test_scene_matches_oracle(name, size, samples, scenes, oracle):
    sc = scenes(name)
    r = _renderer(sc, size, samples)
    v = _cuda(sc["verts"][None])
    scr = r.screen(v)[0].cpu().numpy()
    rgb, ids = r.render(v, want_ids=True)
    rgb, ids = rgb[0].cpu().numpy(), ids[0].cpu().numpy()
    o = oracle(name, size, samples)
    _same(rgb, ids, scr, o, f"{name} {size} samples={samples}")
    o_ids = o[1]
    if size == (256, 256):                       # the scene shows what it is there for
        if name == "ties":
            assert (o_ids >= 0).sum() > 10000 and o_ids.max() < sc["n_fan"], "a later copy owns a sample"
        elif name == "guard_band":
            assert not np.isin(o_ids, sc["dropped_faces"]).any() and (o_ids == 2).sum() > 1000
        elif name == "stack":
            assert len(np.unique(o_ids[96:128, 96:128])) > 10
        elif name == "facets":
            assert len(np.unique(o_ids)) > 300
        elif name == "close":
            assert (o_ids >= 0).all() and len(np.unique(o_ids)) <= 8
        elif name.startswith("grid"):
            assert len(np.unique(o_ids[o_ids >= 0])) > 0.3 * (int(name[4:]) - 1), "triangles of ~1 pixel: a good part holds a sample"
        else:
            assert np.isin(sc["blade_faces"], o_ids).any(), "the blade (zero normals) is not visible"


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("size,offset", [((300, 170), 1), ((256, 256), 1), ((301, 170), 0)])
def test_output_not_dword_aligned_takes_the_byte_store_path(size, offset, samples, scenes, oracle):
    """wide == 0 for full tiles: an output one byte off a dword boundary with W % 4 == 0, and W % 4 != 0 at offset 0."""
    sc = scenes("ellipsoid_wall_blade")
    W, H = size
    n, pad = H * W * 3, 64
    r = _renderer(sc, size, samples, SC.COLOURED)
    v = _cuda(sc["verts"][None])
    plain, ids = r.render(v, want_ids=True)
    _same(plain[0].cpu().numpy(), ids[0].cpu().numpy(), None, oracle("ellipsoid_wall_blade", size, samples, "COLOURED"), f"{size} aligned")
    buf = torch.full((pad + offset + n + pad + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    out = buf[pad + offset:pad + offset + n].view(1, H, W, 3)
    assert out.data_ptr() % 4 == offset and out.is_contiguous()
    r.render(v, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, plain), "the render into the view differs from the aligned render"
    host = buf.cpu().numpy()
    assert (host[:pad + offset] == 0xA5).all(), "bytes before the image were written"
    assert (host[pad + offset + n:] == 0xA5).all(), "bytes behind the image were written"


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("n", [65, 130])
def test_more_frames_than_one_chunk(n, samples, scenes, oracle):
    from sdfa_amd.render import CHUNK_FRAMES
    assert CHUNK_FRAMES == 64
    sc = scenes("ellipsoid_wall_blade")
    size = (33, 31)
    rs = np.random.RandomState(n)
    batch = sc["verts"][None] + rs.normal(0, 2e-3, (n,) + sc["verts"].shape).astype(np.float32)
    r = _renderer(sc, size, samples)
    v = _cuda(batch)
    rgb, ids = r.render(v, want_ids=True)
    scr = r.screen(v).cpu().numpy()
    rgb, ids = rgb.cpu().numpy(), ids.cpu().numpy()
    for i in (0, 63, 64, n - 1):
        _same(rgb[i], ids[i], scr[i], oracle("ellipsoid_wall_blade", size, samples, verts=batch[i], key=(n, i)), f"frame {i} of {n}")
    for i in range(n):
        one = r.render(v[i:i + 1])[0].cpu().numpy()
        assert np.array_equal(one, rgb[i]), f"frame {i} of {n} differs from its batch-of-one render"


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("rig", ["COLOURED", "AMBIENT_ONLY", "SATURATING", "CAMERA2"])
def test_custom_parameters(rig, samples, scenes, oracle):
    sc = scenes("ellipsoid_wall_blade")
    size = (256, 256)
    r = _renderer(sc, size, samples, getattr(SC, rig))
    v = _cuda(sc["verts"][None])
    scr = r.screen(v)[0].cpu().numpy()
    rgb, ids = r.render(v, want_ids=True)
    o = oracle("ellipsoid_wall_blade", size, samples, rig)
    _same(rgb[0].cpu().numpy(), ids[0].cpu().numpy(), scr, o, f"{rig} samples={samples}")
    o_rgb, o_ids, _ = o
    lit = o_rgb[o_ids >= 0]
    assert len(lit) > 20000
    if rig != "CAMERA2":
        assert not (lit[:, 0] == lit[:, 2]).all(), "red and blue must differ for a channel swap to show"
    if rig == "SATURATING":
        assert 0.2 < (lit[:, 0] == 255).mean() < 0.95, "the clamp at 1.0 must act on part of the image"
    if rig == "AMBIENT_ONLY" and samples == 1:
        assert len(np.unique(lit, axis=0)) == 1, "ambient only: one colour"
