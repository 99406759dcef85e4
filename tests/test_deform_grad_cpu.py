"""mesh -> dgrad (deformation.get_deform_grad) without a GPU: the float64 restatement tests/dgrad_ref64.py against the reference's own
output (tests/golden/deform_grad.npz, tests/gen_golden_deform_grad.py), the non-face triangle set, and the host-side checks of the
public calls that run before any device work."""
import numpy as np
import pytest

from dgrad_ref64 import deform_grad64
from sdfa_amd import _lib
from sdfa_amd.mesh import deform_grad, DeformGrad       # noqa: F401  (the mirror of get_deform_grad and its device form)

WELL = ("speech", "1cm", "rot10", "rot90")               # rotations well away from pi: ~1e-14 from the reference
SMALL_WELL = (0, 5, 9, 10)                               # general, 5e-6 rad, 3 rad (well conditioned), identity
SMALL_MIRROR = (1, 2)                                    # det < 0 (reflection: equal singular values), mirrored stretch
SMALL_ILL = (3, 4, 6, 7, 8)                              # angles within 1e-5 of a branch threshold of rotation_log_exp::log


def _flame(golden):
    g = golden["mesh_flame"]
    return g["verts"], g["faces"]


def test_symbol_is_exported():
    assert "sdfa_mesh_deform_grad" in _lib.SYMBOLS and hasattr(_lib.lib, "sdfa_mesh_deform_grad")


def test_restatement_matches_reference_on_flame(golden):
    z = golden["deform_grad"]
    V, F = _flame(golden)
    st = int(z["flame_faces_stride"])
    for i, name in enumerate(z["flame_names"]):
        mine = deform_grad64(V, z["flame_targets"][i], F).reshape(-1, 9)[::st]
        err = float(np.abs(mine - z["flame_dgrad"][i]).max())
        if name in WELL:
            assert err <= 1e-12, (name, err)                # measured <= 7e-15
        else:
            # 179.9 degrees: pi - angle = 1.7e-3, acos and 1 / sin(angle) amplify rounding; the rotation still agrees to 1e-8
            assert name == "rot179.9" and err <= 1e-8, (name, err)


def test_restatement_matches_reference_preload_case(golden):
    z = golden["deform_grad"]
    V, F = _flame(golden)
    from speech_anime.datasets.vocaset_mask import non_face_tris
    mask = non_face_tris(F)
    tgt = V + z["preload_offsets"]                          # float32 + float32, as preload.py:770
    dg = deform_grad64(V, tgt, F).reshape(-1, 9)
    dg[mask] = 0
    assert np.abs(dg[::int(z["flame_faces_stride"])] - z["preload_dgrad"]).max() <= 1e-12
    rows = z["preload_rows_f32"]
    assert np.array_equal(dg.reshape(-1).astype(np.float32)[:len(rows)], rows)


def test_restatement_matches_reference_small_cases(golden):
    z = golden["deform_grad"]
    for k, eps in enumerate(z["small_eps"]):
        for f, tgt in enumerate(z["small_targets"]):
            ref = z["small_dgrad"][k, f].reshape(-1, 9)
            mine, parts = deform_grad64(z["small_src"], tgt, z["small_faces"], eps, return_parts=True)
            mine = mine.reshape(-1, 9)
            nan = np.isnan(ref).any(1)
            assert np.array_equal(nan, np.isnan(mine).any(1))       # coincident vertices: a zero-length edge is not "degenerate"
            assert nan.sum() == 1 and nan[6]
            err = float(np.abs(mine[~nan] - ref[~nan]).max())
            if f in SMALL_WELL:
                assert err <= 1e-12, (eps, f, err)
            elif f in SMALL_MIRROR:
                assert err <= 1e-11, (eps, f, err)          # measured 2.2e-12
            else:
                # branch thresholds: which side a triangle falls on is decided by rounding; the scale part still agrees, and
                # both results reproduce T = R scale to the threshold's accuracy
                assert np.abs(mine[~nan, :6] - ref[~nan, :6]).max() <= 1e-9, (eps, f)
            degenerate = ~parts["good"]
            assert np.all(ref[degenerate] == 0) and np.all(mine[degenerate] == 0)
    # collinear triangles (0..5) are degenerate at both eps; the |cos| = 0.995 sliver (7) only at eps = 1e-2
    _, p6 = deform_grad64(z["small_src"], z["small_targets"][0], z["small_faces"], 1e-6, return_parts=True)
    _, p2 = deform_grad64(z["small_src"], z["small_targets"][0], z["small_faces"], 1e-2, return_parts=True)
    assert not p6["good"][:6].any() and p6["good"][7] and not p2["good"][7]


def test_non_face_triangles_are_the_references(golden):
    from speech_anime.datasets.vocaset_mask import non_face_tris
    _, F = _flame(golden)
    assert int(non_face_tris(F).sum()) == 7375


def test_bad_faces_are_refused_on_the_host(golden):
    V, F = _flame(golden)
    bad = F.astype(np.int64).copy()
    bad[3, 1] = len(V)
    with pytest.raises(ValueError, match="out of range"):
        deform_grad(V, V, bad)


def test_source_mesh_must_be_flame(golden):
    from speech_anime import viewer
    g = golden["mesh"]
    with pytest.raises(ValueError, match="FLAME topology"):
        viewer.set_source_mesh((g["verts"], g["faces"]))
    assert not viewer.has_source_mesh()
    V, F = _flame(golden)
    viewer.set_source_mesh((V, F))
    try:
        assert viewer.has_source_mesh()
    finally:
        viewer.clear_source_mesh()


def test_source_mesh_needs_a_template(tmp_path, golden):
    from speech_anime.api import evaluate_model
    with pytest.raises(ValueError, match="--source_mesh needs --template_mesh"):
        evaluate_model(dict(mode="evaluate", source_mesh=str(tmp_path / "flame.obj")))


def test_cli_accepts_source_mesh():
    from speech_anime.__main__ import _parser
    ns = _parser().parse_args(["evaluate", "--source_mesh", "flame.obj", "--template_mesh", "t.obj"])
    assert ns.source_mesh == "flame.obj"
