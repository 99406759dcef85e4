"""Pins tests/mesh_ref64.py (the float64 restatement the GPU mesh test judges the kernels by) on the CPU: against the fixtures the
reference project's own compiled module and saber.stream.seek produced, against oracle/mesh_oracle.py, by its own residual, and
shows that each injected failure changes its output where it should and nowhere else.  Also the host-side logic of
tests/test_gpu_mesh_ref64.py that needs no GPU: the launch-form restatement, the sizes and the seek plans."""
import numpy as np
import pytest
import torch

from mesh_oracle import MeshOracle
from mesh_ref64 import MeshRef64
import test_gpu_mesh_ref64 as G


def flame_rows(g):
    rows = [np.random.RandomState(int(s)).normal(0, float(sig), (len(g["faces"]), 9)).astype(np.float32)
            for s, sig in zip(g["dgrad_seed"], g["dgrad_sigma"])]
    rows[int(g["rot_only"])][:, :6] = 0.0
    return np.stack(rows).reshape(len(rows), -1)


@pytest.fixture(scope="module")
def all_meshes(golden):
    return G.meshes(golden)


@pytest.fixture(scope="module")
def flame(golden, all_meshes):
    return MeshRef64(**{k: all_meshes["flame"][k] for k in ("verts", "faces", "cnsts")}), flame_rows(golden["mesh_flame"])


def oracle_rounding(mesh):
    """Half a float32 ulp of the largest coordinate (MeshOracle returns float32), and 1 % for the two float64 solves."""
    return 1.01 * float(np.spacing(np.float32(np.abs(mesh).max()))) / 2


def test_ref64_matches_reference_module_small_fixture(golden):
    g = golden["mesh"]
    ref = MeshRef64(g["verts"], g["faces"], g["cnsts"])
    d = g["dgrad"].reshape(len(g["dgrad"]), -1)
    out = ref.get_mesh(d).numpy()
    assert out.dtype == np.float64 and out.shape == g["mesh"].shape
    assert np.abs(out - g["mesh"]).max() <= 1e-7
    assert np.abs(ref.get_mesh(np.zeros_like(d[:1])).numpy()[0] - g["verts"]).max() <= 1e-7          # zero dgrad -> template
    orc = MeshOracle(g["verts"], g["faces"], g["cnsts"])
    for k in range(len(d)):
        assert np.abs(out[k] - orc.get_mesh(d[k])).max() <= oracle_rounding(g["mesh"]), k


def test_ref64_matches_reference_module_at_flame_size(golden, flame):
    g = golden["mesh_flame"]
    ref, rows = flame
    out = ref.get_mesh(rows).numpy()
    for k in (1, 3, 4):
        assert np.abs(out[k] - g["mesh"][k]).max() <= 2e-7, k
    r0, r1 = (int(x) for x in g["blend_rows"])
    t0, t1, q = (int(x) for x in g["blend_ts"])
    src, w = MeshRef64.seek_plan([[t0, t1]], 8.0)                                  # query 1 at 125 ms, between 117 and 133
    assert len(src) == 2 and 1000.0 / 8.0 == q
    blended = MeshRef64.blend(rows[[r0, r1]], src, w)
    assert np.abs(ref.get_mesh(blended).numpy()[1] - g["blend_mesh"]).max() <= 2e-7
    orc = MeshOracle(g["verts"], g["faces"], g["cnsts"])
    assert np.abs(out[3] - orc.get_mesh(rows[3])).max() <= oracle_rounding(g["mesh"])


def test_ref64_correspondences_match_reference_module(golden):
    g = golden["mesh_corres"]
    ref = MeshRef64(g["verts"], g["faces"], g["cnsts"], corr_count=g["corr_count"], corr_faces=g["corr_faces"])
    d = g["dgrad"].reshape(len(g["dgrad"]), -1)
    out = ref.get_mesh(d).numpy()
    assert np.abs(out - g["mesh"]).max() <= 2e-7
    orc = MeshOracle(g["verts"], g["faces"], g["cnsts"], corr_count=g["corr_count"], corr_faces=g["corr_faces"])
    for k in range(len(d)):
        assert np.abs(out[k] - orc.get_mesh(d[k])).max() <= oracle_rounding(g["mesh"]), k


def test_transform_follows_the_references_rule():
    """Identity below an angle of 1e-10, Rodrigues above; against MeshOracle.transform vector by vector, at every EDGE_NORMS angle.
    The two associate the products differently: some twenty float64 roundings on entries below 2.5, 20 x 2.5 x 2.2e-16 ~ 1e-14."""
    rs = np.random.RandomState(3)
    d = np.concatenate([rs.normal(0, 0.1, (len(G.EDGE_NORMS), 6)).astype(np.float32), G.edge_row(len(G.EDGE_NORMS), rs)[:, 6:]], 1)
    T = MeshRef64.transform(torch.from_numpy(d)).numpy()
    for k in range(len(d)):
        assert np.abs(T[k] - MeshOracle.transform(d[k].astype(np.float64))).max() <= 1e-14, (k, G.EDGE_NORMS[k])
    S0 = MeshRef64.transform(torch.from_numpy(np.concatenate([d[:1, :6], np.full((1, 3), 5e-11, np.float32)], 1))).numpy()[0]
    assert np.array_equal(S0, S0.T)                                                # below 1e-10: the symmetric scale part alone


def test_seek_restatement_is_bit_exact(golden):
    g = golden["seek_track"]
    for name in g["cases"]:
        ts, seq, fps, want = g[f"{name}_ts"], g[f"{name}_seq"], float(g[f"{name}_fps"]), g[f"{name}_out"]
        assert MeshRef64.query_count(ts[-1], fps) == len(want) - 3, name           # the fixtures run 3 queries past model.py's range
        src, w = MeshRef64.seek_plan([ts], fps, query_counts=[len(want)])
        assert src.dtype == np.int64 and w.dtype == np.float32
        out = MeshRef64.blend(seq, src, w)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), want.view(np.uint32)), name
        out_t = MeshRef64.blend(torch.from_numpy(seq), src, w).numpy()             # the torch form the GPU test runs on the device
        assert np.array_equal(out_t.view(np.uint32), want.view(np.uint32)), name
    # all 13-column 60 fps clips in one plan: global row indices
    small = [str(n) for n in g["cases"] if g[f"{n}_seq"].shape[1] == 13 and float(g[f"{n}_fps"]) == 60.0]
    assert len(small) >= 2
    src, w = MeshRef64.seek_plan([g[f"{n}_ts"] for n in small], 60.0)
    out = MeshRef64.blend(np.concatenate([g[f"{n}_seq"] for n in small]), src, w)
    assert np.array_equal(out, np.concatenate([g[f"{n}_out"][:-3] for n in small]))


def test_own_residual_is_far_below_the_gpu_bounds(all_meshes, flame):
    """|(A^T A + reg) X - rhs| / |rhs| of the reference's own solve, on every mesh the GPU test uses: a condition on the meshes (all
    have constraints; without any the system would be conditioned by reg alone), at least 100x below the smallest GPU bound."""
    smallest = min(G.BOUNDS.values())
    res = {"flame": flame[0].residual(flame[1])}
    for name in ("corres", "grid16x8", "grid43x3"):
        m = all_meshes[name]
        assert len(m["cnsts"]) > 0
        res[name] = G.make_ref(m, "cpu").residual(G.draw_rows(6, m["n_src"], m["sigmas"], 11, G.SMALL_SPECIAL))
    print("\nresiduals", res, "smallest GPU bound", smallest)
    assert max(res.values()) * 100 <= smallest, res


def test_synthetic_meshes_have_the_wanted_sizes(all_meshes):
    free = {name: len(m["verts"]) - len(m["cnsts"]) for name, m in all_meshes.items()}
    assert free["flame"] == 1261 and free["grid16x8"] == 128 and free["grid43x3"] == 129
    g = all_meshes["corres"]
    assert g["n_src"] != len(g["faces"]) and (g["corr"]["corr_count"] == 0).any() and (g["corr"]["corr_count"] > 1).any()


def test_each_injected_failure_changes_the_reference(flame):
    ref, rows = flame
    good = ref.get_mesh(rows)
    v = int(ref.free[len(ref.free) // 2])
    bad = ref.get_mesh(rows, drop_incidence=(v, 1))
    diff = (bad - good).abs().amax(2)
    assert (diff[:4, v] > 1e-5).all() and diff[4].max() <= 1e-12, diff[:, v]        # frame 4 is the zero row: the term is zero
    bad = ref.get_mesh(rows, stale_frame=(1, 2))
    diff = (bad - good).abs().flatten(1).amax(1)
    assert diff[1] > 1e-4 and torch.equal(bad[[0, 2, 3, 4]], good[[0, 2, 3, 4]]) and torch.equal(bad[1], good[2])
    bad = ref.get_mesh(rows, skip_k_block=(4, 17))
    diff = (bad - good).abs().amax(2)
    tile = np.zeros(ref.n_verts, bool)
    tile[ref.free[512:640]] = True
    assert (diff[:4][:, tile].amax(1) > 1e-5).all() and diff[:, ~tile].max() == 0 and diff[4].max() <= 1e-12, diff[:, tile].amax(1)


# ------------------------------------------------------------------------------- host logic of tests/test_gpu_mesh_ref64.py
def test_launch_form_restatement_on_256_cus():
    assert G.sizes_for(256) == [1, 512, 513, 8789, 8790]
    assert [G.round_up(3 * n) for n in G.SMALL_SIZES] == [128, 128, 128, 256, 256, 384, 512]      # where ld changes, and 130
    assert [G.mesh_form(1280, n, 256) for n in (1, 512, 513, 8746, 8747, 8789, 8790)] == [G.SMALL, G.SMALL, G.TILE, G.TILE, G.FAT, G.FAT, G.TILE]
    assert {G.mesh_form(1280, n, 256) for n in G.sizes_for(256)} == {G.mesh_form(1280, n, 256) for n in range(1, G.FLAME_LIMIT)}
    assert G.gemm_form(1280, 26368, 1280, 256) == G.FAT and 26368 == 103 * 256 and 5 * 103 >= 512 > 5 * 102


def test_plans_have_exactly_the_wanted_queries_and_every_case():
    clips = G.flame_clips()
    assert [len(t) for t in clips] == list(G.CLIP_FRAMES) and all(8 <= len(t) <= 12 for t in clips)
    assert all(np.all(np.diff(t) > 0) and len(set(np.diff(t))) > 1 for t in clips)          # ascending, irregular
    for n in (512, 513, 8789, 8790, 300, 2048):
        ts, fps, counts = G.plan_for(n)
        src, w = MeshRef64.seek_plan(ts, fps, query_counts=counts)
        assert len(src) == n == sum(counts)
        assert min(G.plan_cases(ts, fps, counts).values()) > 0, (n, G.plan_cases(ts, fps, counts))
        copies = (src[:, 0] == src[:, 1])
        assert np.array_equal(w[copies], np.broadcast_to(np.float32([1, 0]), w[copies].shape))
        assert ((src[:, 0] == G.FLAME_ZERO_ROW) & copies).any() and ((src[:, 0] == G.FLAME_EDGE_ROW) & copies).any()
        assert src.min() == 0 and src.max() == sum(G.CLIP_FRAMES) - 1
