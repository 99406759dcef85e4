"""CPU checks of the PCA fit's contract (include/sdfa_pca.h): the float64 restatement tests/pca_ref64.py is what sklearn's PCA
computes (against sklearn where it imports, against tests/golden/pca_fit.npz everywhere); the selector restatement is the
reference's two flatten() expressions; the ABI of the header is bound and exported; every host-side refusal is made before
a launch (null device pointers are never touched); the library's float64 host algebra (cyclic Jacobi, Cholesky) agrees with
numpy on a 256 x 256 matrix with clustered eigenvalues."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pca_ref64 as R
from gen_golden_pca import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(96, 288), (257, 111), (300, 37)]


def _close(ref, mean, comps, var, ratio, tol):
    assert ref.k == len(comps)
    assert np.abs(ref.mean - mean).max() <= tol
    assert np.abs(ref.components - comps).max() <= tol
    assert np.abs(ref.variance / var - 1).max() <= tol
    assert np.abs(ref.ratio - ratio).max() <= tol


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_golden_sklearn(golden, name):
    g = golden["pca_fit"]
    x = g[name.rsplit("_", 1)[0] + ".x"]
    nc = float(g[name + ".n_components"])
    assert x.dtype == np.float32 and np.array_equal(x, R.tracks(*CASES[name][:6]))          # the generator is what made the fixture
    ref = R.pca(x, nc if nc < 1 else int(nc))
    _close(ref, g[name + ".mean"], g[name + ".components"], g[name + ".variance"], g[name + ".ratio"], 1e-12)


@pytest.mark.parametrize("F,D", SHAPES)
@pytest.mark.parametrize("nc", [0.97, 0.6, 5])
def test_restatement_matches_sklearn(F, D, nc):
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    x = R.tracks(F, D, 24, 0.8, 0.003, F + D)
    p = PCA(n_components=nc, svd_solver="full").fit(x.astype(np.float64))
    _close(R.pca(x, nc), p.mean_, p.components_, p.explained_variance_, p.explained_variance_ratio_, 1e-12)
    p32 = PCA(n_components=nc, svd_solver="full").fit(x.copy())                              # float32 in, as the reference fits it
    ref = R.pca(x, nc)
    assert p32.n_components_ == ref.k
    assert np.abs(p32.explained_variance_ / ref.variance - 1).max() <= 1e-4
    assert np.abs(np.abs(p32.components_ @ ref.components.T) - np.eye(ref.k)).max() <= 1e-3


def test_ratio_rule_is_searchsorted_right():
    full = R.pca_full(R.tracks(40, 30, 10, 0.7, 0.01, 3))
    for k in (1, 2, 5):
        assert R.choose_k(full, full.cumulative[k - 1]) == k + 1          # a ratio equal to a cumulative value takes one more
        mid, margin = R.midpoint_ratio(full, k)
        assert margin > 0 and R.choose_k(full, mid) == k
    assert R.choose_k(full, 7) == 7


def test_sign_rule_first_index_on_ties():
    x = np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    c = R.pca_full(x).components[0]
    assert abs(abs(c[0]) - abs(c[1])) < 1e-15 and c[np.argmax(np.abs(c))] > 0


def test_selector_is_the_reference_flatten():
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((4, 9 * 37)).astype(np.float32)
    for r, row in enumerate(rows):
        dg = np.reshape(row, (-1, 9))                                                          # preload.py:927-929
        assert np.array_equal(R.select(rows, (9, 0, 6))[r], dg[:, :6].flatten())
        assert np.array_equal(R.select(rows, (9, 6, 3))[r], dg[:, 6:].flatten())
    assert np.array_equal(R.select(rows, (1, 0, 1)), rows)
    assert np.array_equal(R.select_columns(18, (9, 6, 3)), [6, 7, 8, 15, 16, 17])


def test_pca_header_symbols_bound_and_exported():
    from sdfa_amd import pca, obj, jpeg, render, _lib
    hdr = open(os.path.join(ROOT, "include", "sdfa_pca.h")).read()
    assert re.search(r"#define SDFA_PCA_ABI_VERSION 1\b", hdr)
    for name, want in (("MAX_BLOCK", pca.MAX_BLOCK), ("OVERSAMPLE", pca.OVERSAMPLE), ("MAX_COMPONENTS", pca.MAX_COMPONENTS), ("SLAB", pca.SLAB), ("ZSLAB", pca.ZSLAB),
                       ("ENOTCONVERGED", pca.ENOTCONVERGED), ("EZEROVAR", pca.EZEROVAR), ("ERATIO", pca.ERATIO)):
        assert int(re.search(r"#define SDFA_PCA_%s\s+(-?\d+)" % name, hdr).group(1)) == want, name
    assert pca.MAX_COMPONENTS == pca.MAX_BLOCK - pca.OVERSAMPLE == 248
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    declared = set(re.findall(r"\b(sdfa_pca_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(pca.SYMBOLS), declared ^ set(pca.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.sdfa_pca_abi_version() == pca.ABI_VERSION == 1
    for other in (_lib, jpeg, render, obj):
        assert not declared & set(other.SYMBOLS), "pca symbols belong to their own header"
    assert _lib.lib.sdfa_abi_version() == _lib.ABI_VERSION == 5              # the core ABI did not move
    assert C.sizeof(pca.Info) == 56


def _fit_rc(rows, W, sel, nc, block=0, cap=256, n_chunks=None, p=None):
    """sdfa_pca_fit with device pointers that are null (or, with p, never to be dereferenced): only the host checks can answer"""
    from sdfa_amd import pca, _lib
    n = len(rows) if n_chunks is None else n_chunks
    nrows = (C.c_int64 * max(1, len(rows)))(*rows)
    ptrs = (C.c_void_p * max(1, len(rows)))(*([p] * len(rows)))
    info = pca.Info()
    g, o, t = sel
    rc = _lib.lib.sdfa_pca_fit(ptrs, nrows, n, W, g, o, t, float(nc), 0, block, 0.0, 0, p, p, cap, p, p, C.byref(info) if p else None, p, 0, None)
    return rc, _lib.lib.sdfa_last_error()


def test_fit_refusals_come_before_any_launch():
    from sdfa_amd import _lib
    E = _lib.EINVAL
    for p in (None, 1 << 12):
        assert _fit_rc([1], 90, (9, 0, 6), 0.97, p=p) == (E, b"pca_fit: 1 row, a fit needs at least 2")
        rc, msg = _fit_rc([5, 5], 91, (9, 0, 6), 0.97, p=p)
        assert rc == E and b"no multiple of the group" in msg
        rc, msg = _fit_rc([10], 90, (9, 5, 6), 0.97, p=p)
        assert rc == E and b"leaves its group" in msg
        rc, msg = _fit_rc([10], 90, (9, 0, 6), 10, p=p)                      # min(F - 1, D) = 9
        assert rc == E and b"at most min(F - 1, D) = 9" in msg
        rc, msg = _fit_rc([4], 90, (9, 6, 3), 4, p=p)                        # F - 1 = 3
        assert rc == E and b"min(F - 1, D) = 3" in msg
        rc, msg = _fit_rc([500], 900, (1, 0, 1), 249, p=p)
        assert rc == E and b"holds at most 248" in msg
        assert _fit_rc([500], 900, (1, 0, 1), 248, p=p)[0] == E             # accepted as k; refused next for the pointers / workspace
        for nc in (0.0, 1.5, -2, float("nan")):
            rc, msg = _fit_rc([10], 90, (9, 0, 6), nc, p=p)
            assert rc == E and b"neither a ratio" in msg, nc
        for block in (16, 48, 288, -32):
            rc, msg = _fit_rc([500], 900, (1, 0, 1), 0.9, block=block, p=p)
            assert rc == E and b"no multiple of 32" in msg
        rc, msg = _fit_rc([500], 900, (1, 0, 1), 60, block=64, p=p)
        assert rc == E and b"oversampling" in msg
        rc, msg = _fit_rc([], 90, (9, 0, 6), 0.97, n_chunks=0, p=p)
        assert rc == E and b"no chunks" in msg
    rc, msg = _fit_rc([10], 90, (9, 0, 6), 0.97)
    assert rc == E and b"null pointer" in msg
    rc, msg = _fit_rc([10], 90, (9, 0, 6), 0.97, p=1 << 12)
    assert rc == E and b"workspace of 0 bytes" in msg


def test_workspace_and_stateless_calls_refuse_bad_shapes():
    from sdfa_amd import _lib, pca
    lib = _lib.lib
    rows = (C.c_int64 * 2)(257, 100)
    small = lib.sdfa_pca_workspace_bytes(rows, 2, 90, 9, 0, 6)
    assert small > 0 and small % 256 == 0
    assert lib.sdfa_pca_workspace_bytes(rows, 2, 180, 9, 0, 6) > small
    assert lib.sdfa_pca_workspace_bytes(rows, 2, 91, 9, 0, 6) == _lib.EINVAL
    assert lib.sdfa_pca_workspace_bytes(rows, 0, 90, 9, 0, 6) == _lib.EINVAL
    cap = 65535 * pca.SLAB                                                   # column slabs are a grid's y dimension
    assert lib.sdfa_pca_workspace_bytes(rows, 2, cap, 1, 0, 1) > 0
    assert lib.sdfa_pca_workspace_bytes(rows, 2, cap + 1, 1, 0, 1) == _lib.EINVAL
    assert b"selected columns, at most 67107840" in lib.sdfa_last_error()
    assert lib.sdfa_pca_workspace_bytes(rows, 2, 9 * (cap // 6), 9, 0, 6) > 0                    # D, not W, is what is capped
    assert _fit_rc([10], cap + 1, (1, 0, 1), 0.97, p=1 << 12)[0] == _lib.EINVAL
    assert lib.sdfa_pca_transform(None, 0, 90, 9, 0, 6, None, None, 4, None, None) == 0          # no rows: a no-op
    assert lib.sdfa_pca_transform(None, 3, 90, 9, 0, 6, None, None, 4, None, None) == _lib.EINVAL
    assert b"null pointer" in lib.sdfa_last_error()
    p = 1 << 12
    assert lib.sdfa_pca_transform(p, 3, 90, 9, 0, 6, p, p, 257, p, None) == _lib.EINVAL
    assert lib.sdfa_pca_inverse_transform(p, 3, 0, p, p, 90, 9, 0, 6, p, None) == _lib.EINVAL
    assert lib.sdfa_pca_inverse_transform(p, 3, 4, p, p, 90, 9, 7, 3, p, None) == _lib.EINVAL
    assert lib.sdfa_pca_inverse_transform(None, 3, 4, None, None, 90, 9, 6, 3, None, None) == _lib.EINVAL


def test_host_algebra_against_numpy_on_clustered_spectrum():
    from sdfa_amd import pca, _lib
    rng = np.random.default_rng(5)
    n = 256
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.concatenate([1 + 1e-9 * np.arange(64), 0.5 + 1e-7 * np.arange(64), np.geomspace(0.1, 1e-6, 128)])      # two tight clusters
    a = (q * w) @ q.T
    a = 0.5 * (a + a.T)
    ev, vec, rinv = pca.host_algebra(a)
    want = np.linalg.eigh(a)[0][::-1]
    assert np.all(np.diff(ev) <= 0)
    assert np.abs(ev - want).max() <= 1e-12 * want[0]
    assert np.abs(vec.T @ vec - np.eye(n)).max() <= 1e-12
    assert np.abs(a @ vec - vec * ev).max() <= 1e-12 * want[0]              # eigenvectors of a cluster are not unique; the pairs are exact
    assert np.abs(np.tril(rinv, -1)).max() == 0.0                           # R^-1 is upper triangular
    r = np.linalg.cholesky(a).T
    assert np.abs(rinv @ r - np.eye(n)).max() <= 1e-9                       # cond(a) = 1e6
    assert np.abs(rinv.T @ a @ rinv - np.eye(n)).max() <= 1e-9
    b = a.copy()
    b[3, 3] = -1.0
    with pytest.raises(_lib.SdfaError, match="not positive definite"):
        pca.host_algebra(b)


def test_frame_file_patterns(tmp_path):
    from speech_anime.datasets import pca as P
    for name in ("000010_dgrad.npy", "000002_dgrad.npy", "7.npy", "-3.npy", "notes.npy", "000001.obj", "12_offsets.npy"):
        (tmp_path / name).write_bytes(b"")
    got = [os.path.basename(p) for p in P.find_frames(str(tmp_path))]
    # the reference's order: paths sorted as strings, so that its `i % step` picks the same frames
    assert got == ["-3.npy", "000002_dgrad.npy", "000010_dgrad.npy", "12_offsets.npy", "7.npy"]
    assert [os.path.basename(p) for p in P.find_frames(str(tmp_path), 2)] == ["-3.npy", "000010_dgrad.npy", "7.npy"]
    (tmp_path / "sub").mkdir()                                              # and its walk of the tree
    (tmp_path / "sub" / "000001.npy").write_bytes(b"")
    got = [os.path.relpath(p, tmp_path) for p in P.find_frames(str(tmp_path))]
    assert got == ["-3.npy", "000002_dgrad.npy", "000010_dgrad.npy", "12_offsets.npy", "7.npy", os.path.join("sub", "000001.npy")]
