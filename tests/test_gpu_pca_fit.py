"""GPU checks of the PCA fit (sdfa_amd.pca, include/sdfa_pca.h) against the float64 restatement of sklearn's PCA,
tests/pca_ref64.py -- the reference, never the code under test.

Data are dgrad-like: base 1 + 0.01 * ((U s) V^T sqrt(F) + noise N), s_i = decay^i.  A ratio is always the midpoint between two
consecutive cumulative ratios of the reference (both margins asserted >= 5e-4 first), so the count cannot hinge on rounding;
the default 0.97 is exercised where its margins are >= 2e-3.

Bounds.  Each is 4 x the largest value measured on an MI355X over the cases of this file, rounded up to one digit (the
accumulation order changes with tile and chunk shape); `_figures` prints every figure before it asserts.  Measured maxima:
see MEASURED below; DESIGN.md section 11 repeats them.  transform / inverse_transform are held to two bounds each: the
per-element rounding bound of a float32 dot product of that length, written next to its assertion, and a measured cap."""
import os

import numpy as np
import pytest
import torch

import pca_ref64 as R

pytestmark = pytest.mark.gpu

SCALE, ROTAT, PLAIN = (9, 0, 6), (9, 6, 3), (1, 0, 1)

# quantity -> (largest value measured over this file's cases, asserted bound = 4 x that, rounded up to one digit)
MEASURED = {
    "mean": (5.96e-8, 3e-7),          # max |mean - ref|, data near 1: half an ulp of float32 at 1
    "eig": (1.88e-6, 8e-6),           # max |lambda_i / ref - 1|                          (F = 513, D = 15)
    "ratio": (3.63e-7, 2e-6),         # max |ratio_i - ref|                               (F = 3, D = 1161)
    "comp": (4.35e-6, 2e-5),          # max |component entry - ref| after the sign rule, relative gaps >= 0.03   (F = 96, D = 2304, seed 1, default 0.97)
    "orth": (1.08e-6, 5e-6),          # max |C C^T - I|                                   (slowly decaying spectrum)
    "proj": (9.58e-7, 4e-6),          # max |C^T C - ref|                                 (F = 513, D = 15)
    "res": (2.03e-6, 3e-6),           # the fit's own stopping test: <= the default tol by construction, not 4 x
    "captured": (4.86e-8, 2e-7),      # |sum of the kept ratios - ref|, slowly decaying spectrum (0.971778978 against 0.971779026)
    "span": (3.5e-6, 2e-5),           # full width: norm of a component's part outside the head basis (scale 2.6e-6, rotat 3.5e-6)
    "transform": (9.8e-9, 4e-8),      # max |coefficient - float64|, F = 257, W = 333, k = 8, all three selectors
    "inverse": (6.0e-8, 3e-7),        # max |row entry - float64|, data near 1: half an ulp of float32 at 1
    "roundtrip": (1.2e-7, 5e-7),      # max |row entry - row| over rows in the span, there and back
}
BOUND = {k: v[1] for k, v in MEASURED.items()}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _figures(name, fit, ref, components=True, projector=True):
    """Prints and returns the figures of one fit against its reference; k must agree.  The projector is D x D: not at full width."""
    assert fit.k == ref.k, (name, fit.k, ref.k)
    c = fit.components.cpu().numpy().astype(np.float64)
    lam = fit.explained_variance.cpu().numpy().astype(np.float64)
    fig = {
        "mean": np.abs(fit.means.cpu().numpy() - ref.mean).max(),
        "eig": np.abs(lam / ref.variance - 1).max(),
        "ratio": np.abs(fit.explained_variance_ratio.cpu().numpy() - ref.ratio).max(),
        "orth": np.abs(c @ c.T - np.eye(fit.k)).max(),
        "res": fit.max_residual,
    }
    if projector:
        fig["proj"] = np.abs(c.T @ c - ref.components.T @ ref.components).max()
    if components:
        fig["comp"] = np.abs(c - ref.components).max()
    print("PCAFIG %s k=%d block=%d sweeps=%d " % (name, fit.k, fit.block, fit.sweeps) + " ".join("%s=%.3e" % kv for kv in sorted(fig.items())))
    return fig


def _check(name, fit, ref, components=True, projector=True):
    fig = _figures(name, fit, ref, components, projector)
    for q, v in fig.items():
        assert v <= BOUND[q], (name, q, v, BOUND[q])
    return fig


def _midpoint(full, k, least=5e-4):
    ratio, margin = R.midpoint_ratio(full, k)
    assert margin >= least, (k, margin)
    return ratio


def _gaps_ok(full, k, least=0.03):
    ev = np.append(full.eigenvalues, 0.0)
    gaps = (ev[:k] - ev[1:k + 1]) / ev[:k]
    assert gaps.min() >= least, gaps.min()


EDGES = [  # F, triangles n (W = 9 n), selector: D from 3 to 1161, F < D, F > D and F - 1 below the block
    (2, 1, ROTAT), (2, 37, SCALE), (3, 5, ROTAT), (3, 129, PLAIN), (33, 1, SCALE), (33, 37, PLAIN), (255, 5, SCALE),
    (255, 128, ROTAT), (256, 37, SCALE), (257, 129, SCALE), (257, 1, PLAIN), (513, 128, PLAIN), (513, 5, ROTAT),
]


@pytest.mark.parametrize("F,n,sel", EDGES)
def test_tile_edges(F, n, sel):
    from sdfa_amd import pca
    x = R.tracks(F, 9 * n, 24, 0.8, 0.003, 100 + F + n)
    xs = R.select(x, sel)
    full = R.pca_full(xs)
    k = min(6, F - 1, xs.shape[1])
    _gaps_ok(full, k)
    ratio = _midpoint(full, k)
    ref = R.pca(xs, ratio)
    assert ref.k == k
    _check(f"edge-F{F}-W{9 * n}-{sel}", pca.fit(_dev(x), ratio, sel), ref)
    _check(f"edge-int-F{F}-W{9 * n}-{sel}", pca.fit(_dev(x), k, sel), R.pca(xs, k))


# rank 24, decay 0.8, noise 0.003.  Seed 1 at F = 96 / D = 2304: 0.97 lies 0.0048 / 0.0055 from its neighbours.  At F = 33 / D = 30 seed 1
# leaves 0.0136 / 0.0016 with this generator, short of the 2e-3 asked of a default-ratio case, so seed 3 stands in there
# (0.0130 / 0.0023); seed 3 at F = 96 (0.0046 / 0.0055) is kept as a third case.
@pytest.mark.parametrize("F,D,seed", [(33, 30, 3), (96, 2304, 1), (96, 2304, 3)])
def test_default_ratio(F, D, seed):
    from sdfa_amd import pca
    x = R.tracks(F, D, 24, 0.8, 0.003, seed)
    full = R.pca_full(x)
    k = R.choose_k(full, 0.97)
    assert 0.97 - (full.cumulative[k - 2] if k > 1 else 0.0) >= 2e-3 and full.cumulative[k - 1] - 0.97 >= 2e-3
    _gaps_ok(full, k)
    _check(f"default-F{F}-D{D}-s{seed}", pca.fit(_dev(x)), R.pca(x, 0.97))
    _check(f"default-offsets-F{F}-D{D}-s{seed}", pca.fit_offsets(_dev(x)), R.pca(x, 0.97))


def test_slowly_decaying_spectrum():
    from sdfa_amd import pca
    x = R.tracks(600, 2160, 200, 0.975, 0.0005, 7)
    xs = R.select(x, SCALE)                                # D = 1440
    full = R.pca_full(xs)
    k = 70
    ratio = _midpoint(full, k)
    ref = R.pca(xs, ratio)
    fit = pca.fit(_dev(x), ratio, SCALE)
    fig = _figures("slow", fit, ref, components=False)     # single components are ill-conditioned here (relative gaps of 0.011)
    for q in ("mean", "eig", "ratio", "orth", "proj", "res"):
        assert fig[q] <= BOUND[q], (q, fig[q])
    captured = float(fit.explained_variance_ratio.double().sum())
    print("PCAFIG slow captured=%.9f ref=%.9f diff=%.3e" % (captured, ref.ratio.sum(), abs(captured - ref.ratio.sum())))
    assert abs(captured - ref.ratio.sum()) <= BOUND["captured"]


def test_constant_columns():
    """74 % of the columns identically zero, as the reference's masked non-face triangles make them."""
    from sdfa_amd import pca
    x = R.tracks(257, 9 * 64, 24, 0.8, 0.003, 9)
    dead = np.random.default_rng(9).random(x.shape[1]) < 0.74
    x[:, dead] = 0.0
    xs, dead_s = R.select(x, SCALE), dead[R.select_columns(x.shape[1], SCALE)]
    assert 0.6 < dead_s.mean() < 0.9
    full = R.pca_full(xs)
    _gaps_ok(full, 8)
    ratio = _midpoint(full, 8)
    fit = pca.fit(_dev(x), ratio, SCALE)
    _check("constant", fit, R.pca(xs, ratio))
    assert not fit.means.cpu().numpy()[dead_s].any()
    assert not fit.components.cpu().numpy()[:, dead_s].any()


def _same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("means", "components", "explained_variance", "explained_variance_ratio")) and a.k == b.k


def test_chunking_and_determinism():
    from sdfa_amd import pca
    x = R.tracks(257, 9 * 37, 24, 0.8, 0.003, 5)
    xs = R.select(x, SCALE)
    full = R.pca_full(xs)
    _gaps_ok(full, 8)
    ratio = _midpoint(full, 8)
    ref = R.pca(xs, ratio)
    d = _dev(x)
    whole = pca.fit(d, ratio, SCALE)
    parts = [d[:1], d[1:129], d[129:]]
    split = pca.fit(parts, ratio, SCALE)
    _check("chunk-whole", whole, ref)
    _check("chunk-split", split, ref)                                     # another chunking: within the accuracy bound
    assert _same(split, pca.fit(parts, ratio, SCALE))                     # the same chunking: the same bits
    assert _same(whole, pca.fit(d.clone(), ratio, SCALE))
    c = _dev(xs)                                                          # the selector only addresses
    assert _same(whole, pca.fit(c, ratio, PLAIN))
    assert _same(split, pca.fit([c[:1], c[1:129], c[129:]], ratio, PLAIN))


def test_integer_k_and_the_cap():
    from sdfa_amd import pca
    x = R.tracks(257, 9 * 37, 24, 0.8, 0.003, 5)
    _gaps_ok(R.pca_full(x), 5)
    _check("int5", pca.fit(_dev(x), 5), R.pca(x, 5))
    # the cap: 248 components of 250 rows (the block is then the whole row space, 249 columns)
    x = R.tracks(250, 300, 250, 0.99, 0.0005, 6)
    ref = R.pca(x, pca.MAX_COMPONENTS)
    fit = pca.fit(_dev(x), pca.MAX_COMPONENTS)
    fig = _figures("cap248", fit, ref, components=False)                  # gaps of 0.02: single components are not compared
    for q in ("mean", "ratio", "orth", "res"):                            # (its projector, 1.9e-5 measured, is as ill-defined as its components)
        assert fig[q] <= BOUND[q], (q, fig[q])
    lam = fit.explained_variance.cpu().numpy().astype(np.float64)
    assert np.abs(lam - ref.variance).max() <= BOUND["eig"] * ref.variance[0]      # the stopping test is relative to lambda_1
    with pytest.raises(Exception, match="holds at most 248"):
        pca.fit(_dev(R.tracks(300, 300, 24, 0.8, 0.003, 6)), 249)


def test_exact_rank_below_the_block():
    """Noise-free rows of rank 10 at block 32 < min(F - 1, D): the block's 22 surplus columns are rounding noise, which the
    orthonormalisation has to keep independent (the header names the limit: a pivot lost there ends the fit with "lost rank",
    never with a result).  These rows fit, and as accurately as any."""
    from sdfa_amd import pca
    x = R.tracks(100, 207, 10, 0.8, 0.0, 12)
    full = R.pca_full(x)
    assert full.eigenvalues[10] <= 1e-9 * full.eigenvalues[0]                         # rank 10, exactly but for float32 rounding of the rows
    _gaps_ok(full, 5)
    fit = pca.fit(_dev(x), 5)
    assert fit.block == 32
    _check("rank10", fit, R.pca(x, 5))


def test_failing_fits_raise():
    from sdfa_amd import pca
    x = R.tracks(300, 400, 24, 0.8, 0.003, 8)              # 24 directions and a flat floor of 275: 0.99999 needs more than 248
    with pytest.raises(pca.PcaNotConverged, match="not reached within 248"):
        pca.fit(_dev(x), 0.99999)
    with pytest.raises(pca.PcaNotConverged, match="no variance"):
        pca.fit(_dev(np.full((40, 90), 1.25, np.float32)), 0.97, SCALE)
    with pytest.raises(pca.PcaNotConverged, match="not converged after 1 sweeps"):
        pca.fit(_dev(R.tracks(257, 333, 24, 0.8, 0.003, 5)), 8, max_sweeps=1, tol=1e-12)


def test_transform_and_inverse_transform():
    from sdfa_amd import pca
    u = 2.0 ** -24
    x = R.tracks(257, 9 * 37, 24, 0.8, 0.003, 5)
    d = _dev(x)
    for sel in (SCALE, ROTAT, PLAIN):
        xs = R.select(x, sel).astype(np.float64)
        fit = pca.fit(d, 8, sel)
        mean, comp = fit.means.cpu().numpy().astype(np.float64), fit.components.cpu().numpy().astype(np.float64)
        D, k = xs.shape[1], fit.k
        xc = (R.select(x, sel) - fit.means.cpu().numpy()).astype(np.float64)          # the float32 difference the kernel forms
        coef = fit.transform(d).cpu().numpy()
        want = xc @ comp.T
        # a float32 dot product of length D: |error| <= D u sum |a||b| <= D u |xc_r| |c_i|, plus the rounding of the result
        bound = D * u * np.linalg.norm(xc, axis=1)[:, None] * np.linalg.norm(comp, axis=1)[None, :] + u * np.abs(want)
        err = np.abs(coef - want)
        print("PCAFIG transform-%s err=%.3e bound=%.3e" % (sel, err.max(), bound.min()))
        assert (err <= bound).all() and err.max() <= BOUND["transform"]
        out = torch.full((257, x.shape[1]), 7.0, device="cuda")
        back = fit.inverse_transform(_dev(coef), out)
        assert back.data_ptr() == out.data_ptr()
        back = back.cpu().numpy()
        cols = R.select_columns(x.shape[1], sel)
        other = np.setdiff1d(np.arange(x.shape[1]), cols)
        assert (back[:, other] == 7.0).all()                                            # only the selected columns are written
        want = mean + coef.astype(np.float64) @ comp
        bound = (k + 1) * u * (np.abs(mean) + np.abs(coef.astype(np.float64)) @ np.abs(comp)) + u * np.abs(want)
        err = np.abs(back[:, cols] - want)
        print("PCAFIG inverse-%s err=%.3e bound=%.3e" % (sel, err.max(), bound.min()))
        assert (err <= bound).all() and err.max() <= BOUND["inverse"]
        # rows that lie in the span come back: mean + c0 C, rounded to float32 once
        c0 = np.random.default_rng(3).standard_normal((50, k)) * 0.05
        rows = np.zeros((50, x.shape[1]), np.float32)
        rows[:, cols] = (mean + c0 @ comp).astype(np.float32)
        trip = fit.inverse_transform(fit.transform(_dev(rows))).cpu().numpy()
        # coefficient error: the transform's dot-product bound, the rounding of the rows (u |row| per entry, sqrt(D) of them against a
        # unit vector) and the basis' distance from orthonormal; k of them enter an entry, each times a component entry; then the
        # inverse's own rounding
        n0 = np.linalg.norm(c0, axis=1)
        cerr = D * u * n0 * 1.01 + np.sqrt(D) * u * np.abs(rows).max() + BOUND["orth"] * np.sqrt(k) * n0
        bound = (k * cerr * np.abs(comp).max())[:, None] + (k + 3) * u * (np.abs(rows[:, cols]) + np.abs(c0) @ np.abs(comp))
        err = np.abs(trip[:, cols] - rows[:, cols])
        print("PCAFIG roundtrip-%s err=%.3e bound=%.3e" % (sel, err.max(), bound.min()))
        assert (err <= bound).all() and err.max() <= BOUND["roundtrip"]
        assert not trip[:, other].any()
        assert fit.compT.shape == (D, k) and torch.equal(fit.compT, fit.components.t())


def test_full_width_synthetic_head(synth_sd):
    """W = 89,784, F = 192: rows in the span of the synthetic head's bases, built on the device."""
    from sdfa_amd import pca
    sd = synth_sd["dgrad"]
    F, T = 192, 9976
    g = torch.Generator(device="cpu").manual_seed(11)
    rows = torch.empty(F, T, 9, device="cuda")
    heads = {}
    for name, per, lo, nc in (("scale", 6, 0, 85), ("rotat", 3, 6, 180)):
        compT = next(v for k, v in sd.items() if k.endswith(f"_{name}_pca.compT"))
        means = next(v for k, v in sd.items() if k.endswith(f"_{name}_pca.means"))
        assert compT.shape == (T * per, nc)
        coef = torch.randn(F, nc, generator=g) * (0.85 ** torch.arange(nc, dtype=torch.float32)) * 3.0
        part = _dev(means) + coef.cuda() @ _dev(compT).t()                              # torch for the product only
        rows[:, :, lo:lo + per] = part.reshape(F, T, per)
        heads[name] = np.linalg.qr(compT.astype(np.float64))[0]                         # the head basis, orthonormalised in float64
    rows = rows.reshape(F, T * 9)
    host = rows.cpu().numpy()
    for name, sel, nc in (("scale", SCALE, 85), ("rotat", ROTAT, 180)):
        xs = R.select(host, sel)
        full = R.pca_full(xs)
        k = 12
        _gaps_ok(full, k, 0.03)
        ratio = _midpoint(full, k)
        ref = R.pca(xs, ratio)
        fit = pca.fit(rows, ratio, sel)
        assert fit.k == ref.k == k <= nc
        _check(f"fullwidth-{name}", fit, ref, projector=False)
        c = fit.components.cpu().numpy().astype(np.float64)
        B = heads[name]
        out_of_span = np.linalg.norm(c - (c @ B) @ B.T, axis=1)
        print("PCAFIG fullwidth-%s out_of_span=%.3e" % (name, out_of_span.max()))
        assert out_of_span.max() <= BOUND["span"]
    tensors = fit.head_tensors("_output_module._rotat")
    assert sorted(tensors) == ["_output_module._rotat_pca.compT", "_output_module._rotat_pca.means"]
    assert tensors["_output_module._rotat_pca.compT"].shape == (T * 3, k)


def test_refit_basis_loads_into_the_head(synth_sd):
    """An integer-k refit has the shapes the existing head takes: the engine runs with it."""
    from sdfa_amd import pca
    from sdfa_amd.engine import Engine
    sd = dict(synth_sd["offsets"])
    key = next(k for k in sd if k.endswith("_pca.compT"))
    prefix = key[:-len("_pca.compT")]
    D, nc = sd[key].shape
    rng = np.random.default_rng(2)
    rows = (sd[prefix + "_pca.means"] + (rng.standard_normal((96, nc)) * 0.9 ** np.arange(nc)).astype(np.float32) @ sd[key].T
            + 1e-4 * rng.standard_normal((96, D))).astype(np.float32)
    fit = pca.fit_offsets(_dev(rows), nc)
    for name, t in fit.head_tensors(prefix).items():
        assert name in sd and tuple(t.shape) == sd[name].shape
        sd[name] = t.cpu().numpy()
    eng = Engine(sd, device="cuda:0", max_frames=64)
    assert eng is not None


def test_pca_dgrad_surface(tmp_path, capsys):
    from speech_anime.datasets import pca as P
    x = R.tracks(40, 9 * 12, 10, 0.7, 0.003, 1)
    clip = tmp_path / "clip0"
    clip.mkdir()
    for i, row in enumerate(x):
        np.save(clip / f"{i:06d}_dgrad.npy", row.reshape(-1, 9))
    (clip / "audio.wav").write_bytes(b"")
    out = tmp_path / "out"
    scale, rotat = P.pca_dgrad([str(clip)], str(out), step=2)
    names = sorted(os.listdir(out / "pca"))
    assert names == ["rotat_compT.npy", "rotat_means.npy", "scale_compT.npy", "scale_means.npy"]
    for name, fit, per, sel in (("scale", scale, 6, SCALE), ("rotat", rotat, 3, ROTAT)):
        compT, means = np.load(out / "pca" / f"{name}_compT.npy"), np.load(out / "pca" / f"{name}_means.npy")
        assert compT.dtype == means.dtype == np.float32
        assert compT.shape == (12 * per, fit.k) and means.shape == (12 * per,)
        full = R.pca_full(R.select(x[::2], sel))
        ref = R.pca(R.select(x[::2], sel), 0.97)
        assert min(0.97 - full.cumulative[ref.k - 2], full.cumulative[ref.k - 1] - 0.97) >= 2e-3      # 0.97 is no close call here
        assert fit.k == ref.k
        assert np.abs(means - ref.mean).max() <= BOUND["mean"]
    stamp = os.path.getmtime(out / "pca" / "scale_compT.npy")
    assert P.pca_dgrad([str(clip)], str(out), step=2) is None                           # a second call skips
    assert "already calculated" in capsys.readouterr().err
    assert os.path.getmtime(out / "pca" / "scale_compT.npy") == stamp
    small = P.CHUNK_BYTES
    try:                                                                                # arrays are cut into chunks like files are
        P.CHUNK_BYTES = 7 * 108 * 4
        chunks = P.load_chunks(x, step=3)
        assert [c.shape[0] for c in chunks] == [7, 7] and all(c.is_cuda and c.is_contiguous() for c in chunks)
        assert np.array_equal(torch.cat(chunks).cpu().numpy(), x[::3])
        chunks = P.load_chunks([x[:20], _dev(x[20:])], step=1)
        assert [c.shape[0] for c in chunks] == [7, 7, 6, 20] and np.array_equal(torch.cat(chunks).cpu().numpy(), x)
    finally:
        P.CHUNK_BYTES = small
    off = P.pca_offsets(x, str(tmp_path / "off"))
    assert np.load(tmp_path / "off" / "pca" / "compT.npy").shape == (108, off.k)
