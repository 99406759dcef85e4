"""float64 numpy restatement of sklearn.decomposition.PCA as the reference uses it (preload.py pca_offsets / pca_dgrad), and of
the column selector of include/sdfa_pca.h.  This is the reference of the PCA tests, never the code under test.

    mean_                      x.mean(axis=0)
    U, S, Vt                   numpy.linalg.svd(x - mean_, full_matrices=False)
    sign rule (svd_flip)       each row of Vt is signed so that its entry of largest magnitude is positive (first index on ties)
    explained_variance_        S^2 / (F - 1)
    explained_variance_ratio_  explained_variance_ / explained_variance_.sum()
    n_components in (0, 1)     k = searchsorted(cumsum(ratio), n_components, side="right") + 1
    n_components integer       k
"""
import numpy as np


def select_columns(W, select):
    """Row columns of the selected columns d = 0 .. D - 1: (d // t) * g + o + d % t."""
    g, o, t = select
    assert W % g == 0 and 0 <= o and t >= 1 and o + t <= g, (W, select)
    d = np.arange(W // g * t)
    return (d // t) * g + o + d % t


def select(rows, sel):
    rows = np.asarray(rows)
    return rows[:, select_columns(rows.shape[1], sel)]


class Ref:
    pass


def pca_full(x):
    """Every component of x (F x D): the float64 decomposition the kept ones are cut from."""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    r = Ref()
    r.mean = x.mean(axis=0)
    xc = x - r.mean
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    idx = np.argmax(np.abs(vt), axis=1)
    signs = np.sign(vt[np.arange(vt.shape[0]), idx])
    signs[signs == 0] = 1.0
    r.components = vt * signs[:, None]
    r.eigenvalues = s * s                                  # of Xc^T Xc
    r.variance = r.eigenvalues / (F - 1)
    r.total_variance = r.variance.sum()
    r.ratio = r.variance / r.total_variance
    r.cumulative = np.cumsum(r.ratio)
    return r


def choose_k(full, n_components):
    if 0 < n_components < 1:
        return int(np.searchsorted(full.cumulative, n_components, side="right") + 1)
    return int(n_components)


def pca(x, n_components):
    """The fitted PCA: mean, components [k][D], variance [k], ratio [k], k."""
    full = pca_full(x)
    k = choose_k(full, n_components)
    r = Ref()
    r.k = k
    r.mean = full.mean
    r.components = full.components[:k]
    r.variance = full.variance[:k]
    r.ratio = full.ratio[:k]
    r.eigenvalues = full.eigenvalues[:k]
    r.full = full
    return r


def midpoint_ratio(full, k):
    """A ratio that selects exactly k components, half way between the cumulative ratios of k - 1 and k components, and its
    distance to either."""
    lo = full.cumulative[k - 2] if k >= 2 else 0.0
    hi = full.cumulative[k - 1]
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def tracks(F, D, rank, decay, noise, seed, base=1.0, amp=0.01):
    """dgrad-like rows: base + amp * ((U s) V^T sqrt(F) + noise * N) with orthonormal seeded U (F x rank), V (D x rank),
    s_i = decay^i; float32."""
    rng = np.random.default_rng(seed)
    rank = min(rank, F, D)
    u, _ = np.linalg.qr(rng.standard_normal((F, rank)))
    v, _ = np.linalg.qr(rng.standard_normal((D, rank)))
    s = decay ** np.arange(rank)
    x = (u * s) @ v.T * np.sqrt(F) + noise * rng.standard_normal((F, D))
    return (base + amp * x).astype(np.float32)
