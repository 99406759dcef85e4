"""Float64 numpy restatement of deformation.get_deform_grad (deformation/cpp/src/pybind.cpp:78-99,
deform_triangle_impl.hpp:143-213,447-470, rotation/utils_rotation.cpp log) -- the arithmetic csrc/dgrad.hip runs, vectorised over
triangles: the frames and T = B A^-1, Eigen's two-sided Jacobi SVD of a square 3x3 (JacobiSVD.h, RealSvd2x2.h, Jacobi.h), the
polar part and the rotation log with every branch.  Pinned to the reference's own output in tests/golden/deform_grad.npz."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
DBL_EPS = np.finfo(np.float64).eps
LOG_TOL = 1.0e-6
MAX_SWEEPS = 64


def _edge3(e1, e2, eps):
    e3 = np.cross(e1, e2)
    len1 = np.sqrt((e1 * e1).sum(-1))
    len2 = np.sqrt((e2 * e2).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        abs_cos = np.abs((e1 * e2).sum(-1) / (len1 * len2))
        good = ~(abs_cos > 1.0 - eps)              # NaN (a zero-length edge) is not degenerate, as in the reference
        n = np.maximum(np.power((e3 * e3).sum(-1), 0.25), eps)
        e3 = e3 / n[:, None]
    return e3, good


def _inverse(A):
    """Eigen compute_inverse_size3_helper: cofactors, determinant from column 0."""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return A[:, i1, j1] * A[:, i2, j2] - A[:, i1, j2] * A[:, i2, j1]
    C = np.stack([np.stack([cof(i, j) for j in range(3)], -1) for i in range(3)], 1)      # C[:, i, j] = cofactor(i, j)
    with np.errstate(divide="ignore", invalid="ignore"):
        invdet = 1.0 / (C[:, 0, 0] * A[:, 0, 0] + C[:, 1, 0] * A[:, 1, 0] + C[:, 2, 0] * A[:, 2, 0])
    return np.transpose(C, (0, 2, 1)) * invdet[:, None, None]


def _rot_rows(M, p, q, c, s, on):
    x, y = M[:, p, :].copy(), M[:, q, :].copy()
    M[:, p, :] = np.where(on[:, None], c[:, None] * x + s[:, None] * y, x)
    M[:, q, :] = np.where(on[:, None], -s[:, None] * x + c[:, None] * y, y)


def _rot_cols(M, p, q, c, s, on):
    x, y = M[:, :, p].copy(), M[:, :, q].copy()
    M[:, :, p] = np.where(on[:, None], c[:, None] * x + s[:, None] * y, x)
    M[:, :, q] = np.where(on[:, None], -s[:, None] * x + c[:, None] * y, y)


def jacobi_svd(T):
    """Eigen::JacobiSVD<MatrixXd>(T, ComputeThinU | ComputeThinV) for a batch of 3x3: (U, singular values descending, V)."""
    n = T.shape[0]
    scale = np.abs(T).reshape(n, 9).max(1)
    scale = np.where(scale == 0.0, 1.0, scale)
    W = T / scale[:, None, None]
    U = np.tile(np.eye(3), (n, 1, 1))
    V = U.copy()
    max_diag = np.abs(np.diagonal(W, axis1=1, axis2=2)).max(1)
    alive = np.ones(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(MAX_SWEEPS):
            any_rot = np.zeros(n, bool)
            for p, q in ((1, 0), (2, 0), (2, 1)):
                thr = np.maximum(DBL_MIN, 2.0 * DBL_EPS * max_diag)
                on = alive & ((np.abs(W[:, p, q]) > thr) | (np.abs(W[:, q, p]) > thr))
                any_rot |= on
                m00, m01, m10, m11 = W[:, p, p], W[:, p, q], W[:, q, p], W[:, q, q]
                t, d = m00 + m11, m10 - m01
                small = np.abs(d) < DBL_MIN
                u = t / d
                tmp = np.sqrt(1.0 + u * u)
                s1 = np.where(small, 0.0, 1.0 / tmp)
                c1 = np.where(small, 1.0, u / tmp)
                n00, n10 = c1 * m00 + s1 * m10, -s1 * m00 + c1 * m10
                n01, n11 = c1 * m01 + s1 * m11, -s1 * m01 + c1 * m11
                deno = 2.0 * np.abs(n01)
                nz = ~(deno < DBL_MIN)
                tau = (n00 - n11) / deno
                w = np.sqrt(tau * tau + 1.0)
                tt = np.where(tau > 0.0, 1.0 / (tau + w), 1.0 / (tau - w))
                sign_t = np.where(tt > 0.0, 1.0, -1.0)
                nn = 1.0 / np.sqrt(tt * tt + 1.0)
                sr = np.where(nz, -sign_t * (n01 / np.abs(n01)) * np.abs(tt) * nn, 0.0)
                cr = np.where(nz, nn, 1.0)
                cl = c1 * cr - s1 * (-sr)
                sl = c1 * (-sr) + s1 * cr
                _rot_rows(W, p, q, cl, sl, on)
                _rot_cols(U, p, q, cl, sl, on)
                _rot_cols(W, p, q, cr, -sr, on)
                _rot_cols(V, p, q, cr, -sr, on)
                max_diag = np.where(on, np.maximum(max_diag, np.maximum(np.abs(W[:, p, p]), np.abs(W[:, q, q]))), max_diag)
            alive &= any_rot
            if not alive.any():
                break
    a = np.diagonal(W, axis1=1, axis2=2)
    sv = np.abs(a) * scale[:, None]
    U = U * np.where(a < 0.0, -1.0, 1.0)[:, None, :]
    # descending selection sort, first maximum wins, stop at a zero maximum
    idx = np.arange(n)
    pos = np.zeros(n, int)
    pos = np.where(sv[:, 1] > sv[idx, pos], 1, pos)
    pos = np.where(sv[:, 2] > sv[idx, pos], 2, pos)
    go = sv[idx, pos] != 0.0

    def swap(mask, i, j):
        sv[mask, i], sv[mask, j] = sv[mask, j].copy(), sv[mask, i].copy()
        for M in (U, V):
            M[mask, :, i], M[mask, :, j] = M[mask, :, j].copy(), M[mask, :, i].copy()
    swap(go & (pos == 1), 0, 1)
    swap(go & (pos == 2), 0, 2)
    swap(go & (sv[:, 2] > sv[:, 1]), 1, 2)
    return U, sv, V


def _det3(m):
    return (m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1])
            - m[:, 0, 1] * (m[:, 1, 0] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 0])
            + m[:, 0, 2] * (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]))


def rotation_log(R):
    """rotation_log_exp::log -> ((log R)01, (log R)02, (log R)12) and the branch taken per matrix:
    0 zero angle, 1 angle pi, 2 regular, 3 regular with the 'larger than pi' retry, -1 not orthogonal / csin out of range (zeros)."""
    n = R.shape[0]
    E = np.einsum("nki,nkj->nij", R, R) - np.eye(3)
    ortho = ~(np.sqrt((E * E).sum((1, 2))) > LOG_TOL)
    csin = (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0) / 2.0
    out_range = (csin < -1.0) | (csin > 1.0)
    bad = out_range & (np.abs(csin - 1.0) > LOG_TOL) & (np.abs(csin + 1.0) > LOG_TOL)
    csin = np.where(out_range & ~bad, np.maximum(np.minimum(1.0, csin), -1.0), csin)
    with np.errstate(divide="ignore", invalid="ignore"):
        tangle = np.arccos(csin)
        zero = np.abs(tangle) < LOG_TOL
        is_pi = ~zero & (np.abs(tangle - np.pi) < LOG_TOL)
        B = (R + np.eye(3)) / 2.0
        k1 = np.sqrt(B[:, 0, 0])
        k2 = np.where(k1 * B[:, 0, 1] > 0.0, np.sqrt(B[:, 1, 1]), -np.sqrt(B[:, 1, 1]))
        k3 = np.where(k1 * B[:, 0, 2] > 0.0, np.sqrt(B[:, 2, 2]), -np.sqrt(B[:, 2, 2]))
        taxis = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
        sinv = np.sin(tangle)
        t = taxis / (2.0 * sinv)[:, None]
        omc = 1.0 - csin
        r01 = omc * t[:, 0] * t[:, 1] - t[:, 2] * sinv
        r02 = omc * t[:, 0] * t[:, 2] + t[:, 1] * sinv
        r10 = omc * t[:, 0] * t[:, 1] + t[:, 2] * sinv
        r12 = omc * t[:, 1] * t[:, 2] - t[:, 0] * sinv
        r20 = omc * t[:, 0] * t[:, 2] - t[:, 1] * sinv
        r21 = omc * t[:, 1] * t[:, 2] + t[:, 0] * sinv
        check = ((R[:, 0, 1] - r01) ** 2 + (R[:, 0, 2] - r02) ** 2 + (R[:, 1, 0] - r10) ** 2 + (R[:, 1, 2] - r12) ** 2
                 + (R[:, 2, 0] - r20) ** 2 + (R[:, 2, 1] - r21) ** 2)
        retry = ~(check < LOG_TOL)
        tangle2 = 2 * np.pi - tangle
        t2 = taxis / (2.0 * np.sin(tangle2))[:, None]
        angle = np.where(is_pi, np.pi, np.where(retry, tangle2, tangle))
        ax = np.where(is_pi[:, None], np.stack([k1, k2, k3], -1), np.where(retry[:, None], t2, t))
        lg = np.stack([angle * (0.0 - ax[:, 2]), angle * (ax[:, 1] - 0.0), angle * (0.0 - ax[:, 0])], -1)
    unset = ~ortho | bad
    lg = np.where((unset | zero)[:, None], 0.0, lg)
    branch = np.where(unset, -1, np.where(zero, 0, np.where(is_pi, 1, np.where(retry, 3, 2))))
    return lg, branch


def deform_grad64(verts_a, verts_b, faces, eps=1e-6, return_parts=False):
    """One frame: float32 vertices (as the reference's binding casts them) -> float64 (n_tris*9,)."""
    a = np.asarray(verts_a, np.float32).reshape(-1, 3).astype(np.float64)
    b = np.asarray(verts_b, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ea1, ea2 = a[f[:, 1]] - a[f[:, 0]], a[f[:, 2]] - a[f[:, 0]]
    eb1, eb2 = b[f[:, 1]] - b[f[:, 0]], b[f[:, 2]] - b[f[:, 0]]
    ea3, good_a = _edge3(ea1, ea2, eps)
    eb3, good_b = _edge3(eb1, eb2, eps)
    good = good_a & good_b
    A = np.stack([ea1, ea2, ea3], -1)
    B = np.stack([eb1, eb2, eb3], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.einsum("nij,njk->nik", B, _inverse(A))
    T = np.where(good[:, None, None], T, np.eye(3))         # degenerate rows are replaced by zeros below
    U, sv, V = jacobi_svd(T)
    d = _det3(np.einsum("nik,njk->nij", U, V))
    Ud = U.copy()
    Ud[:, :, 2] *= d[:, None]
    R = np.einsum("nik,njk->nij", Ud, V)
    Vd = V * np.stack([np.ones_like(d), np.ones_like(d), d], -1)[:, None, :]
    S = np.einsum("nik,njk->nij", Vd * sv[:, None, :], V)
    lg, branch = rotation_log(R)
    g = np.stack([S[:, 0, 0] - 1.0, S[:, 0, 1], S[:, 0, 2], S[:, 1, 1] - 1.0, S[:, 1, 2], S[:, 2, 2] - 1.0,
                  lg[:, 0], lg[:, 1], lg[:, 2]], -1)
    g = np.where(good[:, None], g, 0.0)
    if return_parts:
        return g.reshape(-1), dict(good=good, branch=np.where(good, branch, -2), T=T, R=R, S=S)
    return g.reshape(-1)
