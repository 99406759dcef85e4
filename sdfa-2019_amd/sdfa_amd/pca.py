"""PCA bases of dgrad and offsets tracks, fitted on the GPU: host side of the PCA fit in libsdfa_hip.so (csrc/pcafit.hip and
api_pca.cpp, C ABI in include/sdfa_pca.h).  It produces the tensors the regressor's last stage consumes, `*_pca.compT` and
`*_pca.means`, the way the reference's preload.pca_offsets / pca_dgrad do with sklearn.decomposition.PCA(0.97): the same
means, components, signs, variances and component count, for the leading components only.  The contract -- centring,
accumulation, determinism, refusals -- is written down in the header and in DESIGN.md section 11.

The rows stay where they are on the device, in one tensor or a list of chunks; the column selector addresses the scale
(9, 0, 6) and rotat (9, 6, 3) parts of interleaved dgrad rows in place.  fit() synchronises (the block-sized algebra runs
on the host between sweeps); transform() and inverse_transform() are stream-ordered.  A fit that did not converge raises;
a library without the PCA symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from ._lib import bind, lib, check, SdfaError
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_pca.h SDFA_PCA_ABI_VERSION this binding was written against
MAX_BLOCK, OVERSAMPLE, MAX_COMPONENTS, SLAB, ZSLAB = 256, 8, 248, 1024, 2048
ENOTCONVERGED, EZEROVAR, ERATIO = -32, -33, -34
SELECT_OFFSETS, SELECT_SCALE, SELECT_ROTAT = (1, 0, 1), (9, 0, 6), (9, 6, 3)


class Info(C.Structure):
    _fields_ = [("k", C.c_int64), ("sweeps", C.c_int64), ("block", C.c_int64), ("max_residual", C.c_double),
                ("total_sum_squares", C.c_double), ("z_pass_ms", C.c_double), ("y_pass_ms", C.c_double)]


_p, _i64, _d = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_pca_abi_version": (C.c_int, []),
    "sdfa_pca_workspace_bytes": (_i64, [_p, _i64, _i64, _i64, _i64, _i64]),
    "sdfa_pca_fit": (C.c_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _d, C.c_uint64, C.c_int, _d, C.c_int, _p, _p, _i64, _p, _p,
                               _p, _p, _i64, _p]),
    "sdfa_pca_transform": (C.c_int, [_p, _i64, _i64, _i64, _i64, _i64, _p, _p, _i64, _p, _p]),
    "sdfa_pca_inverse_transform": (C.c_int, [_p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i64, _p, _p]),
    "sdfa_pca_host_algebra": (C.c_int, [_p, _i64, _p, _p, _p]),
}


bind(SYMBOLS, "sdfa_pca_abi_version", ABI_VERSION, "pca")


class PcaNotConverged(SdfaError):
    """The fit ended without a result: the residual test failed, the rows have no variance, or the ratio is out of reach.
    `sweeps`, `block` and `max_residual` say where it stood."""

    def __init__(self, code, msg, info=None):
        super().__init__(code, msg)
        self.sweeps = int(info.sweeps) if info is not None else 0
        self.block = int(info.block) if info is not None else 0
        self.max_residual = float(info.max_residual) if info is not None else float("nan")


def selected_dim(W, select):
    g, o, t = select
    return W // g * t


def _chunks(rows):
    """One tensor or a list of them -> a list of contiguous float32 cuda [F_c][W] chunks (never copied when they already are)."""
    chunks = [rows] if torch.is_tensor(rows) else list(rows)
    assert chunks, "fit: no rows"
    out = []
    for c in chunks:
        assert torch.is_tensor(c) and c.is_cuda, "sdfa_amd.pca takes cuda tensors: there is no CPU path"
        assert c.dtype == torch.float32, c.dtype
        c = c.reshape(c.shape[0], -1)
        assert c.is_contiguous(), "rows must be contiguous (row stride W): the fit reads them in place"
        if c.shape[0]:
            out.append(c)
    assert out, "fit: no rows"
    assert len({(c.shape[1], c.device) for c in out}) == 1, "chunks differ in width or device"
    return out


@dataclass
class PcaFit:
    means: torch.Tensor                       # [D]
    components: torch.Tensor                  # [k][D], rows orthonormal
    explained_variance: torch.Tensor          # [k]
    explained_variance_ratio: torch.Tensor    # [k]
    k: int
    sweeps: int
    max_residual: float
    select: tuple
    width: int                                # W of the rows it was fitted on
    block: int = 0
    total_sum_squares: float = 0.0
    z_pass_ms: float = 0.0                    # device time of the last sweep's two passes over the rows
    y_pass_ms: float = 0.0
    _compT: torch.Tensor = None

    @property
    def compT(self):
        """components.T, [D][k] contiguous: the layout of `*_pca.compT`."""
        if self._compT is None:
            self._compT = self.components.t().contiguous()
        return self._compT

    def transform(self, rows):
        """[F][W] cuda rows -> [F][k] coefficients (x[sel] - means) @ compT."""
        assert torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32
        rows = rows.reshape(rows.shape[0], -1).contiguous()
        assert rows.shape[1] == self.width, (rows.shape, self.width)
        g, o, t = self.select
        with torch.cuda.device(rows.device):
            coef = torch.empty(rows.shape[0], self.k, dtype=torch.float32, device=rows.device)
            check(lib.sdfa_pca_transform(_ptr(rows), rows.shape[0], self.width, g, o, t, _ptr(self.means), _ptr(self.compT), self.k,
                                         _ptr(coef), _stream()))
        return coef

    def inverse_transform(self, coef, out=None):
        """[F][k] coefficients -> rows [F][W]: means + coef @ components, written into the selected columns of `out` only
        (a fresh `out` is zero elsewhere)."""
        assert torch.is_tensor(coef) and coef.is_cuda and coef.dtype == torch.float32
        coef = coef.reshape(-1, self.k).contiguous()
        g, o, t = self.select
        with torch.cuda.device(coef.device):
            if out is None:
                alloc = torch.empty if self.select == SELECT_OFFSETS else torch.zeros
                out = alloc(coef.shape[0], self.width, dtype=torch.float32, device=coef.device)
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == coef.shape[0] * self.width
            check(lib.sdfa_pca_inverse_transform(_ptr(coef), coef.shape[0], self.k, _ptr(self.means), _ptr(self.components), self.width,
                                                 g, o, t, _ptr(out), _stream()))
        return out

    def file_stem(self):
        return {SELECT_SCALE: "scale_", SELECT_ROTAT: "rotat_"}.get(tuple(self.select), "")

    def save(self, out_dir):
        """Writes the reference's files: {out_dir}/pca/[scale_|rotat_]compT.npy ([D][k]) and ...means.npy ([D]), float32."""
        d = os.path.join(out_dir, "pca")
        os.makedirs(d, exist_ok=True)
        stem = self.file_stem()
        np.save(os.path.join(d, stem + "compT.npy"), self.compT.cpu().numpy().astype(np.float32))
        np.save(os.path.join(d, stem + "means.npy"), self.means.cpu().numpy().astype(np.float32))

    def head_tensors(self, prefix):
        """The state-dict entries of a head: {prefix}_pca.compT [D][k] and {prefix}_pca.means [D]."""
        return {f"{prefix}_pca.compT": self.compT, f"{prefix}_pca.means": self.means}


def fit(rows_or_chunks, n_components=0.97, select=SELECT_OFFSETS, seed=0, block=None, tol=None, max_sweeps=None):
    """Fits the leading principal components of the selected columns of float32 cuda rows (one [F][W] tensor or a list of
    chunks of the same W).  n_components is a ratio in (0, 1) or an integer k >= 1, as in sklearn's PCA.  Synchronises."""
    chunks = _chunks(rows_or_chunks)
    dev, W = chunks[0].device, int(chunks[0].shape[1])
    g, o, t = (int(v) for v in select)
    n = len(chunks)
    ptrs = (C.c_void_p * n)(*[c.data_ptr() for c in chunks])
    nrows = (C.c_int64 * n)(*[int(c.shape[0]) for c in chunks])
    F = sum(nrows)
    need = int(check(lib.sdfa_pca_workspace_bytes(nrows, n, W, g, o, t)))
    D = selected_dim(W, (g, o, t))
    ncomp = float(n_components)
    by_ratio = 0.0 < ncomp < 1.0
    cap = max(1, min(MAX_COMPONENTS, F - 1, D)) if by_ratio else max(1, min(int(ncomp) if ncomp >= 1 else 1, MAX_COMPONENTS))
    info = Info()
    with torch.cuda.device(dev):
        means = torch.empty(D, dtype=torch.float32, device=dev)
        comps = torch.empty(cap, D, dtype=torch.float32, device=dev)
        var = torch.empty(cap, dtype=torch.float32, device=dev)
        ratio = torch.empty(cap, dtype=torch.float32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rc = lib.sdfa_pca_fit(ptrs, nrows, n, W, g, o, t, ncomp, int(seed) & (2 ** 64 - 1), int(block or 0), float(tol or 0.0),
                              int(max_sweeps or 0), _ptr(means), _ptr(comps), cap, _ptr(var), _ptr(ratio), C.byref(info), _ptr(ws),
                              need, _stream())
    if rc in (ENOTCONVERGED, EZEROVAR, ERATIO):
        raise PcaNotConverged(rc, lib.sdfa_last_error().decode("utf-8", "replace"), info)
    check(rc)
    k = int(info.k)
    return PcaFit(means=means, components=comps[:k], explained_variance=var[:k], explained_variance_ratio=ratio[:k], k=k,
                  sweeps=int(info.sweeps), max_residual=float(info.max_residual), select=(g, o, t), width=W, block=int(info.block),
                  total_sum_squares=float(info.total_sum_squares), z_pass_ms=float(info.z_pass_ms), y_pass_ms=float(info.y_pass_ms))


def fit_offsets(rows, n_components=0.97, **kw):
    """The offsets head's basis: the rows as they are."""
    return fit(rows, n_components, SELECT_OFFSETS, **kw)


def fit_dgrad(rows, n_components=0.97, **kw):
    """The dgrad head's two bases, (scale, rotat), from interleaved [F][T * 9] rows: per triangle six scale and three rotat
    values, as the regressor writes them.  Two fits, each reading the rows in place through its selector; they are not run in
    lock-step (DESIGN.md section 11 says why)."""
    return fit(rows, n_components, SELECT_SCALE, **kw), fit(rows, n_components, SELECT_ROTAT, **kw)


def host_algebra(a):
    """(evals descending, evecs as columns, R^-1 with a = R^T R) of a symmetric positive definite matrix, by the library's
    float64 host routines (cyclic Jacobi, Cholesky).  Host only; exists so that they can be checked on their own."""
    a = np.ascontiguousarray(a, np.float64)
    n = a.shape[0]
    assert a.shape == (n, n)
    w, v, r = np.empty(n), np.empty((n, n)), np.empty((n, n))
    check(lib.sdfa_pca_host_algebra(a.ctypes.data, n, w.ctypes.data, v.ctypes.data, r.ctypes.data))
    return w, v, r
