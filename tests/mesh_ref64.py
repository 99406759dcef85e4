"""Float64 restatement of the dgrad -> mesh stage (seek blend, right-hand side, solve, scatter), for judging the fp32 kernels.

TEST INFRASTRUCTURE ONLY.  Torch float64, vectorised over triangles and frames, on "cpu" or "cuda:0"; nothing here calls a project
kernel.  It follows oracle/mesh_oracle.py and what that file cites -- deformation/cpp/src/deform_triangle_impl.hpp (setStaticTarget
:8-140, getMeshFromDeformationGradients :215-310) and rotation/utils_rotation.cpp:33-49 -- and is written independently of the
product's host code:

  * triangle edges are subtracted in float32 and then widened (:96-97); the per-triangle pseudo-inverse is R^-1 Q^T of a QR (:98-100);
  * A (free vertices) and Ar (constrained ones) are kept as index lists (equation, column, three coefficients), A^T A + reg I dense;
  * the right-hand side is A^T (M - Ar C) on ABSOLUTE positions (:282-286) -- the kernels solve for the displacement from the
    template instead, so the two share no intermediate value;
  * the system is solved by a float64 Cholesky factorisation and two triangular solves: no inverse is formed, nothing is rounded
    to float32 before the result;
  * transform(): identity below an angle of 1e-10, otherwise Rodrigues on the angle-scaled skew matrix, all in double.

seek_plan() / blend() restate saber.stream.seek for the uniform video-rate queries (oracle/sdfa_oracle.py seek_track,
speech_anime/stream.py): the search and the weights on the host in numpy, the blend as numpy's three separately rounded float32
array operations.

The keyword arguments `drop_incidence`, `stale_frame` and `skip_k_block` of get_mesh() perturb the reference the way a subtle kernel
bug would; the GPU test uses them to show that its bounds catch such a bug.  Each acts on what the kernels would lose: the
displacement part of the term, not the absolute one (which would move even the rest pose by the template's own size).

Pinned to the reference project's fixtures by tests/test_mesh_ref64_cpu.py.
"""
import numpy as np
import torch

F64 = torch.float64


class MeshRef64:
    def __init__(self, verts, faces, cnsts, reg=1e-10, corr_count=None, corr_faces=None, device="cpu"):
        V = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
        F = np.asarray(faces, np.int64).reshape(-1, 3)
        cn = np.asarray(cnsts, np.int64).reshape(-1)
        self.device = device
        self.n_verts, self.n_tris = len(V), len(F)
        free = np.setdiff1d(np.arange(len(V)), cn)
        self.free, self.cn = free, cn
        self.n_free = len(free)
        col = -np.ones(len(V), np.int64)
        col[free] = np.arange(len(free))
        self.col = col
        # equations (:16-21, :102): target triangle j contributes max(1, count[j]) of them; an equation of a triangle with
        # correspondences takes the transform of source triangle corr_faces[k], the others (count 0: one filler entry) the identity
        if corr_count is None:
            eq_tri = np.arange(len(F))
            eq_src = eq_tri.copy()
        else:
            count = np.asarray(corr_count, np.int64).reshape(-1)
            eq_tri = np.repeat(np.arange(len(F)), np.maximum(1, count))
            cf = np.asarray(corr_faces, np.int64).reshape(-1)
            assert len(cf) == len(eq_tri), "corr_faces holds one entry per equation"
            eq_src = np.where(count[eq_tri] > 0, cf, -1)
        self.n_eq = len(eq_tri)
        self.eq_src = eq_src
        # per-triangle pseudo-inverse U (2 x 3) of [v2 - v1, v3 - v1]; the coefficients of the three corners: -U0 - U1, U0, U1
        Va = torch.from_numpy(np.stack([V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]], 2)).to(F64)      # float32 subtraction
        Q, R = torch.linalg.qr(Va)
        U = torch.linalg.solve_triangular(R, Q.transpose(1, 2), upper=True).numpy()                          # (T, 2, 3)
        coef = np.stack([-U[:, 0] - U[:, 1], U[:, 0], U[:, 1]], 1)[eq_tri]                                  # (E, corner, 3)
        vert = F[eq_tri]                                                                                     # (E, corner)
        is_free = col[vert] >= 0
        # index lists: A[3e + r, col] = coef[r] for free corners, Ar[3e + r, ccol] = coef[r] for constrained ones
        e_idx = np.broadcast_to(np.arange(self.n_eq)[:, None], vert.shape)
        k_idx = np.broadcast_to(np.arange(3)[None, :], vert.shape)
        self.a_eq, self.a_corner, self.a_vert, self.a_coef = e_idx[is_free], k_idx[is_free], vert[is_free], coef[is_free]
        self.r_eq, self.r_vert, self.r_coef = e_idx[~is_free], vert[~is_free], coef[~is_free]
        AtA = np.zeros((self.n_free, self.n_free))
        for k in range(3):
            for l in range(3):
                m = is_free[:, k] & is_free[:, l]
                np.add.at(AtA, (col[vert[m, k]], col[vert[m, l]]), (coef[m, k] * coef[m, l]).sum(1))
        AtA[np.arange(self.n_free), np.arange(self.n_free)] += reg                                           # :122-131
        self.AtA = torch.from_numpy(AtA)
        self.chol = torch.linalg.cholesky(self.AtA)                                                          # on the host, once
        # (Ar C) per equation, (E, 3, 3): rows r of the equation's block, columns the coordinate
        ArC = np.zeros((self.n_eq, 3, 3))
        np.add.at(ArC, self.r_eq, self.r_coef[:, :, None] * V[self.r_vert].astype(np.float64)[:, None, :])
        t = lambda a, dt=F64: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
        self.V64 = t(V)
        self.d_ArC, self.d_chol = t(ArC), self.chol.to(device)
        self.d_coef = t(coef)                                                        # every corner's; the column says which list
        self.d_cols = t(np.where(is_free, col[vert], self.n_free), torch.int64)      # A's column, or n_free for an entry of Ar
        self.d_eq_src = t(np.maximum(eq_src, 0), torch.int64)
        self.d_eq_ident = t(eq_src < 0, torch.bool)
        self.d_free = t(free, torch.int64)
        self.plain = corr_count is None
        self._inv = None
        self._rhs_rest = None

    # ------------------------------------------------------------------ the stage
    @staticmethod
    def transform(d):
        """exp(log R) S of 9-vectors (..., 9) in float64 -> (..., 3, 3)   (:225-242; utils_rotation.cpp:33-49)."""
        d = d.to(F64)
        ang = torch.sqrt(d[..., 6] ** 2 + d[..., 7] ** 2 + d[..., 8] ** 2)
        ident = ang < 1e-10
        safe = torch.where(ident, torch.ones_like(ang), ang)
        n1, n2, n3 = d[..., 6] / safe, d[..., 7] / safe, d[..., 8] / safe            # K / angle = [[0 n1 n2] [-n1 0 n3] [-n2 -n3 0]]
        s, c = torch.sin(ang), 1 - torch.cos(ang)
        one, zero = torch.ones_like(ang), torch.zeros_like(ang)
        # I + sin K + (1 - cos) K^2, entry by entry (3 x 3 products of millions of matrices as elementwise operations)
        R = [[1 - c * (n1 * n1 + n2 * n2), s * n1 - c * n2 * n3, s * n2 + c * n1 * n3],
             [-s * n1 - c * n2 * n3, 1 - c * (n1 * n1 + n3 * n3), s * n3 - c * n1 * n2],
             [-s * n2 + c * n1 * n3, -s * n3 - c * n1 * n2, 1 - c * (n2 * n2 + n3 * n3)]]
        eye = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
        R = [[torch.where(ident, eye[i][j], R[i][j]) for j in range(3)] for i in range(3)]
        S = [[d[..., 0] + 1, d[..., 1], d[..., 2]], [d[..., 1], d[..., 3] + 1, d[..., 4]], [d[..., 2], d[..., 4], d[..., 5] + 1]]
        T = [R[i][0] * S[0][j] + R[i][1] * S[1][j] + R[i][2] * S[2][j] for i in range(3) for j in range(3)]
        return torch.stack(T, -1).reshape(d.shape[:-1] + (3, 3))

    def _rhs(self, T):
        """A^T (M - Ar C) for transforms T (n, n_src, 3, 3) -> (n_free, n, 3); M's block of an equation is its transform transposed."""
        n = T.shape[0]
        G = T.transpose(2, 3) if self.plain else T[:, self.d_eq_src].transpose(2, 3)
        if not self.plain:
            G = torch.where(self.d_eq_ident[None, :, None, None], torch.eye(3, dtype=F64, device=T.device), G)
        G = G - self.d_ArC                                                                                   # (n, E, 3, 3)
        rhs = torch.zeros((n, self.n_free + 1, 3), dtype=F64, device=T.device)       # last row: where constrained corners go
        for k in range(3):               # the entries of A, one corner of every equation at a time: sum_r coef[r] * block[r, :]
            c = self.d_coef[:, k]
            rhs.index_add_(1, self.d_cols[:, k], c[:, 0][None, :, None] * G[:, :, 0] + c[:, 1][None, :, None] * G[:, :, 1]
                           + c[:, 2][None, :, None] * G[:, :, 2])
        return rhs[:, :self.n_free].permute(1, 0, 2).contiguous()

    def _solve(self, rhs):
        """(A^T A + reg I) X = rhs by the Cholesky factor: two float64 triangular solves."""
        y = torch.linalg.solve_triangular(self.d_chol, rhs.reshape(self.n_free, -1), upper=False)
        return torch.linalg.solve_triangular(self.d_chol.T, y, upper=True).reshape(rhs.shape)

    def frames_per_chunk(self):
        """So that the 9 x triangles x frames block of float64 transforms stays at a quarter of a GiB (it, the entry-wise temporaries
        of transform(), the per-equation blocks and one corner's products then stay below about 1 GiB together)."""
        return max(1, (2 ** 30 // 4) // (72 * max(self.n_eq, int(self.eq_src.max()) + 1)))

    @torch.no_grad()
    def get_mesh(self, dgrad_rows, drop_incidence=None, stale_frame=None, skip_k_block=None, want_system=False):
        """float32 rows (n, n_src_tris * 9) -> float64 vertices (n, n_verts, 3) on self.device.

        drop_incidence=(vertex, k): the k-th incidence of free vertex `vertex` loses its term of the right-hand side.
        stale_frame=(f, g): frame f is solved from frame g's transforms.
        skip_k_block=(row_tile, kb): the 128 unknowns of row tile `row_tile` are computed without the 32 unknowns of block `kb` of
        the contraction, as a GEMM tile that skips one K block would: X - Inv64[rows, block] @ rhs[block], with the displacement
        right-hand side the kernels contract and a float64 inverse that only this control uses.
        want_system: also return (X, rhs) of the last chunk, for residual()."""
        d = torch.as_tensor(dgrad_rows)
        assert d.dtype == torch.float32, "the stage takes float32 rows"
        d = d.reshape(d.shape[0], -1, 9)
        if stale_frame is not None:
            d = d.clone()
            d[stale_frame[0]] = d[stale_frame[1]]
        dropped = None
        if drop_incidence is not None:
            v, k = drop_incidence
            hits = np.nonzero(self.a_vert == v)[0]
            assert self.col[v] >= 0 and k < len(hits), "drop_incidence needs a free vertex and one of its incidences"
            dropped = int(hits[k])
        n = d.shape[0]
        out = self.V64.unsqueeze(0).repeat(n, 1, 1)
        step = self.frames_per_chunk()
        system = None
        for f0 in range(0, n, step):
            T = self.transform(d[f0:f0 + step].to(self.device))
            rhs = self._rhs(T)
            if dropped is not None:      # coef . (T^T - I) of that entry: the term mesh_rhs_kernel would not have added
                e = int(self.a_eq[dropped])
                Te = torch.eye(3, dtype=F64, device=T.device).expand(T.shape[0], 3, 3) if self.eq_src[e] < 0 else T[:, int(self.eq_src[e])]
                rhs[self.col[v]] -= torch.einsum("r,nrs->ns", self.d_coef[e, int(self.a_corner[dropped])], Te.transpose(1, 2) - torch.eye(3, dtype=F64, device=T.device))
            del T
            X = self._solve(rhs)
            if skip_k_block is not None:
                tile, kb = skip_k_block
                rows = slice(tile * 128, min(tile * 128 + 128, self.n_free))
                blk = slice(kb * 32, min(kb * 32 + 32, self.n_free))
                assert rows.start < self.n_free and blk.start < self.n_free
                disp = rhs - self.rhs_rest()[:, None, :]
                X[rows] -= torch.einsum("pk,kns->pns", self.inverse()[rows, blk], disp[blk])
            out[f0:f0 + step, self.d_free] = X.permute(1, 0, 2)
            if want_system:
                system = (X, rhs)
        return (out, system) if want_system else out

    def rhs_rest(self):
        """The right-hand side of the rest pose (every transform the identity), (n_free, 3)."""
        if self._rhs_rest is None:
            n_src = int(self.eq_src.max()) + 1
            T = torch.eye(3, dtype=F64, device=self.device).expand(1, n_src, 3, 3)
            self._rhs_rest = self._rhs(T)[:, 0]
        return self._rhs_rest

    def inverse(self):
        """A float64 inverse of the system, for the skip_k_block control only."""
        if self._inv is None:
            self._inv = torch.cholesky_inverse(self.chol).to(self.device)
        return self._inv

    @torch.no_grad()
    def residual(self, dgrad_rows):
        """|(A^T A + reg I) X - rhs| / |rhs| (max norms) of this reference's own solve of the given frames (one chunk)."""
        _, (X, rhs) = self.get_mesh(dgrad_rows, want_system=True)
        r = self.AtA.to(self.device) @ X.reshape(self.n_free, -1) - rhs.reshape(self.n_free, -1)
        return float(r.abs().max() / rhs.abs().max())

    # ------------------------------------------------------------------ saber.stream.seek
    @staticmethod
    def query_count(last_timestamp, fps):
        """len(range(int(tslist[-1] * fps / 1000.0) + 1))   (speech_anime/model/model.py:205-207)."""
        return max(0, int(int(last_timestamp) * float(fps) / 1000.0) + 1)

    @staticmethod
    def seek_plan(tslists, fps, query_counts=None):
        """For clips whose rows are concatenated in order: per query (global row of frame m, of frame m + 1 or m again) int64 and the
        two float32 weights -- (n_queries, 2) each.  Query i of a clip is at i * 1000.0 / fps; before the first / after the last
        timestamp and on the last frame the row is copied (m, m, 1, 0); otherwise a = (t[m+1] - ts) / (t[m+1] - t[m]) in float64
        and the weights are float32(a), float32(1 - a), as numpy applies a Python float to a float32 array.  `query_counts`: per
        clip, how many queries to plan instead of model.py's count (stream.seek itself takes any time)."""
        fps = float(fps)
        src, w, f0 = [], [], 0
        for c, tl in enumerate(tslists):
            t = np.asarray([int(x) for x in tl], np.int64)
            n = len(t)
            nq = MeshRef64.query_count(t[-1], fps) if query_counts is None else int(query_counts[c])
            ts = np.arange(nq, dtype=np.float64) * 1000.0 / fps
            m = np.clip(np.searchsorted(t, ts, side="right") - 1, 0, n - 1)       # last m with t[m] <= ts
            copy = (ts < t[0]) | (ts > t[-1]) | (m + 1 >= n)
            m1 = np.minimum(m + 1, n - 1)
            with np.errstate(divide="ignore", invalid="ignore"):
                a = (t[m1] - ts) / (t[m1] - t[m]).astype(np.float64)
            wa = np.where(copy, np.float32(1), a.astype(np.float32))
            wb = np.where(copy, np.float32(0), (1.0 - a).astype(np.float32))
            src.append(np.stack([f0 + m, f0 + np.where(copy, m, m1)], 1))
            w.append(np.stack([wa, wb], 1).astype(np.float32))
            f0 += n
        return np.concatenate(src).astype(np.int64), np.concatenate(w).astype(np.float32)

    @staticmethod
    def blend(rows, src, w):
        """w[:, 0] * rows[src[:, 0]] + w[:, 1] * rows[src[:, 1]]: three float32 array operations, each rounded on its own (numpy
        arrays on the host, torch tensors on any device: eager elementwise kernels, nothing contracted into an FMA)."""
        if torch.is_tensor(rows):
            src = torch.as_tensor(src, device=rows.device)
            w = torch.as_tensor(w, device=rows.device)
            assert rows.dtype == torch.float32 and w.dtype == torch.float32
            shape = (-1,) + (1,) * (rows.dim() - 1)
            x = w[:, 0].reshape(shape) * rows[src[:, 0]]
            y = w[:, 1].reshape(shape) * rows[src[:, 1]]
            return x + y
        rows, w = np.asarray(rows), np.asarray(w)
        assert rows.dtype == np.float32 and w.dtype == np.float32
        shape = (-1,) + (1,) * (rows.ndim - 1)
        x = w[:, 0].reshape(shape) * rows[src[:, 0]]
        y = w[:, 1].reshape(shape) * rows[src[:, 1]]
        return x + y
