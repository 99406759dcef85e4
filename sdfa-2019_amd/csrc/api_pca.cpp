// Host driver of the PCA fit (include/sdfa_pca.h): a blocked subspace iteration with Rayleigh-Ritz.
// The rows are only ever touched by the kernels of pcafit.hip; everything of block size (b <= 256) -- the Cholesky factors
// of the orthonormalisation, the symmetric eigenproblem of the Ritz step, the choice of k -- runs here in float64.
//
// One sweep, with Q (D x b) orthonormal:
//     Z = Xc Q                 F x b     reads the rows; column slabs of SDFA_PCA_ZSLAB, so that few rows still fill the chip
//     T = Z^T Z                b x b     = Q^T C Q, C = Xc^T Xc; T = S diag(lambda) S^T on the host (cyclic Jacobi)
//     Y = Xc^T Z               D x b     reads the rows; = C Q
//     Qr = Q S, Yr = Y S                 Ritz vectors and C times them
//     res_i = ||Yr_i - lambda_i Qr_i||   from the difference vector, in double
//     Q <- orth(Yr)                      Cholesky-QR on the column-scaled Gram, repeated until the Gram is the identity
#include "host.h"
#include "pcafit.h"
#include "../../include/sdfa_pca.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int MAXB = SDFA_PCA_MAX_BLOCK, OVER = SDFA_PCA_OVERSAMPLE, SLAB = SDFA_PCA_SLAB, ZSLAB = SDFA_PCA_ZSLAB;

// a (n x n, symmetric, row-major) = L L^T; li = L^-1 (lower).  False when a pivot is not safely positive.
bool cholesky_inverse(std::vector<double> &a, int n, std::vector<double> &li, double min_pivot) {
    for (int j = 0; j < n; ++j) {
        double d = a[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
        if (!(d > min_pivot)) return false;
        const double ljj = std::sqrt(d);
        a[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double v = a[(size_t)i * n + j];
            const double *ri = &a[(size_t)i * n], *rj = &a[(size_t)j * n];
            for (int k = 0; k < j; ++k) v -= ri[k] * rj[k];
            a[(size_t)i * n + j] = v / ljj;
        }
    }
    li.assign((size_t)n * n, 0.0);
    for (int c = 0; c < n; ++c) {
        li[(size_t)c * n + c] = 1.0 / a[(size_t)c * n + c];
        for (int i = c + 1; i < n; ++i) {
            double v = 0.0;
            const double *ri = &a[(size_t)i * n];
            for (int k = c; k < i; ++k) v -= ri[k] * li[(size_t)k * n + c];
            li[(size_t)i * n + c] = v / ri[i];
        }
    }
    return true;
}

// Cyclic Jacobi on a symmetric n x n matrix (row-major, destroyed): w the eigenvalues in descending order, v[i][j]
// component i of eigenvector j.  Rotations whose off-diagonal element is below 2^-60 of its diagonal pair are skipped; the
// iteration ends when a whole cycle rotated nothing.
void jacobi_eigh(std::vector<double> &a, int n, std::vector<double> &w, std::vector<double> &v) {
    std::vector<double> vt((size_t)n * n, 0.0);            // rows are the eigenvectors while rotating
    for (int i = 0; i < n; ++i) vt[(size_t)i * n + i] = 1.0;
    const double tiny = std::ldexp(1.0, -60);
    for (int cycle = 0; cycle < 64; ++cycle) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
                if (apq == 0.0 || std::fabs(apq) <= tiny * std::sqrt(std::fabs(app * aqq))) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                double *rp = &a[(size_t)p * n], *rq = &a[(size_t)q * n];
                for (int k = 0; k < n; ++k) {              // rows p, q
                    const double x = rp[k], y = rq[k];
                    rp[k] = c * x - s * y;
                    rq[k] = s * x + c * y;
                }
                for (int k = 0; k < n; ++k) {              // columns p, q
                    double *rk = &a[(size_t)k * n];
                    const double x = rk[p], y = rk[q];
                    rk[p] = c * x - s * y;
                    rk[q] = s * x + c * y;
                }
                rp[q] = 0.0;
                rq[p] = 0.0;
                double *vp = &vt[(size_t)p * n], *vq = &vt[(size_t)q * n];
                for (int k = 0; k < n; ++k) {
                    const double x = vp[k], y = vq[k];
                    vp[k] = c * x - s * y;
                    vq[k] = s * x + c * y;
                }
            }
        if (!rotated) break;
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * n + x] > a[(size_t)y * n + y]; });
    w.resize(n);
    v.resize((size_t)n * n);
    for (int j = 0; j < n; ++j) {
        w[j] = a[(size_t)order[j] * n + order[j]];
        for (int i = 0; i < n; ++i) v[(size_t)i * n + j] = vt[(size_t)order[j] * n + i];
    }
}

struct Layout {
    int64_t q, y, yr, qr, z, part, g, m, lam, res, col, total;      // byte offsets
};

struct Shape {
    int64_t F, D, nslab_rows;      // nslab_rows: row slabs, cut per chunk
};

Layout layout(const Shape &s) {
    const int64_t nslab_d = (s.D + SLAB - 1) / SLAB, nslab_f = (s.F + SLAB - 1) / SLAB;
    Layout l;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += round_up(bytes, 256); return o; };
    const int64_t mat = s.D * MAXB * 4;
    l.q = take(mat);
    l.y = take(mat);
    l.yr = take(mat);
    l.qr = take(mat);
    l.z = take(s.F * MAXB * 4);
    int64_t part = s.nslab_rows * mat;                                       // Y partials (float), column moments (double) fit
    part = std::max(part, std::max(nslab_d, nslab_f) * (int64_t)MAXB * MAXB * 4);   // Gram partials
    part = std::max(part, std::max(s.nslab_rows * s.D, nslab_d * MAXB) * 8);
    part = std::max(part, (s.D + ZSLAB - 1) / ZSLAB * s.F * MAXB * 4);            // Z partials over column slabs
    l.part = take(part);
    l.g = take((int64_t)MAXB * MAXB * 4);
    l.m = take((int64_t)MAXB * MAXB * 4);
    l.lam = take(MAXB * 4);
    l.res = take(MAXB * 8);
    l.col = take(s.D * 8);
    l.total = at;
    return l;
}

// The argument checks every entry point shares.  Fills shape on success.
int check_rows(const char *who, const int64_t *chunk_rows, int64_t n_chunks, int64_t W, int64_t g, int64_t o, int64_t t, Shape *s) {
    if (!chunk_rows || n_chunks < 1) return sdfa_fail(SDFA_EINVAL, "%s: no chunks", who);
    if (W < 1 || W > (1ll << 30)) return sdfa_fail(SDFA_EINVAL, "%s: row width %lld outside 1 .. 2^30", who, (long long)W);
    if (g < 1 || g > W || W % g != 0) return sdfa_fail(SDFA_EINVAL, "%s: the row width %lld is no multiple of the group %lld", who, (long long)W, (long long)g);
    if (o < 0 || t < 1 || o + t > g)
        return sdfa_fail(SDFA_EINVAL, "%s: selector (first %lld, take %lld) leaves its group of %lld", who, (long long)o, (long long)t, (long long)g);
    s->F = 0;
    s->nslab_rows = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        if (chunk_rows[c] < 1 || chunk_rows[c] > (1ll << 40)) return sdfa_fail(SDFA_EINVAL, "%s: chunk %lld has %lld rows", who, (long long)c, (long long)chunk_rows[c]);
        s->F += chunk_rows[c];
        s->nslab_rows += (chunk_rows[c] + SLAB - 1) / SLAB;
    }
    s->D = W / g * t;
    if (s->nslab_rows > 65535) return sdfa_fail(SDFA_EINVAL, "%s: %lld row slabs of %d, at most 65535", who, (long long)s->nslab_rows, SLAB);
    // the column slabs of the Gram (SLAB) and of Z (ZSLAB) are the y dimension of their grids, like the row slabs above
    if (s->D > SDFA_PCA_MAX_COLUMNS)
        return sdfa_fail(SDFA_EINVAL, "%s: %lld selected columns, at most %lld (65535 slabs of %d)", who, (long long)s->D, (long long)SDFA_PCA_MAX_COLUMNS, SLAB);
    return SDFA_OK;
}

struct Fit {
    const float *const *chunks;
    const int64_t *rows;
    int64_t n_chunks;
    Shape s;
    PcaSel sel;
    hipStream_t st;
    float *mu, *Q, *Y, *Yr, *Qr, *Z, *part, *G, *M, *lam;
    double *res, *col;
    int b = 0;

    // g64 = src^T src for src [n][b], symmetrised, through the host
    int gram(const float *src, int64_t n, std::vector<double> &g64) {
        const int64_t nslab = (n + SLAB - 1) / SLAB;
        pca_mm_plain(true, src, b, b, n, src, b, b, part, b, SLAB, (int64_t)b * b, st);
        pca_reduce_f32(part, nslab, (int64_t)b * b, G, st);
        std::vector<float> h((size_t)b * b);
        HIP_TRY(hipMemcpyAsync(h.data(), G, h.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        g64.resize(h.size());
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) g64[(size_t)i * b + j] = 0.5 * ((double)h[(size_t)i * b + j] + (double)h[(size_t)j * b + i]);
        return SDFA_OK;
    }

    // dst[D][b] = src[D][b] * m (b x b, float64 on the host)
    int times_small(const float *src, const std::vector<double> &m, float *dst) {
        std::vector<float> h(m.size());
        for (size_t i = 0; i < m.size(); ++i) h[i] = (float)m[i];
        HIP_TRY(hipMemcpyAsync(M, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                      // h leaves scope
        pca_mm_plain(false, src, b, s.D, b, M, b, b, dst, b, b, 0, st);
        return SDFA_OK;
    }

    // dst = an orthonormal basis of span(src); tmp is scratch; src is destroyed when a third pass is needed.
    // Cholesky-QR: G = src^T src scaled to a unit diagonal = R^T R, src <- src diag(1 / |column|) R^-1, repeated (at least
    // twice, at most five times) until the Gram of the result is the identity to 1e-5.  > 0: the block lost rank.
    int orthonormalise(float *src, float *tmp, float *dst) {
        std::vector<double> g, li, m((size_t)b * b);
        const float *in = src;
        for (int pass = 0; pass < 6; ++pass) {
            int rc = gram(in, s.D, g);
            if (rc < 0) return rc;
            std::vector<double> d(b);
            double off = 0.0;
            for (int i = 0; i < b; ++i) {
                if (!(g[(size_t)i * b + i] > 0.0)) return 1;
                d[i] = 1.0 / std::sqrt(g[(size_t)i * b + i]);
            }
            for (int i = 0; i < b; ++i)
                for (int j = 0; j < b; ++j) {
                    if (i != j) off = std::max(off, std::fabs(g[(size_t)i * b + j]));
                    g[(size_t)i * b + j] *= d[i] * d[j];
                }
            bool unit = off <= 1e-5;
            for (int i = 0; i < b; ++i) unit = unit && std::fabs(1.0 / (d[i] * d[i]) - 1.0) <= 1e-5;
            if (pass >= 2 && unit && in == dst) return SDFA_OK;
            if (pass == 5) return 1;
            if (!cholesky_inverse(g, b, li, 1e-9)) return 1;
            for (int i = 0; i < b; ++i)
                for (int j = 0; j < b; ++j) m[(size_t)i * b + j] = d[i] * li[(size_t)j * b + i];
            float *out = in == tmp ? dst : tmp;
            rc = times_small(in, m, out);
            if (rc < 0) return rc;
            in = out;
        }
        return 1;
    }
};

}  // namespace

extern "C" {

int sdfa_pca_abi_version(void) { return SDFA_PCA_ABI_VERSION; }

int64_t sdfa_pca_workspace_bytes(const int64_t *chunk_rows, int64_t n_chunks, int64_t W, int64_t g, int64_t o, int64_t t) {
    Shape s;
    const int rc = check_rows("pca_workspace_bytes", chunk_rows, n_chunks, W, g, o, t, &s);
    if (rc < 0) return rc;
    return layout(s).total;
}

int sdfa_pca_fit(const float *const *d_chunks, const int64_t *chunk_rows, int64_t n_chunks, int64_t W, int64_t g, int64_t o,
                 int64_t t, double n_components, uint64_t seed, int block, double tol, int max_sweeps, float *d_means,
                 float *d_components, int64_t component_capacity, float *d_variance, float *d_ratio, sdfa_pca_info *info,
                 void *d_ws, int64_t ws_bytes, void *stream) {
    Fit f;
    int rc = check_rows("pca_fit", chunk_rows, n_chunks, W, g, o, t, &f.s);
    if (rc < 0) return rc;
    const int64_t F = f.s.F, D = f.s.D;
    if (F < 2) return sdfa_fail(SDFA_EINVAL, "pca_fit: %lld row, a fit needs at least 2", (long long)F);
    const int64_t rank_cap = std::min(F - 1, D);
    const bool by_ratio = n_components > 0.0 && n_components < 1.0;
    int64_t k_fixed = 0;
    if (!by_ratio) {
        if (!(n_components >= 1.0) || n_components != std::floor(n_components) || n_components > 1e9)
            return sdfa_fail(SDFA_EINVAL, "pca_fit: n_components %g is neither a ratio in (0, 1) nor an integer >= 1", n_components);
        k_fixed = (int64_t)n_components;
        if (k_fixed > rank_cap)
            return sdfa_fail(SDFA_EINVAL, "pca_fit: %lld components of %lld rows and %lld columns, at most min(F - 1, D) = %lld", (long long)k_fixed,
                             (long long)F, (long long)D, (long long)rank_cap);
        if (k_fixed > SDFA_PCA_MAX_COMPONENTS)
            return sdfa_fail(SDFA_EINVAL, "pca_fit: %lld components, the block of %d columns less %d of oversampling holds at most %d", (long long)k_fixed,
                             MAXB, OVER, SDFA_PCA_MAX_COMPONENTS);
        if (component_capacity < k_fixed) return sdfa_fail(SDFA_EINVAL, "pca_fit: room for %lld components, %lld asked for", (long long)component_capacity, (long long)k_fixed);
    }
    if (block != 0 && (block < 32 || block > MAXB || block % 32 != 0))
        return sdfa_fail(SDFA_EINVAL, "pca_fit: block %d is no multiple of 32 in 32 .. %d", block, MAXB);
    if (block != 0 && !by_ratio && block < rank_cap && k_fixed + OVER > block)
        return sdfa_fail(SDFA_EINVAL, "pca_fit: block %d is smaller than %lld components plus %d of oversampling", block, (long long)k_fixed, OVER);
    if (tol < 0.0 || max_sweeps < 0 || component_capacity < 1) return sdfa_fail(SDFA_EINVAL, "pca_fit: negative tol, max_sweeps or no component capacity");
    if (!d_chunks || !d_means || !d_components || !d_variance || !d_ratio || !info || !d_ws) return sdfa_fail(SDFA_EINVAL, "pca_fit: null pointer");
    for (int64_t c = 0; c < n_chunks; ++c)
        if (!d_chunks[c]) return sdfa_fail(SDFA_EINVAL, "pca_fit: chunk %lld is a null pointer", (long long)c);
    const Layout l = layout(f.s);
    if (ws_bytes < l.total) return sdfa_fail(SDFA_EINVAL, "pca_fit: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)l.total);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "pca_fit: workspace not 256-byte aligned");
    if (tol == 0.0) tol = SDFA_PCA_DEFAULT_TOL;
    if (max_sweeps == 0) max_sweeps = SDFA_PCA_DEFAULT_SWEEPS;

    char *ws = (char *)d_ws;
    f.chunks = d_chunks;
    f.rows = chunk_rows;
    f.n_chunks = n_chunks;
    f.sel = PcaSel{W, (int)g, (int)o, (int)t};
    f.st = (hipStream_t)stream;
    f.mu = d_means;
    f.Q = (float *)(ws + l.q);
    f.Y = (float *)(ws + l.y);
    f.Yr = (float *)(ws + l.yr);
    f.Qr = (float *)(ws + l.qr);
    f.Z = (float *)(ws + l.z);
    f.part = (float *)(ws + l.part);
    f.G = (float *)(ws + l.g);
    f.M = (float *)(ws + l.m);
    f.lam = (float *)(ws + l.lam);
    f.res = (double *)(ws + l.res);
    f.col = (double *)(ws + l.col);
    hipStream_t st = f.st;
    *info = sdfa_pca_info{0, 0, 0, 0.0, 0.0, 0.0, 0.0};

    // moments: column sums -> means, then the centred sum of squares, slab by slab in double
    std::vector<double> colsq((size_t)D);
    for (int pass = 0; pass < 2; ++pass) {
        int64_t slab = 0;
        for (int64_t c = 0; c < n_chunks; ++c) {
            pca_moment_slabs(d_chunks[c], f.sel, pass ? f.mu : nullptr, chunk_rows[c], D, (double *)f.part + slab * D, st);
            slab += (chunk_rows[c] + SLAB - 1) / SLAB;
        }
        pca_reduce_f64((const double *)f.part, slab, D, f.col, pass ? nullptr : f.mu, (double)F, st);
    }
    HIP_TRY(hipMemcpyAsync(colsq.data(), f.col, (size_t)D * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double total = 0.0;
    for (int64_t d = 0; d < D; ++d) total += colsq[(size_t)d];
    info->total_sum_squares = total;
    if (!(total > 0.0)) return sdfa_fail(SDFA_PCA_EZEROVAR, "pca_fit: the rows have no variance (sum of squares about the mean is %g)", total);

    int b = by_ratio ? (block ? block : 64) : (block ? block : (int)round_up(k_fixed + OVER, 32));
    b = (int)std::min<int64_t>(b, rank_cap);
    f.b = b;
    pca_start_block(nullptr, 0, f.Yr, b, D, seed, st);
    rc = f.orthonormalise(f.Yr, f.Y, f.Q);
    if (rc < 0) return rc;
    if (rc > 0) return sdfa_fail(SDFA_PCA_ENOTCONVERGED, "pca_fit: the start block of %d columns is rank deficient", b);

    std::vector<double> T, lam, S, res((size_t)MAXB);
    std::vector<float> lamf;
    double prev_cum = -1.0;
    int sweeps_here = 0;
    struct Events {                                                            // the two row passes of a sweep, timed on the device
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
    for (int sweep = 1;; ++sweep) {
        if (sweep > max_sweeps)
            return sdfa_fail(SDFA_PCA_ENOTCONVERGED, "pca_fit: not converged after %d sweeps (block %d, largest relative residual %.3g, tol %.3g)", max_sweeps, b,
                             info->max_residual, tol);
        info->sweeps = sweep;
        info->block = b;
        ++sweeps_here;
        int64_t row = 0, slab = 0;
        HIP_TRY(hipEventRecord(ev.e[0], st));
        for (int64_t c = 0; c < n_chunks; ++c) {                              // Z = Xc Q
            pca_mm_sel(false, d_chunks[c], f.sel, f.mu, chunk_rows[c], D, f.Q, b, b, f.part, b, ZSLAB, chunk_rows[c] * b, st);
            pca_reduce_f32(f.part, (D + ZSLAB - 1) / ZSLAB, chunk_rows[c] * b, f.Z + row * b, st);
            row += chunk_rows[c];
        }
        HIP_TRY(hipEventRecord(ev.e[1], st));
        rc = f.gram(f.Z, F, T);                                                // T = Z^T Z
        if (rc < 0) return rc;
        jacobi_eigh(T, b, lam, S);
        row = 0;
        HIP_TRY(hipEventRecord(ev.e[2], st));
        for (int64_t c = 0; c < n_chunks; ++c) {                              // Y = Xc^T Z, slab partials then their sum
            pca_mm_sel(true, d_chunks[c], f.sel, f.mu, D, chunk_rows[c], f.Z + row * b, b, b, f.part + slab * D * b, b, SLAB, D * b, st);
            row += chunk_rows[c];
            slab += (chunk_rows[c] + SLAB - 1) / SLAB;
        }
        pca_reduce_f32(f.part, slab, D * b, f.Y, st);
        HIP_TRY(hipEventRecord(ev.e[3], st));
        rc = f.times_small(f.Q, S, f.Qr);
        if (rc < 0) return rc;
        rc = f.times_small(f.Y, S, f.Yr);
        if (rc < 0) return rc;
        lamf.resize(b);
        for (int i = 0; i < b; ++i) lamf[i] = (float)lam[i];
        HIP_TRY(hipMemcpyAsync(f.lam, lamf.data(), (size_t)b * 4, hipMemcpyHostToDevice, st));
        const int64_t nslab_d = (D + SLAB - 1) / SLAB;
        pca_residual_slabs(f.Yr, f.Qr, f.lam, D, b, (double *)f.part, st);
        pca_reduce_f64((const double *)f.part, nslab_d, b, f.res, nullptr, 1.0, st);
        HIP_TRY(hipMemcpyAsync(res.data(), f.res, (size_t)b * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms_z = 0.f, ms_y = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_z, ev.e[0], ev.e[1]));
        HIP_TRY(hipEventElapsedTime(&ms_y, ev.e[2], ev.e[3]));
        info->z_pass_ms = ms_z;
        info->y_pass_ms = ms_y;
        if (!(lam[0] > 0.0)) return sdfa_fail(SDFA_PCA_ENOTCONVERGED, "pca_fit: the leading Ritz value is %g", lam[0]);
        for (int i = 0; i < b; ++i) res[i] = std::sqrt(res[i]) / lam[0];

        const int usable = b == rank_cap ? b : b - OVER;
        int64_t k = -1;
        double cum = 0.0;
        if (by_ratio) {
            for (int i = 0; i < usable && i < SDFA_PCA_MAX_COMPONENTS; ++i) {
                cum += lam[i] / total;
                if (cum > n_components) { k = i + 1; break; }
            }
        } else {
            k = k_fixed;
        }
        if (k > 0) {
            double worst = 0.0;
            for (int i = 0; i < k; ++i) worst = std::max(worst, res[i]);
            info->max_residual = worst;
            if (worst <= tol) {
                if (k > component_capacity) return sdfa_fail(SDFA_EINVAL, "pca_fit: %lld components reach the ratio, room for %lld", (long long)k, (long long)component_capacity);
                std::vector<float> var((size_t)k), ratio((size_t)k);
                for (int i = 0; i < k; ++i) {
                    var[i] = (float)(lam[i] / (double)(F - 1));
                    ratio[i] = (float)(lam[i] / total);
                }
                pca_finish(f.Qr, b, D, (int)k, d_components, st);
                HIP_TRY(hipMemcpyAsync(d_variance, var.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_ratio, ratio.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipStreamSynchronize(st));
                HIP_TRY(hipGetLastError());
                info->k = k;
                return SDFA_OK;
            }
        } else {
            // The ratio is not reached inside this block.  Ritz values only grow from sweep to sweep, so the block is given
            // up once their sum has stopped moving (by less than 1 % of what is missing): growing early costs time, never
            // correctness, because k is only ever decided on converged pairs.
            double worst = 0.0;
            for (int i = 0; i < usable; ++i) worst = std::max(worst, res[i]);
            info->max_residual = worst;
            const bool stalled = sweeps_here >= 2 && cum - prev_cum < 0.01 * (n_components - cum);
            prev_cum = cum;
            if (stalled || worst <= tol) {
                const int b2 = (int)std::min<int64_t>(std::min(2 * b, MAXB), rank_cap);
                if (b2 <= b)
                    return sdfa_fail(SDFA_PCA_ERATIO, "pca_fit: %d components explain %.6f of the variance, %.6f is not reached within %d", usable, cum,
                                     n_components, SDFA_PCA_MAX_COMPONENTS);
                pca_start_block(f.Qr, b, f.Yr, b2, D, seed, st);             // the Ritz vectors stay, new start columns join
                b = f.b = b2;
                sweeps_here = 0;
                prev_cum = -1.0;
                rc = f.orthonormalise(f.Yr, f.Y, f.Q);
                if (rc < 0) return rc;
                if (rc > 0) return sdfa_fail(SDFA_PCA_ENOTCONVERGED, "pca_fit: the grown block of %d columns is rank deficient", b);
                continue;
            }
        }
        rc = f.orthonormalise(f.Yr, f.Y, f.Q);
        if (rc < 0) return rc;
        if (rc > 0)
            return sdfa_fail(SDFA_PCA_ENOTCONVERGED, "pca_fit: the block of %d columns lost rank in sweep %d (the rows span fewer directions)", b, sweep);
    }
}

int sdfa_pca_transform(const float *d_rows, int64_t F, int64_t W, int64_t g, int64_t o, int64_t t, const float *d_means,
                       const float *d_compT, int64_t k, float *d_coef, void *stream) {
    Shape s;
    const int64_t rows[1] = {F};
    if (F == 0) return SDFA_OK;
    const int rc = check_rows("pca_transform", rows, 1, W, g, o, t, &s);
    if (rc < 0) return rc;
    if (k < 1 || k > MAXB) return sdfa_fail(SDFA_EINVAL, "pca_transform: %lld components outside 1 .. %d", (long long)k, MAXB);
    if (!d_rows || !d_means || !d_compT || !d_coef) return sdfa_fail(SDFA_EINVAL, "pca_transform: null pointer");
    pca_mm_sel(false, d_rows, PcaSel{W, (int)g, (int)o, (int)t}, d_means, F, s.D, d_compT, k, (int)k, d_coef, k, s.D, 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

int sdfa_pca_inverse_transform(const float *d_coef, int64_t F, int64_t k, const float *d_means, const float *d_components,
                               int64_t W, int64_t g, int64_t o, int64_t t, float *d_rows, void *stream) {
    Shape s;
    const int64_t rows[1] = {F};
    if (F == 0) return SDFA_OK;
    const int rc = check_rows("pca_inverse_transform", rows, 1, W, g, o, t, &s);
    if (rc < 0) return rc;
    if (k < 1 || k > MAXB) return sdfa_fail(SDFA_EINVAL, "pca_inverse_transform: %lld components outside 1 .. %d", (long long)k, MAXB);
    if (!d_coef || !d_means || !d_components || !d_rows) return sdfa_fail(SDFA_EINVAL, "pca_inverse_transform: null pointer");
    pca_expand(d_coef, F, (int)k, d_means, d_components, s.D, PcaSel{W, (int)g, (int)o, (int)t}, d_rows, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

int sdfa_pca_host_algebra(const double *a, int64_t n, double *evals, double *evecs, double *rinv) {
    if (!a || !evals || !evecs || !rinv) return sdfa_fail(SDFA_EINVAL, "pca_host_algebra: null pointer");
    if (n < 1 || n > MAXB) return sdfa_fail(SDFA_EINVAL, "pca_host_algebra: order %lld outside 1 .. %d", (long long)n, MAXB);
    std::vector<double> m(a, a + n * n), w, v, li;
    jacobi_eigh(m, (int)n, w, v);
    std::copy(w.begin(), w.end(), evals);
    std::copy(v.begin(), v.end(), evecs);
    m.assign(a, a + n * n);
    if (!cholesky_inverse(m, (int)n, li, 0.0)) return sdfa_fail(SDFA_EINVAL, "pca_host_algebra: the matrix is not positive definite");
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) rinv[i * n + j] = li[(size_t)(j * n + i)];
    return SDFA_OK;
}

}  // extern "C"
