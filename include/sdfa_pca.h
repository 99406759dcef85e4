/* C ABI of the PCA fit in libsdfa_hip.so (sdfa-2019_amd/csrc/pcafit.hip, api_pca.cpp): the bases `*_pca.compT` and
 * `*_pca.means` of the regressor's last stage, fitted on the device from float32 rows that stay where they are.
 * It restates sklearn.decomposition.PCA(n_components) as the reference uses it (preload.py pca_offsets / pca_dgrad) for the
 * leading components only: a blocked subspace iteration with Rayleigh-Ritz, not a full SVD.  DESIGN.md section 11.
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative code on failure (SDFA_E* or one of
 * the SDFA_PCA_E* below), sdfa_last_error() describes the failure.  The surface is stateless.  It is versioned on its own
 * (SDFA_PCA_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Rows      n_chunks chunks of float32 device rows [F_c][W], row stride W, the same W in every chunk; F = sum F_c.  The
 *           rows are only read.
 * Selector  (g, o, t) with W % g == 0, 0 <= o, 1 <= t, o + t <= g; D = (W / g) * t.  Selected column d is row column
 *           (d / t) * g + o + d % t.  offsets: (1, 0, 1); dgrad scale: (9, 0, 6); dgrad rotat: (9, 6, 3).  The selector only
 *           addresses: a fit through it equals, bit for bit, the fit of a contiguous copy of those columns.
 * Centring  mu[d] = float32(sum_r x[r][d] / F), the sum in double.  Every operand element enters a matrix instruction as
 *           the float32 difference x - mu, formed as it is loaded; no rank-one correction after a product exists.
 * Sums      column sums and sum (x - mu)^2 accumulate in double.  Every reduction over rows or columns runs over fixed
 *           slabs of SDFA_PCA_SLAB (per chunk for rows; SDFA_PCA_ZSLAB columns for Z = Xc Q) whose partial results are
 *           added in ascending order; there are no atomics.  The same
 *           rows in the same chunking give the same bits; another chunking may differ in the last bits.
 * Start     Q0[d][j] = u(seed, d, j) orthonormalised, with h = seed * 0x9E3779B1 ^ (d + 1) * 0x85EBCA77 ^ (j + 1) *
 *           0xC2B2AE3D (uint32, seed folded as lo ^ hi), h ^= h >> 16, h *= 0x85EBCA6B, h ^= h >> 13, h *= 0xC2B2AE35,
 *           h ^= h >> 16 and u = (h >> 8) * 2^-23 - 1, a float32 in [-1, 1).
 * Result    means[D]; components[k][D] with orthonormal rows, each signed so that its entry of largest magnitude (first
 *           index on ties) is positive; explained_variance[i] = lambda_i / (F - 1); explained_variance_ratio[i] =
 *           lambda_i / sum (x - mu)^2 over all rows and selected columns; lambda_i the Ritz values of Xc^T Xc.
 * k         n_components in (0, 1): the smallest k whose cumulative ratio exceeds it, searchsorted(cumsum(ratio),
 *           n_components, side="right") + 1.  n_components an integer >= 1: that k.  k <= min(F - 1, D) and
 *           k <= SDFA_PCA_MAX_COMPONENTS.
 * Block     b columns are iterated, b a multiple of 32 in 32 .. SDFA_PCA_MAX_BLOCK with k + SDFA_PCA_OVERSAMPLE <= b, or
 *           b = min(F - 1, D) when that is smaller (the block is then the whole row space and no oversampling is needed).
 *           block = 0 chooses: the smallest such b for an integer k; 64, then 128, then 256 for a ratio, the converged
 *           vectors kept when it grows.
 * Stop      when every kept component has ||C q_i - lambda_i q_i|| <= tol * lambda_1 (C = Xc^T Xc, the norm taken of the
 *           difference vector).  tol = 0 and max_sweeps = 0 choose the defaults below.
 * Limits    D <= SDFA_PCA_MAX_COLUMNS and at most 65535 row slabs (refused on the host).  Rows of exact rank below the
 *           block: when the centred rows span fewer than b directions although min(F - 1, D) > b (noise-free synthetic rows
 *           of rank 10 at block 32, say), the block's surplus columns are rounding noise.  The orthonormalisation takes a
 *           Cholesky pivot <= 1e-9 on the unit-diagonal Gram as lost rank, and the fit then ends with
 *           SDFA_PCA_ENOTCONVERGED ("lost rank") -- never with a result.  Whether the noise keeps the pivots above that
 *           depends on the rows; measured tracks carry noise in every direction and do not meet this.
 */
#ifndef SDFA_PCA_H
#define SDFA_PCA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_PCA_ABI_VERSION 1

#define SDFA_PCA_MAX_BLOCK       256    /* columns of the iterated block */
#define SDFA_PCA_OVERSAMPLE      8      /* block columns beyond the kept ones */
#define SDFA_PCA_MAX_COMPONENTS  248    /* SDFA_PCA_MAX_BLOCK - SDFA_PCA_OVERSAMPLE: the cap on k */
#define SDFA_PCA_SLAB            1024   /* rows (or columns) per reduction slab */
#define SDFA_PCA_ZSLAB           2048   /* columns per slab of Z = Xc Q */
#define SDFA_PCA_MAX_COLUMNS     (65535LL * SDFA_PCA_SLAB)   /* the cap on D: column slabs are a grid's y dimension */
#define SDFA_PCA_DEFAULT_TOL     3e-6   /* 4 x the largest residual floor measured; DESIGN.md section 11 "Numbers" */
#define SDFA_PCA_DEFAULT_SWEEPS  20     /* twice the most sweeps a converging case of the test matrix needed */

#define SDFA_PCA_ENOTCONVERGED  -32     /* the residual test failed within max_sweeps, or the block lost rank */
#define SDFA_PCA_EZEROVAR       -33     /* sum (x - mu)^2 == 0: every row is the same (sklearn returns NaN ratios) */
#define SDFA_PCA_ERATIO         -34     /* the ratio is not reached within SDFA_PCA_MAX_COMPONENTS components */

typedef struct sdfa_pca_info {
    int64_t k;                 /* components kept */
    int64_t sweeps;            /* sweeps used (each reads the rows twice), over every block size tried */
    int64_t block;             /* the block size the result comes from */
    double max_residual;       /* largest ||C q_i - lambda_i q_i|| / lambda_1 of the kept components */
    double total_sum_squares;  /* sum (x - mu)^2 */
    double z_pass_ms;          /* device time of the last sweep's Z = Xc Q (every chunk), by events */
    double y_pass_ms;          /* device time of the last sweep's Y = Xc^T Z with the sum of its slab partials */
} sdfa_pca_info;

int sdfa_pca_abi_version(void);

/* Device workspace of one sdfa_pca_fit call (any n_components and block), a multiple of 256 bytes. */
int64_t sdfa_pca_workspace_bytes(const int64_t *chunk_rows, int64_t n_chunks, int64_t W, int64_t g, int64_t o, int64_t t);

/* Fits.  d_chunks[c] points to chunk c (device), chunk_rows[c] is F_c; both arrays are host memory.  d_means [D],
 * d_components [component_capacity][D], d_variance and d_ratio [component_capacity] are device float32; rows 0 .. k - 1
 * are written, k = info->k.  component_capacity must be at least an integer k; for a ratio min(SDFA_PCA_MAX_COMPONENTS,
 * F - 1, D) always suffices.  d_ws is 256-byte aligned, at least sdfa_pca_workspace_bytes().
 * Refused with SDFA_EINVAL before any launch: F < 2, W % g != 0, a selector outside its group, n_components neither in
 * (0, 1) nor an integer >= 1, k > min(F - 1, D), k > SDFA_PCA_MAX_COMPONENTS, a block that is no multiple of 32 in 32 ..
 * 256 or smaller than k + SDFA_PCA_OVERSAMPLE, null pointers, a short workspace.  Known only later: SDFA_PCA_EZEROVAR,
 * SDFA_PCA_ERATIO, SDFA_PCA_ENOTCONVERGED; then the result buffers hold nothing usable (info is still filled).
 * THIS CALL SYNCHRONISES `stream` several times per sweep: the block-sized algebra (Cholesky, the symmetric eigenproblem)
 * runs in float64 on the host between the launches. */
int sdfa_pca_fit(const float *const *d_chunks, const int64_t *chunk_rows, int64_t n_chunks, int64_t W, int64_t g, int64_t o,
                 int64_t t, double n_components, uint64_t seed, int block, double tol, int max_sweeps, float *d_means,
                 float *d_components, int64_t component_capacity, float *d_variance, float *d_ratio, sdfa_pca_info *info,
                 void *d_ws, int64_t ws_bytes, void *stream);

/* d_coef[r][i] = sum_d (x[r][sel(d)] - means[d]) * compT[d][i]: d_rows [F][W], d_compT [D][k], d_coef [F][k].
 * Stream-ordered, does not synchronise. */
int sdfa_pca_transform(const float *d_rows, int64_t F, int64_t W, int64_t g, int64_t o, int64_t t, const float *d_means,
                       const float *d_compT, int64_t k, float *d_coef, void *stream);

/* d_rows[r][sel(d)] = means[d] + sum_i coef[r][i] * components[i][d] (i ascending); the other columns of d_rows are not
 * touched.  d_components [k][D].  Stream-ordered, does not synchronise. */
int sdfa_pca_inverse_transform(const float *d_coef, int64_t F, int64_t k, const float *d_means, const float *d_components,
                               int64_t W, int64_t g, int64_t o, int64_t t, float *d_rows, void *stream);

/* Host only (no device is touched): the float64 block algebra of the fit, exposed so that it can be checked on its own.
 * a is a symmetric positive definite n x n matrix, row-major.  evals [n] receives its eigenvalues in descending order and
 * evecs [n][n] the eigenvectors as columns (cyclic Jacobi); rinv [n][n] the inverse of the upper Cholesky factor R,
 * a = R^T R.  n <= SDFA_PCA_MAX_BLOCK.  A matrix that is not positive definite is SDFA_EINVAL. */
int sdfa_pca_host_algebra(const double *a, int64_t n, double *evals, double *evecs, double *rinv);

#ifdef __cplusplus
}
#endif
#endif
