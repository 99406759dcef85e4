// Launchers of the PCA-fit kernels (pcafit.hip) for the host driver (api_pca.cpp).  Every launcher only enqueues.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Column selector of interleaved rows: selected column d is row column (d / t) * g + o + d % t.
struct PcaSel {
    int64_t W;
    int g, o, t;
};

// out[s][m][j] = sum over k in slab s of A(m, k) * B[k][j], j < nb <= 256, slab s = rows [s * slab_k, (s + 1) * slab_k) of K,
// written at out + s * slab_stride with row stride ldo.  A(m, k) is a(m, k), or a(k, m) when `trans`.
// sel form: a(r, d) = x[r * W + sel(d)] - mu[d].  plain form: a(r, c) = x[r * lda + c].
void pca_mm_sel(bool trans, const float *x, PcaSel sel, const float *mu, int64_t M, int64_t K, const float *B, int64_t ldb, int nb,
                float *out, int64_t ldo, int64_t slab_k, int64_t slab_stride, hipStream_t st);
void pca_mm_plain(bool trans, const float *x, int64_t lda, int64_t M, int64_t K, const float *B, int64_t ldb, int nb, float *out,
                  int64_t ldo, int64_t slab_k, int64_t slab_stride, hipStream_t st);
// out[i] = sum_s part[s * n + i], s ascending, in double, rounded once.
void pca_reduce_f32(const float *part, int64_t nslab, int64_t n, float *out, hipStream_t st);

// part[s][d] = sum over the rows of slab s of x[r][sel(d)] (mu == nullptr) or of (x[r][sel(d)] - mu[d])^2, in double.
void pca_moment_slabs(const float *x, PcaSel sel, const float *mu, int64_t F, int64_t D, double *part, hipStream_t st);
// out64[i] = sum_s part[s * n + i]; out32[i] = float(out64[i] / div) where out32 is not null.
void pca_reduce_f64(const double *part, int64_t nslab, int64_t n, double *out64, float *out32, double div, hipStream_t st);

// dst[d][j] (row stride b) = src[d][j] (row stride b_src) for j < b_src, the start hash u(seed, d, j) beyond.
void pca_start_block(const float *src, int b_src, float *dst, int b, int64_t D, uint64_t seed, hipStream_t st);
// part[s][j] = sum over the rows d of slab s of (Y[d][j] - lam[j] * Q[d][j])^2, in double.
void pca_residual_slabs(const float *Y, const float *Q, const float *lam, int64_t D, int b, double *part, hipStream_t st);
// comp[i][d] = sign_i * Q[d][i], i < k, sign_i making the entry of largest magnitude (first index on ties) positive.
void pca_finish(const float *Q, int b, int64_t D, int k, float *comp, hipStream_t st);
// rows[r][sel(d)] = mu[d] + sum_i coef[r][i] * comp[i][d].
void pca_expand(const float *coef, int64_t F, int k, const float *mu, const float *comp, int64_t D, PcaSel sel, float *rows, hipStream_t st);
