// Kernels of the PCA fit (include/sdfa_pca.h): the device side of a blocked subspace iteration on
// float32 rows that stay where they are.  The host driver is api_pca.cpp.
//
// One matrix kernel carries every product, pca_mm_kernel<Op, TRANS>, on v_mfma_f32_32x32x2_f32 (exact fp32):
//     out[s][m][j] = sum over k in slab s of A(m, k) * B[k][j]         j < nb <= 256
//   TRANS = false, "rows x small":   A(m, k) = op(m, k).  Z = Xc Q and transform (SelOp); Q <- Y M (PlainOp).  One slab.
//   TRANS = true,  "tall^T x tall":  A(m, k) = op(k, m), k over rows in slabs of SDFA_PCA_SLAB whose partial products go
//                                    to workspace and are added in slab order by pca_reduce_f32_kernel.  Y = Xc^T Z
//                                    (SelOp); the b x b Grams (PlainOp).
// The operand policy is the only place that knows how an element is addressed: SelOp reads column (d / t) * g + o + d % t
// of an interleaved row and subtracts the column's mean in fp32 as the element is loaded, PlainOp reads a dense matrix.
// Both feed the same loop in the same order, so a fit through a selector equals the fit of a contiguous copy bit for bit.
//
// A workgroup of four waves owns 128 rows of `out` (four 32-row tiles) and all nb columns; wave w owns column tiles w and
// w + 4, so 4 x 2 accumulators of 16 registers (two workgroups per CU: __launch_bounds__(256, 2)).  Per 32-deep k step the A tile (32 x 128) and the B tile (32 x nb) are
// staged in LDS; every tail (M, K, nb, the slab's end) is zero-filled there and masked at the store.  No workgroup waits on
// another and nothing is atomic.
#include "common.h"
#include "pcafit.h"
#include "../../include/sdfa_pca.h"

namespace {

constexpr int MT = 4;                    // 32-row tiles of `out` per workgroup
constexpr int BM = 32 * MT;              // rows of `out` per workgroup
constexpr int BK = 32;                   // k step
constexpr int LDA = BM + 1;              // As[k][m]: +1 so that the k-contiguous fill (TRANS = false) spreads over banks
constexpr int LDB = 256 + 1;
constexpr int SLAB = SDFA_PCA_SLAB;

struct SelOp {
    const float *x;
    const float *mu;
    int64_t W;
    int g, o, t;
    __device__ __forceinline__ float at(int64_t r, int64_t d) const {
        const unsigned q = (unsigned)d / (unsigned)t, rem = (unsigned)d - q * (unsigned)t;
        return x[r * W + (int64_t)q * g + o + rem] - mu[d];
    }
};

struct PlainOp {
    const float *x;
    int64_t ld;
    __device__ __forceinline__ float at(int64_t r, int64_t c) const { return x[r * ld + c]; }
};

template <class Op, bool TRANS>
__global__ __launch_bounds__(256, 2) void pca_mm_kernel(Op op, int64_t M, int64_t K, const float *__restrict__ B, int64_t ldb, int nb,
                                                        float *__restrict__ out, int64_t ldo, int64_t slab_k, int64_t slab_stride) {
    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * LDB];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, h = l >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int64_t k_begin = (int64_t)blockIdx.y * slab_k;
    const int64_t k_end = k_begin + slab_k < K ? k_begin + slab_k : K;
    const int nct = (nb + 31) >> 5;

    f32x16 acc[MT][2];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

    for (int64_t k0 = k_begin; k0 < k_end; k0 += BK) {
        if (TRANS) {                         // op(row = k, column = m): contiguous along m
#pragma unroll
            for (int it = 0; it < BK * BM / 256; ++it) {
                const int e = tid + 256 * it, m = e % BM, k = e / BM;
                As[k * LDA + m] = (m0 + m < M && k0 + k < k_end) ? op.at(k0 + k, m0 + m) : 0.f;
            }
        } else {                             // op(row = m, column = k): contiguous along k
#pragma unroll
            for (int it = 0; it < BK * BM / 256; ++it) {
                const int e = tid + 256 * it, k = e % BK, m = e / BK;
                As[k * LDA + m] = (m0 + m < M && k0 + k < k_end) ? op.at(m0 + m, k0 + k) : 0.f;
            }
        }
        for (int e = tid; e < BK * 256; e += 256) {
            const int k = e >> 8, c = e & 255;
            if (c < nct * 32) Bs[k * LDB + c] = (k0 + k < k_end && c < nb) ? B[(k0 + k) * ldb + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < BK / 2; ++s) {
            const int kk = 2 * s + h;
            float av[MT];
#pragma unroll
            for (int a = 0; a < MT; ++a) av[a] = As[kk * LDA + 32 * a + i];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int ct = w + 4 * c;
                if (ct < nct) {              // wave-uniform
                    const float bv = Bs[kk * LDB + 32 * ct + i];
#pragma unroll
                    for (int a = 0; a < MT; ++a) acc[a][c] = MFMA(av[a], bv, acc[a][c]);
                }
            }
        }
        __syncthreads();
    }

    float *o = out + (int64_t)blockIdx.y * slab_stride;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = 32 * (w + 4 * c) + i;
        if (col >= nb) continue;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < M) o[row * ldo + col] = acc[a][c][r];
            }
    }
}

__global__ __launch_bounds__(256) void pca_reduce_f32_kernel(const float *__restrict__ part, int64_t nslab, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t k = 0; k < nslab; ++k) s += (double)part[k * n + i];
    out[i] = (float)s;
}

__global__ __launch_bounds__(256) void pca_reduce_f64_kernel(const double *__restrict__ part, int64_t nslab, int64_t n, double *__restrict__ out64,
                                                             float *__restrict__ out32, double div) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t k = 0; k < nslab; ++k) s += part[k * n + i];
    out64[i] = s;
    if (out32) out32[i] = (float)(s / div);
}

// One thread per selected column, one workgroup row per slab of rows: the column's sum, or its centred sum of squares.
template <bool SQ>
__global__ __launch_bounds__(256) void pca_moment_kernel(const float *__restrict__ x, const float *__restrict__ mu, int64_t W, int g, int o, int t,
                                                         int64_t F, int64_t D, double *__restrict__ part) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const unsigned q = (unsigned)d / (unsigned)t, rem = (unsigned)d - q * (unsigned)t;
    const int64_t col = (int64_t)q * g + o + rem;
    const int64_t r0 = (int64_t)blockIdx.y * SLAB, r1 = r0 + SLAB < F ? r0 + SLAB : F;
    const float m = SQ ? mu[d] : 0.f;
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const float v = x[r * W + col];
        if (SQ) {
            const double c = (double)(v - m);
            s += c * c;
        } else {
            s += (double)v;
        }
    }
    part[(int64_t)blockIdx.y * D + d] = s;
}

__device__ __forceinline__ float start_value(uint64_t seed, int64_t d, int j) {
    uint32_t hsh = ((uint32_t)seed ^ (uint32_t)(seed >> 32)) * 0x9E3779B1u ^ (uint32_t)(d + 1) * 0x85EBCA77u ^ (uint32_t)(j + 1) * 0xC2B2AE3Du;
    hsh ^= hsh >> 16;
    hsh *= 0x85EBCA6Bu;
    hsh ^= hsh >> 13;
    hsh *= 0xC2B2AE35u;
    hsh ^= hsh >> 16;
    return (float)(hsh >> 8) * (1.0f / 8388608.0f) - 1.0f;
}

__global__ __launch_bounds__(256) void pca_start_kernel(const float *__restrict__ src, int b_src, float *__restrict__ dst, int b, int64_t D, uint64_t seed) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= D * b) return;
    const int64_t d = e / b;
    const int j = (int)(e - d * b);
    dst[e] = j < b_src ? src[d * b_src + j] : start_value(seed, d, j);
}

__global__ __launch_bounds__(256) void pca_residual_kernel(const float *__restrict__ Y, const float *__restrict__ Q, const float *__restrict__ lam, int64_t D,
                                                           int b, double *__restrict__ part) {
    const int j = threadIdx.x;
    if (j >= b) return;
    const int64_t d0 = (int64_t)blockIdx.x * SLAB, d1 = d0 + SLAB < D ? d0 + SLAB : D;
    const float lj = lam[j];
    double s = 0.0;
    for (int64_t d = d0; d < d1; ++d) {
        const double e = (double)(Y[d * b + j] - lj * Q[d * b + j]);
        s += e * e;
    }
    part[(int64_t)blockIdx.x * b + j] = s;
}

// One workgroup per component: the entry of largest magnitude, the smallest index among equals (a maximum with that rule
// does not depend on the order of the comparisons), then the signed, transposed copy.
__global__ __launch_bounds__(256) void pca_finish_kernel(const float *__restrict__ Q, int b, int64_t D, float *__restrict__ comp) {
    __shared__ float s_abs[256];
    __shared__ int64_t s_idx[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    float best = -1.f;
    int64_t at = 0;
    for (int64_t d = tid; d < D; d += 256) {
        const float a = fabsf(Q[d * b + i]);
        if (a > best) { best = a; at = d; }
    }
    s_abs[tid] = best;
    s_idx[tid] = at;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) {
            const float a = s_abs[tid + n];
            const int64_t ia = s_idx[tid + n];
            if (a > s_abs[tid] || (a == s_abs[tid] && ia < s_idx[tid])) { s_abs[tid] = a; s_idx[tid] = ia; }
        }
        __syncthreads();
    }
    const float sign = Q[s_idx[0] * b + i] < 0.f ? -1.f : 1.f;
    for (int64_t d = tid; d < D; d += 256) comp[(int64_t)i * D + d] = sign * Q[d * b + i];
}

__global__ __launch_bounds__(256) void pca_expand_kernel(const float *__restrict__ coef, int k, const float *__restrict__ mu, const float *__restrict__ comp,
                                                         int64_t D, int64_t W, int g, int o, int t, float *__restrict__ rows) {
    __shared__ float cf[SDFA_PCA_MAX_BLOCK];
    const int64_t r = blockIdx.y;
    for (int i = threadIdx.x; i < k; i += 256) cf[i] = coef[r * k + i];
    __syncthreads();
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    float s = 0.f;
    for (int i = 0; i < k; ++i) s = fmaf(cf[i], comp[(int64_t)i * D + d], s);
    const unsigned q = (unsigned)d / (unsigned)t, rem = (unsigned)d - q * (unsigned)t;
    rows[r * W + (int64_t)q * g + o + rem] = s + mu[d];
}

template <class Op>
void launch_mm(bool trans, Op op, int64_t M, int64_t K, const float *B, int64_t ldb, int nb, float *out, int64_t ldo, int64_t slab_k,
               int64_t slab_stride, hipStream_t st) {
    if (M <= 0 || K <= 0 || nb <= 0) return;
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((K + slab_k - 1) / slab_k));
    if (trans) pca_mm_kernel<Op, true><<<grid, 256, 0, st>>>(op, M, K, B, ldb, nb, out, ldo, slab_k, slab_stride);
    else pca_mm_kernel<Op, false><<<grid, 256, 0, st>>>(op, M, K, B, ldb, nb, out, ldo, slab_k, slab_stride);
}

}  // namespace

void pca_mm_sel(bool trans, const float *x, PcaSel sel, const float *mu, int64_t M, int64_t K, const float *B, int64_t ldb, int nb,
                float *out, int64_t ldo, int64_t slab_k, int64_t slab_stride, hipStream_t st) {
    launch_mm(trans, SelOp{x, mu, sel.W, sel.g, sel.o, sel.t}, M, K, B, ldb, nb, out, ldo, slab_k, slab_stride, st);
}

void pca_mm_plain(bool trans, const float *x, int64_t lda, int64_t M, int64_t K, const float *B, int64_t ldb, int nb, float *out,
                  int64_t ldo, int64_t slab_k, int64_t slab_stride, hipStream_t st) {
    launch_mm(trans, PlainOp{x, lda}, M, K, B, ldb, nb, out, ldo, slab_k, slab_stride, st);
}

void pca_reduce_f32(const float *part, int64_t nslab, int64_t n, float *out, hipStream_t st) {
    if (n > 0) pca_reduce_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(part, nslab, n, out);
}

void pca_moment_slabs(const float *x, PcaSel sel, const float *mu, int64_t F, int64_t D, double *part, hipStream_t st) {
    const dim3 grid((unsigned)((D + 255) / 256), (unsigned)((F + SLAB - 1) / SLAB));
    if (mu) pca_moment_kernel<true><<<grid, 256, 0, st>>>(x, mu, sel.W, sel.g, sel.o, sel.t, F, D, part);
    else pca_moment_kernel<false><<<grid, 256, 0, st>>>(x, mu, sel.W, sel.g, sel.o, sel.t, F, D, part);
}

void pca_reduce_f64(const double *part, int64_t nslab, int64_t n, double *out64, float *out32, double div, hipStream_t st) {
    if (n > 0) pca_reduce_f64_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(part, nslab, n, out64, out32, div);
}

void pca_start_block(const float *src, int b_src, float *dst, int b, int64_t D, uint64_t seed, hipStream_t st) {
    pca_start_kernel<<<(unsigned)((D * b + 255) / 256), 256, 0, st>>>(src, b_src, dst, b, D, seed);
}

void pca_residual_slabs(const float *Y, const float *Q, const float *lam, int64_t D, int b, double *part, hipStream_t st) {
    pca_residual_kernel<<<(unsigned)((D + SLAB - 1) / SLAB), 256, 0, st>>>(Y, Q, lam, D, b, part);
}

void pca_finish(const float *Q, int b, int64_t D, int k, float *comp, hipStream_t st) {
    if (k > 0) pca_finish_kernel<<<(unsigned)k, 256, 0, st>>>(Q, b, D, comp);
}

void pca_expand(const float *coef, int64_t F, int k, const float *mu, const float *comp, int64_t D, PcaSel sel, float *rows, hipStream_t st) {
    if (F <= 0 || D <= 0) return;
    for (int64_t r0 = 0; r0 < F; r0 += 65535) {          // grid.y limit
        const int64_t n = F - r0 < 65535 ? F - r0 : 65535;
        const dim3 grid((unsigned)((D + 255) / 256), (unsigned)n);
        pca_expand_kernel<<<grid, 256, 0, st>>>(coef + r0 * k, k, mu, comp, D, sel.W, sel.g, sel.o, sel.t, rows + r0 * sel.W);
    }
}
