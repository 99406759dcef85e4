// Training step of the conv stack (include/sdfa_convtrain.h): three weight-normed convolutions along
// frequency, each with LeakyReLU(0.2) and an inference-form BatchNorm behind it and a max-pool of two behind the first two, and
// backwards from dC to the 15 parameter gradients.
//
// Every buffer is [g = F column + f][channel], so a conv tap is a row shift and its zero padding a test of g mod F, as the step
// shift of lstm_train_rec.h's PrevH is.  Every product is the tile routine of tile_acc.h.  A forward layer is one chain over
// (tap, ci) per output, tap outermost; its epilogue adds the bias, keeps a, applies lrelu and the BatchNorm and pools the row pairs,
// which a lane holds in neighbouring accumulator registers.  A layer's dX is the transposed chain over (tap, co); its epilogue is
// the backward of the layer BELOW's pool, BatchNorm and lrelu: it reads that layer's kept a, decides winner and kink side again
// with act_bn() on the same operands, and leaves da in a's place.  Everything summed over the columns is split into row blocks of
// CT_BLOCK_FRAMES frames, written as float32 partials in the flat parameter layout and added in ascending block order by the
// reduce launch.  Every offset is formed in 64 bits.  No kernel uses atomics or waits for another workgroup.
#include "common.h"
#include "convtrain.h"
#include "lstm_train_rec.h"
#include "tile_acc.h"

namespace {

using namespace sdfa_tile;
using sdfa_rec::Ones;

template <int CI_, int CO_, int KF_, int F_, int64_t OFF, int KOFF>
struct Layer {
    static constexpr int CI = CI_, CO = CO_, KF = KF_, F = F_, K = CI_ * KF_;
    static constexpr int64_t og = OFF, ov = og + CO, ob = ov + (int64_t)CO * K, ogam = ob + CO, obet = ogam + CO;
    static constexpr int cm = KOFF, cv = KOFF + CO;
    static_assert((F & (F - 1)) == 0 && F >= 2, "a row's bin is its low bits; a pooled pair lies in one column");
};
using L1 = Layer<CT_C0, CT_C1, CT_KF1, CT_F1, CT_OFF1, CT_CONST1>;
using L3 = Layer<CT_C1, CT_C3, CT_KF3, CT_F3, CT_OFF3, CT_CONST3>;
using L5 = Layer<CT_C3, CT_C5, CT_KF5, CT_F5, CT_OFF5, CT_CONST5>;
static_assert(L5::obet + L5::CO == CT_NUMEL && L5::cv + L5::CO == CT_CONSTS, "layout");

// ---------------------------------------------------------------------------------------------------- lrelu and BatchNorm
// One function for the forward and for the backward's decisions: explicit operations, nothing the compiler may contract one way
// here and another way there.
struct Bn {
    float s, t, mean, rstd;
};

template <class L>
__device__ __forceinline__ Bn bn_of(const float *P, const float *K, int co) {
    Bn b;
    b.rstd = 1.0f / sqrtf(fadd_exact(K[L::cv + co], SDFA_CONVTRAIN_BN_EPS));
    b.s = fmul_exact(P[L::ogam + co], b.rstd);
    b.mean = K[L::cm + co];
    b.t = fmaf(-b.mean, b.s, P[L::obet + co]);
    return b;
}

__device__ __forceinline__ float lrelu_t(float a) { return a >= 0.f ? a : fmul_exact(0.2f, a); }
__device__ __forceinline__ float act_bn(float a, const Bn &b) { return fmaf(lrelu_t(a), b.s, b.t); }

// dz at a position whose pre-activation is a -> da and dz (y - mean) rstd
__device__ __forceinline__ void through(float dz, float a, const Bn &b, float &da, float &q) {
    da = fmul_exact(fmul_exact(dz, b.s), a > 0.f ? 1.0f : 0.2f);
    q = fmul_exact(dz, fmul_exact(fadd_exact(lrelu_t(a), -b.mean), b.rstd));
}

// ---------------------------------------------------------------------------------------------------- operands of tile_acc
// (i, c = d CH + ch): channel ch of row g0 + i + sgn (d - KF / 2), zero outside the column's F rows.  sgn +1: the forward's taps;
// -1: the transposed ones of dX.
template <int CH, int KF, int F>
struct TapRows {
    static constexpr int NK = CH * KF;
    const float *p;
    int64_t g0, rows;
    int sgn;
    __device__ const float *at(int i, int c) const {
        const int cc = c < NK ? c : NK - 1, d = cc / CH, ch = cc - d * CH;
        int64_t r = g0 + i + sgn * (d - KF / 2);
        r = r < 0 ? 0 : r >= rows ? rows - 1 : r;
        return p + r * CH + ch;
    }
    __device__ float val(int i, int c, float v) const {
        if (c >= NK) return 0.f;
        const int f = (int)((g0 + i) & (F - 1)) + sgn * (c / CH - KF / 2);
        return f >= 0 && f < F ? v : 0.f;
    }
};

template <class L>
struct WFwd {                        // (j = co, c = d CI + ci): W[co][ci][d]
    const float *W;
    __device__ const float *at(int j, int c) const {
        const int cc = c < L::K ? c : L::K - 1, d = cc / L::CI, ci = cc - d * L::CI;
        return W + (j < L::CO ? j : L::CO - 1) * L::K + ci * L::KF + d;
    }
    __device__ float val(int j, int c, float v) const { return j < L::CO && c < L::K ? v : 0.f; }
};

template <class L>
struct WBwd {                        // (j = ci, c = d CO + co): W[co][ci][d]
    static constexpr int NK = L::KF * L::CO;
    const float *W;
    __device__ const float *at(int j, int c) const {
        const int cc = c < NK ? c : NK - 1, d = cc / L::CO, co = cc - d * L::CO;
        return W + co * L::K + (j < L::CI ? j : L::CI - 1) * L::KF + d;
    }
    __device__ float val(int j, int c, float v) const { return j < L::CI && c < NK ? v : 0.f; }
};

struct Mat {                         // p[i si + c sc], i < ni, c < nc
    const float *p;
    int64_t si, sc;
    int ni, nc;
    __device__ const float *at(int i, int c) const { return p + (i < ni ? i : ni - 1) * si + (int64_t)(c < nc ? c : nc - 1) * sc; }
    __device__ float val(int i, int c, float v) const { return i < ni && c < nc ? v : 0.f; }
};

template <int CH, int F>
struct ShiftRows {                   // (j = channel, c): row row0 + c + shift of a [rows][CH] buffer, zero outside the column
    const float *p;
    int64_t row0, rows;
    int shift, nc;
    __device__ const float *at(int j, int c) const {
        int64_t r = row0 + (c < nc ? c : nc - 1) + shift;
        r = r < 0 ? 0 : r >= rows ? rows - 1 : r;
        return p + r * CH + (j < CH ? j : CH - 1);
    }
    __device__ float val(int j, int c, float v) const {
        const int f = (int)((row0 + c) & (F - 1)) + shift;
        return j < CH && c < nc && f >= 0 && f < F ? v : 0.f;
    }
};

// ---------------------------------------------------------------------------------------------------- forward layer
// grid: x = tile of 64 rows g
template <class L, bool POOL>
__device__ __forceinline__ void forward_layer(const CtArgs &a, const float *X, float *A, float *out) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t g0 = (int64_t)blockIdx.x * T, rows = a.N * CT_COLS * L::F;
    f32x16 acc;
    zero(acc);
    tile_acc<true, true>(acc, L::K, TapRows<L::CI, L::KF, L::F>{X, g0, rows, 1}, WFwd<L>{a.W + L::ov}, sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int co = 32 * (wave & 1) + l31;
    if (co >= L::CO) return;
    const float bias = a.P[L::ob + co];
    const Bn bn = bn_of<L>(a.P, a.K, co);
    const int64_t r0 = g0 + 32 * (wave >> 1) + 4 * h;
    if (POOL) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const int64_t g = r0 + tile_row(r, 0);         // even: the pair (g, g + 1) pools to row g / 2
            const float a0 = fadd_exact(acc[r], bias), a1 = fadd_exact(acc[r + 1], bias);
            A[g * L::CO + co] = a0;
            A[(g + 1) * L::CO + co] = a1;
            const float z0 = act_bn(a0, bn), z1 = act_bn(a1, bn);
            out[(g >> 1) * L::CO + co] = z1 > z0 ? z1 : z0;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t g = r0 + tile_row(r, 0);
            const float v = fadd_exact(acc[r], bias);
            A[g * L::CO + co] = v;
            out[g * L::CO + co] = act_bn(v, bn);
        }
    }
}

__global__ __launch_bounds__(THREADS) void convtrain_forward1_kernel(CtArgs a) { forward_layer<L1, true>(a, a.feat, a.a1, a.p1); }
__global__ __launch_bounds__(THREADS) void convtrain_forward3_kernel(CtArgs a) { forward_layer<L3, true>(a, a.p1, a.a3, a.p3); }
__global__ __launch_bounds__(THREADS) void convtrain_forward5_kernel(CtArgs a) { forward_layer<L5, false>(a, a.p3, a.a5, a.C); }

// ---------------------------------------------------------------------------------------------------- backward
// layer 5 has no pool: every position is its own winner.  An element per thread.
__global__ __launch_bounds__(256) void convtrain_da5_kernel(CtArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;         // < 64 N * 32 * 64, whole blocks
    const Bn bn = bn_of<L5>(a.P, a.K, (int)(e & (L5::CO - 1)));
    float da, q;
    through(a.dC[e], a.a5[e], bn, da, q);
    a.a5[e] = da;
    a.q5[e] = q;
}

// dX of layer L, which is dp of the layer below, LP_; then through that layer's pool, BatchNorm and lrelu.  grid: x = tile of 64
// rows of dX
template <class L, class LP_>
__device__ __forceinline__ void dx_layer(const CtArgs &a, const float *da, float *Ap, float *dp, float *q) {
    static_assert(L::CI == LP_::CO && LP_::F == 2 * L::F, "the layer below, pooled");
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t g0 = (int64_t)blockIdx.x * T, rows = a.N * CT_COLS * L::F;
    f32x16 acc;
    zero(acc);
    tile_acc<true, false>(acc, L::KF * L::CO, TapRows<L::CO, L::KF, L::F>{da, g0, rows, -1}, WBwd<L>{a.W + L::ov}, sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int c = 32 * (wave & 1) + l31;
    if (c >= L::CI) return;
    const Bn bn = bn_of<LP_>(a.P, a.K, c);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t g = g0 + 32 * (wave >> 1) + tile_row(r, h);
        float *pa = Ap + 2 * g * LP_::CO + c;
        const float a0 = pa[0], a1 = pa[LP_::CO];
        const bool second = act_bn(a1, bn) > act_bn(a0, bn);            // the forward's comparison on the forward's operands
        float dav, qv;
        through(acc[r], second ? a1 : a0, bn, dav, qv);
        pa[0] = second ? 0.f : dav;
        pa[LP_::CO] = second ? dav : 0.f;
        dp[g * LP_::CO + c] = acc[r];
        q[g * LP_::CO + c] = qv;
    }
}

__global__ __launch_bounds__(THREADS) void convtrain_dx5_kernel(CtArgs a) { dx_layer<L5, L3>(a, a.a5, a.a3, a.dp3, a.q3); }
__global__ __launch_bounds__(THREADS) void convtrain_dx3_kernel(CtArgs a) { dx_layer<L3, L1>(a, a.a3, a.a1, a.dp1, a.q1); }

// ---------------------------------------------------------------------------------------------------- backward, the products
// A layer's tiles of a row block: dW per tap (co x ci), db, dbeta, dgamma (column 0 of a tile against ones).  FZ: rows per column
// of dz and q (the pooled positions).
template <class L, int FZ>
__device__ __forceinline__ void layer_tile(int tile, int64_t blk, const CtArgs &a, const float *da, const float *X, const float *dz,
                                           const float *q, float *sA, float *sB) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int rr = 32 * (wave >> 1) + 4 * h, cj = 32 * (wave & 1) + l31;     // this lane's first row and its column in a tile
    const int64_t R = a.N * CT_COLS, c0 = blk * CT_BLOCK_FRAMES * CT_COLS, cleft = R - c0;
    const int Cr = (int)(cleft < CT_BLOCK_FRAMES * CT_COLS ? cleft : CT_BLOCK_FRAMES * CT_COLS);      // the block's columns
    float *part = a.part + blk * CT_NUMEL;
    f32x16 acc;
    zero(acc);
    if (tile < L::KF) {
        // dW[co][ci][d] = sum_g da[g][co] X[g + d - KF / 2][ci]
        const int64_t g0 = c0 * L::F;
        tile_acc<false, false>(acc, Cr * L::F, Mat{da + g0 * L::CO, 1, L::CO, L::CO, Cr * L::F},
                               ShiftRows<L::CI, L::F>{X, g0, R * L::F, tile - L::KF / 2, Cr * L::F}, sA, sB);
        if (cj >= L::CI) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = rr + tile_row(r, 0);
            if (co < L::CO) part[L::ov + (int64_t)co * L::K + cj * L::KF + tile] = acc[r];
        }
        return;
    }
    tile -= L::KF;
    const float *src = tile == 0 ? da : tile == 1 ? dz : q;
    const int F = tile == 0 ? L::F : FZ;
    const int64_t g0 = c0 * F;
    tile_acc<false, false>(acc, Cr * F, Mat{src + g0 * L::CO, 1, L::CO, L::CO, Cr * F}, Ones{src, Cr * F}, sA, sB);
    if (cj != 0) return;
    float *out = part + (tile == 0 ? L::ob : tile == 1 ? L::obet : L::ogam);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = rr + tile_row(r, 0);
        if (co < L::CO) out[co] = acc[r];
    }
}

constexpr int N_T1 = L1::KF + 3, N_T3 = L3::KF + 3, N_T5 = L5::KF + 3, N_BLK = N_T1 + N_T3 + N_T5;

// grid: x = per row block: layer 1's tiles (the longest chains) | layer 3's | layer 5's
__global__ __launch_bounds__(THREADS) void convtrain_products_kernel(CtArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t blk = blockIdx.x / N_BLK;
    int tile = (int)(blockIdx.x % N_BLK);
    if (tile < N_T1) layer_tile<L1, L1::F / 2>(tile, blk, a, a.a1, a.feat, a.dp1, a.q1, sA, sB);
    else if ((tile -= N_T1) < N_T3) layer_tile<L3, L3::F / 2>(tile, blk, a, a.a3, a.p1, a.dp3, a.q3, sA, sB);
    else layer_tile<L5, L5::F>(tile - N_T3, blk, a, a.a5, a.p3, a.dC, a.q5, sA, sB);
}

// The row blocks' partials, ascending: sdfa_rec::reduce_partials' sum with a bound (11,168 is no multiple of 256) and two
// destinations.  v's slots are dW, which the weight-norm launch turns into dg and dv; g's slots hold nothing.
__global__ __launch_bounds__(256) void convtrain_reduce_kernel(CtArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= CT_NUMEL) return;
    const int64_t o = e >= CT_OFF5 ? e - CT_OFF5 : e >= CT_OFF3 ? e - CT_OFF3 : e;
    const int co = e >= CT_OFF3 ? CT_C3 : CT_C1, k = e >= CT_OFF5 ? CT_K5 : e >= CT_OFF3 ? CT_K3 : CT_K1;
    if (o < co) return;
    float s = 0.f;
    for (int b = 0; b < a.nblk; ++b) s = fadd_exact(s, a.part[(int64_t)b * CT_NUMEL + e]);
    (o < co + (int64_t)co * k ? a.dW : a.grad)[e] = s;
}

}  // namespace

hipError_t convtrain_forward(const CtArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(convtrain_forward1_kernel, dim3((unsigned)(a.N * CT_COLS * CT_F1 / T)), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(convtrain_forward3_kernel, dim3((unsigned)(a.N * CT_COLS * CT_F3 / T)), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(convtrain_forward5_kernel, dim3((unsigned)(a.N * CT_COLS * CT_F5 / T)), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t convtrain_backward(const CtArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(convtrain_da5_kernel, dim3((unsigned)(a.N * CT_COLS * CT_F5 * CT_C5 / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(convtrain_dx5_kernel, dim3((unsigned)(a.N * CT_COLS * CT_F5 / T)), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(convtrain_dx3_kernel, dim3((unsigned)(a.N * CT_COLS * CT_F3 / T)), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t convtrain_products(const CtArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(convtrain_products_kernel, dim3((unsigned)(a.nblk * N_BLK)), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t convtrain_reduce(const CtArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(convtrain_reduce_kernel, dim3((unsigned)((CT_NUMEL + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}
