// Training step of the regressor head (include/sdfa_headtrain.h): the weight-norm fold, the forward
// layers, the backward layers, the backward through the weight norm and Adam.
//
// Every product -- a forward layer Y = X W^T, a layer's dX = dPre W and its dW = dPre^T X -- is the tile routine of tile_acc.h
// (64 x 64 output tiles, four waves, v_mfma_f32_32x32x2_f32, the contraction ascending through one accumulator chain).  The
// operands' val() does the bounds: zero rows past N, zero columns past P or K, the one-hot columns and the column of ones that
// turns db into one more column of dW are formed there and never exist in memory.
//
// No kernel uses atomics or waits for another workgroup.
#include "common.h"
#include "headtrain.h"
#include "tile_acc.h"

#include <math.h>

namespace {

using namespace sdfa_tile;
constexpr int NS = SDFA_HEADTRAIN_SPEAKERS;
static_assert(T == SDFA_HEADTRAIN_TILE, "tiling");

// ---------------------------------------------------------------------------------------------------- weight norm, forward
// A wave per row of every layer: ss = sum v^2 (lane-strided, then a fixed butterfly), inv = 1 / sqrt(ss), s = g inv, W = s v.
__device__ __forceinline__ int layer_of(const HtTable &t, int row) {
    int li = 0;
    for (int i = 1; i < t.nl; ++i)
        if (row >= t.l[i].row0) li = i;
    return li;
}

__global__ __launch_bounds__(THREADS) void headtrain_fold_kernel(HtTable t, const float *__restrict__ params, float *__restrict__ W,
                                                                 float *__restrict__ inv, float *__restrict__ sc) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (row >= t.rows) return;
    const HtLayer L = t.l[layer_of(t, row)];
    const int p = row - L.row0, K = L.K;
    const float *v = params + L.ov + (int64_t)p * K;
    float ss = 0.f;
    for (int k = lane; k < K; k += 64) ss = fmaf(v[k], v[k], ss);
    ss = wave_sum(ss);
    const float iv = 1.0f / sqrtf(ss);
    const float s = params[L.og + p] * iv;
    float *w = W + L.ow + (int64_t)p * K;
    for (int k = lane; k < K; k += 64) w[k] = s * v[k];
    if (lane == 0) {
        inv[row] = iv;
        sc[row] = s;
    }
}

// A wave per row: dg = <dW, v> inv, dv = s (dW - (dg inv) v), into the gradient buffer (the bias gradients are already there).
__global__ __launch_bounds__(THREADS) void headtrain_wnorm_backward_kernel(HtTable t, const float *__restrict__ params, const float *__restrict__ dW,
                                                                           const float *__restrict__ inv, const float *__restrict__ sc,
                                                                           float *__restrict__ grads) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (row >= t.rows) return;
    const HtLayer L = t.l[layer_of(t, row)];
    const int p = row - L.row0, K = L.K;
    const float *v = params + L.ov + (int64_t)p * K, *d = dW + L.ow + (int64_t)p * K;
    float dot = 0.f;
    for (int k = lane; k < K; k += 64) dot = fmaf(d[k], v[k], dot);
    dot = wave_sum(dot);
    const float iv = inv[row], s = sc[row];
    const float dg = dot * iv, c = dg * iv;
    float *gv = grads + L.ov + (int64_t)p * K;
    for (int k = lane; k < K; k += 64) gv[k] = s * (d[k] - c * v[k]);
    if (lane == 0) grads[L.og + p] = dg;
}

// ---------------------------------------------------------------------------------------------------- forward layer
// grid: x = tile along p (a branch with fewer tiles leaves the rest), y = row tile, z = branch
__global__ __launch_bounds__(THREADS) void headtrain_forward_kernel(HtFwdArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const HtFwdJob jb = a.b[blockIdx.z];
    const int p0 = blockIdx.x * T;
    if (p0 >= jb.P) return;
    const int64_t n0 = (int64_t)blockIdx.y * T, N = a.N;
    const bool keep = a.zcopy != nullptr && blockIdx.x == 0;
    struct {
        const HtFwdJob &jb;
        int64_t n0, N;
        float *zcopy;
        __device__ const float *at(int i, int c) const {
            const int64_t n = n0 + i < N ? n0 + i : N - 1;
            return jb.X + n * jb.ldx + (c < jb.Kin ? c : jb.Kin - 1);
        }
        __device__ float val(int i, int c, float v) const {
            const int64_t n = n0 + i;
            if (n >= N || c >= jb.Kin) return 0.f;
            if (zcopy) zcopy[n * SDFA_HEADTRAIN_Z + c] = v;
            return v;
        }
    } opA{jb, n0, N, keep ? a.zcopy : nullptr};
    struct {
        const HtFwdJob &jb;
        int p0;
        __device__ const float *at(int j, int c) const {
            const int p = p0 + j < jb.P ? p0 + j : jb.P - 1;
            return jb.W + (int64_t)p * jb.ldw + (c < jb.Kin ? c : jb.Kin - 1);
        }
        __device__ float val(int j, int c, float v) const { return p0 + j < jb.P && c < jb.Kin ? v : 0.f; }
    } opB{jb, p0};
    f32x16 acc;
    zero(acc);
    tile_acc<true, true>(acc, jb.Kin, opA, opB, sA, sB);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int p = p0 + 32 * (wave & 1) + l31;
    const float bias = p < jb.P ? jb.bias[p] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t n = n0 + 32 * (wave >> 1) + tile_row(r, h);
        if (n >= N) continue;
        const int64_t s = a.sid[n];
        const bool sok = s >= 0 && s < NS;
        if (keep && (wave & 1) == 0 && l31 == 0) a.sidcopy[n] = sok ? (int)s : -1;
        if (p >= jb.P) continue;
        float v = fadd_exact(acc[r], bias);
        if (jb.cond && sok) v = fadd_exact(v, jb.W[(int64_t)p * jb.ldw + jb.Kin + s]);
        if (jb.act == HT_ACT_LRELU) v = lrelu02(v);
        else if (jb.act == HT_ACT_TANH) v = tanhf(v);
        jb.Y[n * jb.ldy + p] = v;
    }
}

// ---------------------------------------------------------------------------------------------------- backward layer
__device__ __forceinline__ void dx_acc(f32x16 &acc, const HtBwdJob &jb, int64_t n0, int k0, int64_t N, float *sA, float *sB) {
    struct {
        const HtBwdJob &jb;
        int64_t n0, N;
        __device__ const float *at(int i, int c) const {
            const int64_t n = n0 + i < N ? n0 + i : N - 1;
            return jb.D + n * jb.ldd + (c < jb.P ? c : jb.P - 1);
        }
        __device__ float val(int i, int c, float v) const { return n0 + i < N && c < jb.P ? v : 0.f; }
    } opA{jb, n0, N};
    struct {
        const HtBwdJob &jb;
        int k0;
        __device__ const float *at(int j, int c) const { return jb.W + (int64_t)(c < jb.P ? c : jb.P - 1) * jb.K + k0 + j; }      // k0 + j < Kin always
        __device__ float val(int j, int c, float v) const { return c < jb.P ? v : 0.f; }
    } opB{jb, k0};
    tile_acc<true, false>(acc, jb.P, opA, opB, sA, sB);
}

// grid: x = [per row block: branch 0's dW tiles | branch 1's dW tiles] [dX tiles].  The dW tiles contract over a row block of up
// to HT_BLOCK_ROWS rows and run longest: they come first.  A batch of more than one row block leaves float32 partials, which the
// reduce launch adds in ascending block order: no accumulator chain is longer than a row block, whatever N.
__global__ __launch_bounds__(THREADS) void headtrain_backward_kernel(HtBwdArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int64_t N = a.N;
    int bid = blockIdx.x;
    const int ndw = a.b[0].ndw + (a.nb == 2 ? a.b[1].ndw : 0);
    f32x16 acc;
    zero(acc);
    if (bid < ndw * a.nblk) {
        // a row block's share of dW[p][k] = sum_n D[n][p] x[n][k]; x's columns Kin .. K - 1 are the one-hot, column K is 1: that
        // one is db.  Rows r0 .. r0 + C - 1; a batch of one row block is the whole contraction and goes to dW and db itself.
        const int blk = bid / ndw;
        bid -= blk * ndw;
        const int br = bid < a.b[0].ndw ? 0 : 1;
        const HtBwdJob jb = a.b[br];
        if (br) bid -= a.b[0].ndw;
        const int p0 = (bid / jb.tk) * T, k0 = (bid % jb.tk) * T;
        const int64_t r0 = (int64_t)blk * HT_BLOCK_ROWS;
        const int C = (int)(N - r0 < HT_BLOCK_ROWS ? N - r0 : HT_BLOCK_ROWS);
        struct {
            const HtBwdJob &jb;
            int p0, C;
            int64_t r0;
            __device__ const float *at(int i, int c) const {
                return jb.D + (r0 + (c < C ? c : C - 1)) * jb.ldd + (p0 + i < jb.P ? p0 + i : jb.P - 1);
            }
            __device__ float val(int i, int c, float v) const { return p0 + i < jb.P && c < C ? v : 0.f; }
        } opA{jb, p0, C, r0};
        struct {
            const HtBwdJob &jb;
            int k0, C;
            int64_t r0;
            const int *sid;
            __device__ const float *at(int j, int c) const {
                return jb.X + (r0 + (c < C ? c : C - 1)) * jb.ldx + (k0 + j < jb.Kin ? k0 + j : jb.Kin - 1);
            }
            __device__ float val(int j, int c, float v) const {
                const int k = k0 + j;
                if (c >= C || k > jb.K) return 0.f;
                if (k < jb.Kin) return v;
                if (k == jb.K) return 1.f;
                return sid[r0 + c] == k - jb.Kin ? 1.f : 0.f;     // the last tile along k only
            }
        } opB{jb, k0, C, r0, a.sid};
        tile_acc<false, false>(acc, C, opA, opB, sA, sB);
        float *dW = a.nblk == 1 ? jb.dW : jb.pW + blk * a.psw, *db = a.nblk == 1 ? jb.db : jb.pb + blk * a.psb;
        const int k = k0 + 32 * (wave & 1) + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = p0 + 32 * (wave >> 1) + tile_row(r, h);
            if (p >= jb.P) continue;
            if (k < jb.K) dW[(int64_t)p * jb.K + k] = acc[r];
            else if (k == jb.K) db[p] = acc[r];
        }
        return;
    }
    // dX[n][k] = sum_p D[n][p] W[p][k], k < Kin
    bid -= ndw * a.nblk;
    const int tiles = a.rowtiles * a.tkx;
    const int br = a.dx_mode == HT_DX_BRANCH ? bid / tiles : 0;
    bid -= br * tiles;
    const int64_t n0 = (int64_t)(bid / a.tkx) * T;
    const int k0 = (bid % a.tkx) * T;
    const HtBwdJob jb = a.b[br];
    dx_acc(acc, jb, n0, k0, N, sA, sB);
    if (a.dx_mode == HT_DX_MERGE) {                         // dh0: the scale branch's share plus the rotat branch's
        f32x16 acc1;
        zero(acc1);
        dx_acc(acc1, a.b[1], n0, k0, N, sA, sB);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fadd_exact(acc[r], acc1[r]);
    }
    const int k = k0 + 32 * (wave & 1) + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t n = n0 + 32 * (wave >> 1) + tile_row(r, h);
        if (n >= N) continue;
        float v = acc[r];
        if (a.dx_mode != HT_DX_PLAIN) {
            const float y = jb.Yprev[n * jb.ldp + k];
            if (a.act_prev == HT_ACT_LRELU) v = y > 0.f ? v : 0.2f * v;
            else if (a.act_prev == HT_ACT_TANH) v = v * fmaf(-y, y, 1.0f);
        }
        jb.Dprev[n * jb.ldp + k] = v;
    }
}

// dW and db of a batch of more than one row block: the row blocks' partials, ascending.  An element per thread.
__global__ __launch_bounds__(256) void headtrain_reduce_kernel(HtReduceArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.wnumel + a.t.rows) return;
    const bool w = e < a.wnumel;
    const float *src = w ? a.pW + e : a.pb + (e - a.wnumel);
    const int64_t stride = w ? a.wnumel : a.t.rows;
    float s = 0.f;
    for (int b = 0; b < a.nblk; ++b) s = fadd_exact(s, src[b * stride]);
    if (w) {
        a.dW[e] = s;
        return;
    }
    const int row = (int)(e - a.wnumel);
    const HtLayer L = a.t.l[layer_of(a.t, row)];
    a.grads[L.ob + row - L.row0] = s;
}

// ---------------------------------------------------------------------------------------------------- Adam
__global__ __launch_bounds__(256) void headtrain_adam_kernel(HtAdamArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float g = a.g[i];
    float m = a.m[i], v = a.v[i];
    m = m + (g - m) * a.omb1;
    v = a.beta2 * v + (a.omb2 * g) * g;
    const float denom = sqrtf(v) / a.bc2s + a.eps;
    a.m[i] = m;
    a.v[i] = v;
    a.p[i] = a.p[i] - a.step * (m / denom);
}

}  // namespace

hipError_t headtrain_fold(const HtTable &t, const float *params, float *W, float *inv, float *sc, hipStream_t st) {
    hipLaunchKernelGGL(headtrain_fold_kernel, dim3((unsigned)((t.rows + 3) / 4)), dim3(THREADS), 0, st, t, params, W, inv, sc);
    return hipGetLastError();
}

hipError_t headtrain_wnorm_backward(const HtTable &t, const float *params, const float *dW, const float *inv, const float *sc, float *grads, hipStream_t st) {
    hipLaunchKernelGGL(headtrain_wnorm_backward_kernel, dim3((unsigned)((t.rows + 3) / 4)), dim3(THREADS), 0, st, t, params, dW, inv, sc, grads);
    return hipGetLastError();
}

hipError_t headtrain_forward_layer(const HtFwdArgs &a, hipStream_t st) {
    int pmax = a.b[0].P;
    if (a.nb == 2 && a.b[1].P > pmax) pmax = a.b[1].P;
    const dim3 grid((unsigned)((pmax + T - 1) / T), (unsigned)((a.N + T - 1) / T), (unsigned)a.nb);
    hipLaunchKernelGGL(headtrain_forward_kernel, grid, dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t headtrain_backward_layer(const HtBwdArgs &a, hipStream_t st) {
    int64_t blocks = (int64_t)a.nblk * (a.b[0].ndw + (a.nb == 2 ? a.b[1].ndw : 0));
    if (a.dx_mode != HT_DX_NONE) blocks += (int64_t)a.rowtiles * a.tkx * (a.dx_mode == HT_DX_BRANCH ? a.nb : 1);
    hipLaunchKernelGGL(headtrain_backward_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t headtrain_reduce(const HtReduceArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(headtrain_reduce_kernel, dim3((unsigned)((a.wnumel + a.t.rows + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t headtrain_adam(const HtAdamArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(headtrain_adam_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}
