// Training step of the Bahdanau attention layer (include/sdfa_attntrain.h): the query convolution and
// its projection, the per-frame scores, softmax and context, and the backward of all of it down to dH.
//
// Every matrix product is the tile routine of tile_acc.h (64 x 64 output tiles, four waves, v_mfma_f32_32x32x2_f32, the
// contraction ascending through one accumulator chain).  An operand here is Op: element (i, c) at p + f(i) si + g(c) sc, clamped for
// the fetch and zeroed past its bounds when it goes to LDS.  f and g are the identity or one of two index maps that let the conv
// weight Wc [512 o][512 c][3 k] and the query window H[n][31 .. 33][:] be read where they lie:
//     map 1: j = k 512 + c  ->  c 3 + k   (a window-ordered index into a row of Wc)
//     map 2: j = c 3 + k    ->  k 512 + c (a Wc-ordered index into the window of H)
// so qc and dHq contract / are written in window order (contiguous in H and dH) and dWc is written in Wc's own order.
//
// "Rows" are the 64 N pairs (n, t).  One frame is exactly one 64-row tile, so the frame kernels own a frame per workgroup and a
// frame's z, align and dH never see another frame.  dWk = dpre^T H contracts over all rows: it is split into row blocks of
// AT_BLOCK_FRAMES frames, each block's 16 tiles written as float32 partials and added in ascending block order by the reduce
// launch; dv and db go the same way.  No kernel uses atomics or waits for another workgroup.
#include "common.h"
#include "attntrain.h"
#include "tile_acc.h"

#include <math.h>

namespace {

using namespace sdfa_tile;
constexpr int TS = AT_T, D = AT_D, NA = AT_A, KW = AT_KW, QW = AT_KW * AT_D;
constexpr int64_t FRAME = (int64_t)TS * D;
constexpr int UP = NA + 1;                                   // LDS row stride of a frame's u
static_assert(TS == T && D % T == 0 && NA % T == 0 && TS * UP <= 2 * CH * LP, "one frame is one row tile");

template <int M>
__device__ __forceinline__ int64_t imap(int64_t x) {
    if (M == 1) return (x & (D - 1)) * KW + (x >> 9);
    if (M == 2) return (x % KW) * D + x / KW;
    return x;
}
static_assert(D == 512, "map 1 shifts by 9");

template <int MI, int MC>
struct Op {
    const float *p;
    int64_t si, sc, i0, ni;
    int nc;
    __device__ const float *at(int i, int c) const {
        const int64_t ii = i0 + i < ni ? i0 + i : ni - 1;
        const int64_t cc = c < nc ? c : nc - 1;
        return p + imap<MI>(ii) * si + imap<MC>(cc) * sc;
    }
    __device__ float val(int i, int c, float v) const { return i0 + i < ni && c < nc ? v : 0.f; }
};

template <int MI, int MC>
__device__ __forceinline__ Op<MI, MC> op_of(const AtOp &o, int64_t i0) {
    return Op<MI, MC>{o.p, o.si, o.sc, i0, o.ni, o.nc};
}

// ---------------------------------------------------------------------------------------------------- the small products
// out[i][j] = sum_c A(i, c) B(j, c); A's contraction index is contiguous.  grid: x = tile along j, y = tile along i
template <int MI, int MC, bool BMIN>
__global__ __launch_bounds__(THREADS) void attntrain_product_kernel(AtProdArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t i0 = (int64_t)blockIdx.y * T;
    const int j0 = blockIdx.x * T;
    f32x16 acc;
    zero(acc);
    tile_acc<true, BMIN>(acc, a.A.nc, op_of<0, 0>(a.A, i0), op_of<MI, MC>(a.B, j0), sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int64_t j = j0 + 32 * (wave & 1) + l31;
    if (j >= a.B.ni) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t i = i0 + 32 * (wave >> 1) + tile_row(r, h);
        if (i < a.A.ni) a.out[i * a.ldo + j] = acc[r];
    }
}

// ---------------------------------------------------------------------------------------------------- forward, a frame per workgroup
// u = tanhf((H Wk^T + qp) + b) through two column tiles; s_t = sum_m v[m] u[t][m], m ascending in one fma chain; the plain
// two-pass softmax over the 64 steps in one wave; z[c] = sum_t a_t H[t][c], t ascending in one fma chain.
__global__ __launch_bounds__(THREADS) void attntrain_frame_forward_kernel(AtFwdArgs a) {
    __shared__ float smem[2 * CH * LP];
    __shared__ float sal[TS];
    float *sA = smem, *sB = smem + CH * LP;
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const float *Hn = a.H + n * FRAME;
    const Op<0, 0> opA{Hn, D, 1, 0, TS, D};
    f32x16 acc[NA / T];
#pragma unroll
    for (int ct = 0; ct < NA / T; ++ct) {
        zero(acc[ct]);
        tile_acc<true, true>(acc[ct], D, opA, Op<0, 0>{a.Wk, D, 1, ct * T, NA, D}, sA, sB);
    }
    __syncthreads();                                        // the slabs become the frame's u
    float *un = a.u + n * TS * NA;
#pragma unroll
    for (int ct = 0; ct < NA / T; ++ct) {
        const int m = ct * T + 32 * (wave & 1) + l31;
        const float qp = a.qp[n * NA + m], b = a.b[m];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = 32 * (wave >> 1) + tile_row(r, h);
            const float u = tanhf(fadd_exact(fadd_exact(acc[ct][r], qp), b));
            un[t * NA + m] = u;
            smem[t * UP + m] = u;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
        for (int m = 0; m < NA; ++m) s = fmaf(a.v[m], smem[lane * UP + m], s);
        float mx = s;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) mx = fmaxf(mx, __shfl_xor(mx, k, 64));
        const float e = expf(s - mx);
        const float al = e / wave_sum(e);
        sal[lane] = al;
        a.al[n * TS + lane] = al;
        a.align[n * TS + lane] = al;
    }
    __syncthreads();
#pragma unroll
    for (int c = tid; c < D; c += THREADS) {
        float z = 0.f;
        for (int t = 0; t < TS; ++t) z = fmaf(sal[t], Hn[t * D + c], z);
        a.z[n * D + c] = z;
    }
}

// ---------------------------------------------------------------------------------------------------- backward, a frame per workgroup
// da_t = dz . H[t] (a wave per step: lane-strided fma chains, then the fixed butterfly); ds_t = a_t (da_t - sum_j a_j da_j);
// dpre[t][m] = (ds_t v[m]) fma(-u, u, 1); the frame's shares dvp[m] = sum_t ds_t u[t][m] and dqp[m] = sum_t dpre[t][m]: each half
// of the steps ascending in one chain, then first half + second half.
__global__ __launch_bounds__(THREADS) void attntrain_frame_backward_kernel(AtFrameBwdArgs a) {
    __shared__ float sda[TS], sds[TS], shv[NA], shq[NA];
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *Hn = a.H + n * FRAME;
    float dz[D / 64];
#pragma unroll
    for (int i = 0; i < D / 64; ++i) dz[i] = a.dz[n * D + lane + 64 * i];
    for (int t = wave * (TS / 4); t < (wave + 1) * (TS / 4); ++t) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < D / 64; ++i) d = fmaf(dz[i], Hn[t * D + lane + 64 * i], d);
        d = wave_sum(d);
        if (lane == 0) sda[t] = d;
    }
    __syncthreads();
    if (wave == 0) {
        const float al = a.al[n * TS + lane], da = sda[lane];
        const float dot = wave_sum(al * da);
        sds[lane] = al * (da - dot);
    }
    __syncthreads();
    const int m = tid & (NA - 1), half = tid >> 7;
    const float vm = a.v[m];
    const float *un = a.u + n * TS * NA;
    float *dp = a.dpre + n * TS * NA;
    float av = 0.f, aq = 0.f;
    for (int t = half * (TS / 2); t < (half + 1) * (TS / 2); ++t) {
        const float u = un[t * NA + m], ds = sds[t];
        const float d = fmul_exact(fmul_exact(ds, vm), fmaf(-u, u, 1.0f));
        dp[t * NA + m] = d;
        av = fmaf(ds, u, av);
        aq = fadd_exact(aq, d);
    }
    if (half == 1) {
        shv[m] = av;
        shq[m] = aq;
    }
    __syncthreads();
    if (half == 0) {
        a.dvp[n * NA + m] = fadd_exact(av, shv[m]);
        a.dqp[n * NA + m] = fadd_exact(aq, shq[m]);
    }
}

// ---------------------------------------------------------------------------------------------------- backward, the products
// grid: x = [dWc tiles 8 x 24 | dWq tiles 2 x 8 | per row block: dWk partial tiles 2 x 8 | per row block: dv, db partials | dH tiles]
constexpr int N_DWC = (D / T) * (QW / T), N_DWQ = (NA / T) * (D / T), N_DWK = (NA / T) * (D / T);

__global__ __launch_bounds__(THREADS) void attntrain_backward_kernel(AtBwdArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int64_t N = a.N;
    int64_t bid = blockIdx.x;
    const int rr = 32 * (wave >> 1) + 4 * h, cj = 32 * (wave & 1) + l31;     // this lane's first row and its column in a tile
    f32x16 acc;
    zero(acc);
    if (bid < N_DWC) {
        // dWc[o][c 3 + k] = sum_n dqc[n][o] H[n][31 + k][c]
        const int o0 = (int)(bid / (QW / T)) * T, j0 = (int)(bid % (QW / T)) * T;
        tile_acc<false, false>(acc, (int)N, Op<0, 0>{a.dqc, 1, D, o0, D, (int)N}, Op<2, 0>{a.H + AT_W0 * D, 1, FRAME, j0, QW, (int)N}, sA, sB);
#pragma unroll
        for (int r = 0; r < 16; ++r) a.gWc[(int64_t)(o0 + rr + tile_row(r, 0)) * QW + j0 + cj] = acc[r];
        return;
    }
    bid -= N_DWC;
    if (bid < N_DWQ + (int64_t)a.nblk * N_DWK) {
        // dWq[m][o] = sum_n dqp[n][m] qc[n][o];   a row block's share of dWk[m][c] = sum_rows dpre[row][m] H[row][c]
        const bool q = bid < N_DWQ;
        if (!q) bid -= N_DWQ;
        const int64_t blk = q ? 0 : bid / N_DWK;
        const int tile = (int)(bid % N_DWK);
        const int m0 = (tile / (D / T)) * T, c0 = (tile % (D / T)) * T;
        const int64_t r0 = blk * AT_BLOCK_FRAMES * TS, left = N * TS - r0;
        const int C = q ? (int)N : (int)(left < AT_BLOCK_FRAMES * TS ? left : AT_BLOCK_FRAMES * TS);
        const Op<0, 0> opA{q ? a.dqp : a.dpre + r0 * NA, 1, NA, m0, NA, C};
        const Op<0, 0> opB{q ? a.qc : a.H + r0 * D, 1, D, c0, D, C};
        tile_acc<false, false>(acc, C, opA, opB, sA, sB);
        float *out = q ? a.gWq : a.part + blk * NA * D;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(m0 + rr + tile_row(r, 0)) * D + c0 + cj] = acc[r];
        return;
    }
    bid -= N_DWQ + (int64_t)a.nblk * N_DWK;
    if (bid < a.nblk) {
        // a row block's share of dv (threads 0 .. 127) and db (128 .. 255): its frames' shares, ascending
        const float *src = tid < NA ? a.dvp : a.dqp;
        const int m = tid & (NA - 1);
        const int64_t f0 = bid * AT_BLOCK_FRAMES, f1 = f0 + AT_BLOCK_FRAMES < N ? f0 + AT_BLOCK_FRAMES : N;
        float s = 0.f;
        for (int64_t f = f0; f < f1; ++f) s = fadd_exact(s, src[f * NA + m]);
        a.partv[bid * 2 * NA + tid] = s;
        return;
    }
    bid -= a.nblk;
    // dH[n][t][c] = fma(a_t, dz[c], sum_m dpre[t][m] Wk[m][c]), + dHq[n][t - 31][c] for t = 31, 32, 33
    const int64_t n = bid / (D / T);
    const int c0 = (int)(bid % (D / T)) * T;
    tile_acc<true, false>(acc, NA, Op<0, 0>{a.dpre + n * TS * NA, NA, 1, 0, TS, NA}, Op<0, 0>{a.Wk, 1, D, c0, D, NA}, sA, sB);
    const int c = c0 + cj;
    const float dz = a.dz[n * D + c];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = rr + tile_row(r, 0);
        float v = fmaf(a.al[n * TS + t], dz, acc[r]);
        if (t >= AT_W0 && t < AT_W0 + KW) v = fadd_exact(v, a.dHq[n * QW + (t - AT_W0) * D + c]);
        a.dH[(n * TS + t) * D + c] = v;
    }
}

// dWk, dv, db: the row blocks' partials, ascending.  An element per thread.
__global__ __launch_bounds__(256) void attntrain_reduce_kernel(AtReduceArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const bool k = e < NA * D;
    const float *src = k ? a.part + e : a.partv + (e - NA * D);
    const int stride = k ? NA * D : 2 * NA;
    float s = 0.f;
    for (int b = 0; b < a.nblk; ++b) s = fadd_exact(s, src[(int64_t)b * stride]);
    if (k) a.gWk[e] = s;
    else if (e - NA * D < NA) a.gv[e - NA * D] = s;
    else a.gb[e - NA * D - NA] = s;
}

}  // namespace

hipError_t attntrain_product(int which, const AtProdArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.B.ni + T - 1) / T), (unsigned)((a.A.ni + T - 1) / T));
    if (which == AT_PROD_QC) hipLaunchKernelGGL((attntrain_product_kernel<0, 1, true>), grid, dim3(THREADS), 0, st, a);
    else if (which == AT_PROD_QP) hipLaunchKernelGGL((attntrain_product_kernel<0, 0, true>), grid, dim3(THREADS), 0, st, a);
    else if (which == AT_PROD_DQC) hipLaunchKernelGGL((attntrain_product_kernel<0, 0, false>), grid, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((attntrain_product_kernel<1, 0, false>), grid, dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t attntrain_frame_forward(const AtFwdArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(attntrain_frame_forward_kernel, dim3((unsigned)a.N), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t attntrain_frame_backward(const AtFrameBwdArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(attntrain_frame_backward_kernel, dim3((unsigned)a.N), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t attntrain_backward(const AtBwdArgs &a, hipStream_t st) {
    int64_t blocks = N_DWC + N_DWQ + (int64_t)a.nblk * (N_DWK + 1);
    if (a.dH) blocks += a.N * (D / T);
    hipLaunchKernelGGL(attntrain_backward_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t attntrain_reduce(const AtReduceArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(attntrain_reduce_kernel, dim3((NA * D + 2 * NA) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
