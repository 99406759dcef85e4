// Tail of the shared-column frequency projection.
//
// gemm_fat_kernel (gemm.hip) is persistent: G workgroups, one per CU, over the 256-column tiles b, b + G, ...  With column sharing
// the number of tiles T is whatever the chunk's distinct columns come to, and the T mod G tiles behind the last whole round cost
// a whole round's time (1.77 ms at K = 8192) on a chip that is mostly idle.  The numbering kernel (share.hip) therefore stops the
// fat kernel at the whole rounds (counts[2] = q_full) and this kernel multiplies the columns [q_full, counts[1]) behind them in
// 64 x 64 blocks: 16 work units per 256-column tile, four workgroups per CU, so a few dozen tiles spread over the whole chip.
//
// One case only: fp32, K4 output, bias per P row, P = 256 rows, Q in the tile-major hidden-state layout (float4[column block of
// 128][q_slab_rows][128]), K = 8192.  Bit-identical to the fat kernel: every accumulator starts at 0 and takes v_mfma_f32_32x32x2_f32
// over k in ascending order with the K4 pairing of common.h (half h of the wave holds k-quad 2 kb + h), then the bias is added --
// what every fp32 kernel of gemm.hip does per accumulator.  Staging is the plain form of gemm_k4_kernel: registers one stage ahead,
// double-buffered LDS, one barrier per 32-deep stage; with 16 waves on a CU the other workgroups' MFMAs cover a workgroup's waits.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TAIL_K = 8192, TAIL_ROWS = 256, KQ = 8, TB = 64;      // contraction, P rows, k-quads per stage, block edge

__global__ __launch_bounds__(256, 4) void gemm_tail_kernel(GemmTailArgs a) {
    __shared__ float4 sP[2][KQ][TB], sQ[2][KQ][TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave >> 1, wq = wave & 1, l31 = lane & 31, h = lane >> 5;
    // unit = (64-column block, row block): the four row blocks of a column block are dispatched together and share its Q stream in L2
    const int64_t q_lo = *a.q_lo, q_hi = std::min<int64_t>(*a.q_hi, a.ldd);
    const int64_t q0 = q_lo + (int64_t)(blockIdx.x >> 2) * TB;
    const int p0 = (blockIdx.x & 3) * TB;
    if (q_lo < 0 || q0 >= q_hi) return;      // surplus workgroup (the grid is sized for the largest tail), or an empty range

    const float4 *__restrict__ P = reinterpret_cast<const float4 *>(a.P) + p0;                                                      // k-quad rows TAIL_ROWS apart
    const float4 *__restrict__ Q = reinterpret_cast<const float4 *>(a.Q) + (q0 >> 7) * (int64_t)a.q_slab_rows * 128 + (q0 & 127);   // k-quad rows 128 apart
    const int r = tid >> 6, c = tid & 63;    // staging: a wave moves 64 consecutive columns (1 KiB) of k-quad rows r and r + 4
    constexpr int nstage = TAIL_K / 32;

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    float4 rp0, rp1, rq0, rq1;
#define TAIL_GLOAD(st)                                                                      \
    {                                                                                       \
        rp0 = P[((st) * KQ + r) * TAIL_ROWS + c]; rp1 = P[((st) * KQ + r + 4) * TAIL_ROWS + c]; \
        rq0 = Q[((st) * KQ + r) * 128 + c];       rq1 = Q[((st) * KQ + r + 4) * 128 + c];   \
    }
#define TAIL_LSTORE(buf) { sP[buf][r][c] = rp0; sP[buf][r + 4][c] = rp1; sQ[buf][r][c] = rq0; sQ[buf][r + 4][c] = rq1; }
    TAIL_GLOAD(0)
    TAIL_LSTORE(0)
    __syncthreads();
    for (int st = 0; st < nstage; ++st) {
        const int buf = st & 1;
        const bool more = st + 1 < nstage;
        if (more) TAIL_GLOAD(st + 1)
#pragma unroll
        for (int kb = 0; kb < KQ / 2; ++kb) {
            const float4 fa = sP[buf][2 * kb + h][wp * 32 + l31], fb = sQ[buf][2 * kb + h][wq * 32 + l31];
            mfma4(acc, fa, fb);
        }
        if (more) TAIL_LSTORE(buf ^ 1)      // the buffer stage st - 1 was read from: every wave passed the barrier behind it
        __syncthreads();
    }
#undef TAIL_GLOAD
#undef TAIL_LSTORE

    // epilogue as store_tile (gemm.hip): register quad g of the accumulator = rows p .. p + 3 of this lane's column
    const int64_t q = q0 + wq * 32 + l31;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int p = p0 + wp * 32 + 8 * g + 4 * h;
        float v[4] = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        const float4 b = ld4(a.bias + p);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
        st4(a.D + ((p / 4) * a.ldd + q) * 4, make_float4(v[0], v[1], v[2], v[3]));
    }
}

}  // namespace

hipError_t sdfa_launch_gemm_tail(const GemmTailArgs &a, hipStream_t s) {
    if (!a.P || !a.Q || !a.D || !a.bias || !a.q_lo || !a.q_hi || a.q_slab_rows < TAIL_K / 4 || a.ldd % 256) return hipErrorInvalidValue;
    if (a.max_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(gemm_tail_kernel, dim3((unsigned)a.max_tiles * 16), dim3(256), 0, s, a);
    return hipGetLastError();
}
