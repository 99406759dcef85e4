// The tile routine of the training kernels (headtrain.hip, attntrain.hip; DESIGN.md sections 16 and 17).
//
// Every product is the same routine: a workgroup of four waves owns a 64 x 64 output tile, wave (wi, wj) its 32 x 32 quarter, and
// walks the contraction in chunks of 64.  A chunk's two operand slabs lie in LDS as sA[c][i] and sB[c][j] (row stride 65:
// consecutive lanes read consecutive banks, and the stores of either thread mapping below hit different banks within a half wave);
// lane (l31, h) feeds v_mfma_f32_32x32x2_f32 with A[i = l31][c = 8 kb + 4 h + q] and B[same c][j = l31], q = 0 .. 3, so the
// contraction index ascends through one accumulator chain: the order of the additions depends on the shape alone.  The next chunk's
// values are fetched into registers while the current one is multiplied.  What an operand IS is a pair of functions of (row or
// column, c): at() gives an address that is ALWAYS valid (indices clamped into the matrix), so the fetch is unconditional and
// nothing waits for it; val() turns the fetched value into the operand when it goes to LDS a chunk later, and does the bounds
// there.  AMIN / BMIN say which index of the operand is contiguous in memory (the contraction index, or the row / column) and pick
// the thread mapping that reads it coalesced.
#pragma once
#include "common.h"

namespace sdfa_tile {

constexpr int T = 64, CH = 64, LP = 65, THREADS = 256;
constexpr int NR = T * CH / THREADS;      // elements of a slab per thread
static_assert(T == 64 && THREADS == 4 * 64 && CH % 8 == 0 && THREADS % CH == 0 && THREADS % T == 0, "tiling");

template <bool AMIN, bool BMIN, class OA, class OB>
__device__ __forceinline__ void tile_acc(f32x16 &acc, const int C, const OA &opA, const OB &opB, float *sA, float *sB) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5, wi = wave >> 1, wj = wave & 1;
    // this thread's NR elements of a slab: (index, c) = (ia + sia r, ca + sca r); consecutive threads take consecutive c (MIN) or
    // consecutive rows
    const int ia = AMIN ? tid / CH : tid % T, sia = AMIN ? THREADS / CH : 0, ca = AMIN ? tid % CH : tid / T, sca = AMIN ? 0 : THREADS / T;
    const int ib = BMIN ? tid / CH : tid % T, sib = BMIN ? THREADS / CH : 0, cb = BMIN ? tid % CH : tid / T, scb = BMIN ? 0 : THREADS / T;
    float ra[NR], rb[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        ra[r] = *opA.at(ia + sia * r, ca + sca * r);
        rb[r] = *opB.at(ib + sib * r, cb + scb * r);
    }
    const int nch = (C + CH - 1) / CH;
    const float *pa = sA + 4 * h * LP + 32 * wi + l31, *pb = sB + 4 * h * LP + 32 * wj + l31;
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();                                    // the previous chunk's (or caller's) reads of the slabs are done
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            sA[(ca + sca * r) * LP + ia + sia * r] = opA.val(ia + sia * r, ch * CH + ca + sca * r, ra[r]);
            sB[(cb + scb * r) * LP + ib + sib * r] = opB.val(ib + sib * r, ch * CH + cb + scb * r, rb[r]);
        }
        __syncthreads();
        if (ch + 1 < nch) {
            const int c0 = (ch + 1) * CH;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                ra[r] = *opA.at(ia + sia * r, c0 + ca + sca * r);
                rb[r] = *opB.at(ib + sib * r, c0 + cb + scb * r);
            }
        }
        const int left = C - ch * CH;
        const int nkb = left >= CH ? CH / 8 : (left + 7) / 8;     // the slab holds zeros from C to the end of its last k-block
        // a k-block's eight operands are read from LDS while the block before it is multiplied: one wave per SIMD has nobody
        // else to hide that latency
        float xa[4], xb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xa[q] = pa[q * LP];
            xb[q] = pb[q * LP];
        }
        for (int kb = 0; kb < nkb; ++kb) {
            float ya[4], yb[4];
            const int nx = kb + 1 < nkb ? kb + 1 : kb;      // the last block reads itself again: no branch around the loads
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ya[q] = pa[(8 * nx + q) * LP];
                yb[q] = pb[(8 * nx + q) * LP];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = MFMA(xa[q], xb[q], acc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                xa[q] = ya[q];
                xb[q] = yb[q];
            }
        }
    }
}

// the row of accumulator register r inside a wave's 32 x 32 quarter, for the lane half h = lane >> 5
__device__ __forceinline__ constexpr int tile_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ void zero(f32x16 &acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

// the fixed butterfly: every lane ends with the same sum
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

}  // namespace sdfa_tile
