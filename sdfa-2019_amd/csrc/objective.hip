// Training objective (include/sdfa_objective.h): PLoss and MLoss of a collated batch [a; b] and their
// gradients with respect to the PCA coefficients, from the coefficients, the basis and the truth rows.  The expanded rows
// and the residual rows live in accumulators and in LDS only.
//
// Grid: x = column partition (those of the scale basis first, then the rotat basis'), y = row tile.  A workgroup owns
// PAIRS = 16 whole pairs -- MFMA rows 0..15 are the a rows k0 .. k0 + 15, rows 16..31 their b rows B + k0 .. -- and walks a
// contiguous range of column blocks of COLS = 128 columns of ONE basis.  Per column block:
//   1. the slab compT[col0 .. col0 + 127][0 .. K) goes to LDS as sB[column][KP], k >= K zero.  In global memory it is one
//      contiguous run of floats (the row stride is K), whatever K's alignment: LDS-DMA moves it in 256-byte pieces.
//   2. expansion: wave w owns columns 32 w .. 32 w + 31: D[32 rows][32 columns] over k with v_mfma_f32_32x32x2_f32, A from the
//      coefficient tile sA[row][KP] (loaded once per workgroup), B from sB, both as float4 along k (common.h: lane half h
//      takes k-quad 2 kb + h).
//   3. epilogue in the accumulator layout: a lane holds column l31 of rows (r & 3) + 8 (r >> 2) + 4 h, so rows i and i + 16 --
//      a pair -- are registers r and r + 8 of the SAME lane: mean, truth, e, the two residuals and the motion difference
//      need no exchange.  Squares go to per-lane doubles (16 row sums + 8 pair sums); g_p and g_m go to LDS as sG[term][row][GP].
//   4. contraction: wave w owns term w & 1 and the coefficient tiles (w >> 1) + 2 u of 32: D[32 rows][32 coefficients] over
//      the block's 128 columns, A = sG as float4 along the columns, B = the SAME slab read across k (lane l31 = coefficient:
//      consecutive banks).  These accumulators live across the workgroup's column blocks.
// At the end the gradient tiles go to the workspace as float32 partials [partition][term][row][KS], the sums of squares --
// reduced over a half wave by a fixed butterfly, over the four waves in ascending order -- as double partials
// [partition][row][2].  Finishing kernels add the partitions in ascending order, in double.  No atomics.
#include "common.h"
#include "objective.h"

#include <math.h>

namespace {

constexpr int COLS = SDFA_OBJECTIVE_COLS, PAIRS = SDFA_OBJECTIVE_PAIRS, ROWS = 2 * PAIRS, THREADS = 256, GP = COLS + 4;
static_assert(ROWS == 32 && COLS == 32 * (THREADS / 64) && SDFA_OBJECTIVE_MAX_K <= 6 * 32 && SDFA_OBJECTIVE_KSTEP == 8, "tiling");

__device__ __forceinline__ float fsub_exact(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

template <bool EXP>
__device__ __forceinline__ void objective_body(const ObjArgs &a, const ObjPart &pt, const int pl, float *smem) {
    const int K = pt.K, KP = pt.KP;
    float *sB = smem;                                       // [COLS][KP]
    float *sA = sB + COLS * KP;                             // [ROWS][KP]
    float *sG = sA + ROWS * KP;                             // [2][ROWS][GP]
    double *sRed = reinterpret_cast<double *>(sG + 2 * ROWS * GP);      // [4 waves][ROWS][2]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int rt = blockIdx.y;
    const int64_t k0 = (int64_t)rt * PAIRS, B = a.B, W = a.W;
    const int cb0 = (int)((int64_t)pl * pt.ncb / pt.P), cb1 = (int)((int64_t)(pl + 1) * pt.ncb / pt.P);

    // the coefficient tile: rows of pairs past B are zeros
    for (int i = wave; i < ROWS; i += 4) {
        const int64_t k = k0 + (i & 15);
        const bool ok = k < B;
        const float *src = a.coef + (ok ? (i < 16 ? k : B + k) : 0) * a.Kc + pt.koff;
        for (int kk = lane; kk < KP; kk += 64) sA[i * KP + kk] = ok && kk < K ? src[kk] : 0.f;
    }
    // the slab starts as zeros: the padding k >= K is never written again, and the columns past the end of the last block keep
    // finite values (zeros, or an earlier block's) that only ever meet g = 0
    for (int i = tid; i < COLS * KP; i += THREADS) sB[i] = 0.f;

    double sp[16], sm[8];
#pragma unroll
    for (int r = 0; r < 16; ++r) sp[r] = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) sm[r] = 0.0;
    f32x16 gacc[3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) gacc[u][r] = 0.f;
    const int term = wave & 1, it0 = wave >> 1;
    const int nkb = (K + 7) / 8;

    // A block's slab goes from global memory straight to LDS (LDS-DMA, one dword per lane: a piece is 64 consecutive k of one
    // column, 256 contiguous bytes on both sides; K's alignment does not matter).  A wave takes every fourth column; the lanes
    // past K of a column's last piece are masked off.  No registers, no index arithmetic, all of a block's pieces in flight.
#define OBJ_SLAB(cb_)                                                                                  \
    {                                                                                                  \
        const int64_t c0_ = (int64_t)(cb_) * COLS;                                                     \
        const int nc_ = (int)(pt.C - c0_ < COLS ? pt.C - c0_ : COLS);                                  \
        const float *src_ = pt.compT + c0_ * K + lane;                                                 \
        for (int c = wave; c < nc_; c += 4)                                                            \
            for (int p = 0; p < K; p += 64)                                                            \
                if (p + lane < K)                                                                      \
                    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(src_ + c * K + p), \
                                                     (void __attribute__((address_space(3))) *)(sB + c * KP + p), 4, 0, 0); \
    }

    for (int cb = cb0; cb < cb1; ++cb) {
        const int64_t col0 = (int64_t)cb * COLS;
        const int ncols = (int)(pt.C - col0 < COLS ? pt.C - col0 : COLS);
        // this lane's column, its mean and (below, in flight together with the slab) its truth values
        const int cl = 32 * wave + l31;
        const int64_t q = col0 + cl;
        const bool valid = cl < ncols;
        const float mean = valid ? pt.means[q] : 0.f;
        const int64_t tc = (q / pt.G) * pt.S + pt.OFF + q % pt.G;
        __syncthreads();                                    // the previous block's contraction is done with sB and sG
        OBJ_SLAB(cb)
        float ta[8], tb[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t k = k0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool ok = valid && k < B;
            ta[r] = ok ? a.truth[k * W + tc] : 0.f;
            tb[r] = ok ? a.truth[(B + k) * W + tc] : 0.f;
        }
        __builtin_amdgcn_s_waitcnt(0x0070);                 // this wave's pieces have landed (the compiler does not count LDS-DMA) ...
        __syncthreads();                                    // ... and everyone's

        // expansion: two accumulators take alternate k-blocks, so consecutive MFMAs do not wait for each other
        f32x16 acc, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc1[r] = 0.f; }
        {
            const float *pa = sA + l31 * KP + 4 * h, *pb = sB + (32 * wave + l31) * KP + 4 * h;
            for (int kb = 0; kb < nkb; kb += 2) {
                mfma4(acc, ld4(pa + 8 * kb), ld4(pb + 8 * kb));
                if (kb + 1 < nkb) mfma4(acc1, ld4(pa + 8 * kb + 8), ld4(pb + 8 * kb + 8));
            }
        }
        // epilogue
        {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * h;           // 0 .. 15: the pair inside the tile
                const int64_t k = k0 + i;
                float gpa = 0.f, gpb = 0.f, gma = 0.f, gmb = 0.f;
                if (valid && k < B) {
                    const float xa = (acc[r] + acc1[r]) + mean, xb = (acc[r + 8] + acc1[r + 8]) + mean;
                    const float epa = EXP ? expf(xa) : xa, epb = EXP ? expf(xb) : xb;
                    const float eta = EXP ? expf(ta[r]) : ta[r], etb = EXP ? expf(tb[r]) : tb[r];
                    const float da = fsub_exact(epa, eta), db = fsub_exact(epb, etb);
                    const float m = fsub_exact(fsub_exact(epb, epa), fsub_exact(etb, eta));
                    sp[r] += (double)da * (double)da;
                    sp[r + 8] += (double)db * (double)db;
                    sm[r] += (double)m * (double)m;
                    gpa = EXP ? fmul_exact(da, epa) : da;
                    gpb = EXP ? fmul_exact(db, epb) : db;
                    gma = -(EXP ? fmul_exact(m, epa) : m);
                    gmb = EXP ? fmul_exact(m, epb) : m;
                }
                sG[i * GP + cl] = gpa;
                sG[(i + 16) * GP + cl] = gpb;
                sG[(ROWS + i) * GP + cl] = gma;
                sG[(ROWS + i + 16) * GP + cl] = gmb;
            }
        }
        __syncthreads();

        // contraction over the block's columns
        {
            const float *ga = sG + (term * ROWS + l31) * GP + 4 * h;
            for (int c8 = 0; c8 < COLS / 8; ++c8) {
                const float4 av = ld4(ga + 8 * c8);
                const float *bb = sB + (8 * c8 + 4 * h) * KP + l31;
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int it = it0 + 2 * u;
                    if (32 * it < K) {                      // uniform
                        const float b0 = bb[32 * it], b1 = bb[KP + 32 * it], b2 = bb[2 * KP + 32 * it], b3 = bb[3 * KP + 32 * it];
                        gacc[u] = MFMA(av.x, b0, gacc[u]);
                        gacc[u] = MFMA(av.y, b1, gacc[u]);
                        gacc[u] = MFMA(av.z, b2, gacc[u]);
                        gacc[u] = MFMA(av.w, b3, gacc[u]);
                    }
                }
            }
        }
    }

#undef OBJ_SLAB
    // partial gradients: every row of the tile, the zeros of pairs past B included
    {
        float *gp = a.gpart + pt.gpart_off + (((int64_t)pl * 2 + term) * a.rowtiles + rt) * ROWS * pt.KS;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int it = it0 + 2 * u;
            if (32 * it < K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
                    gp[i * pt.KS + 32 * it + l31] = gacc[u][r];
                }
            }
        }
    }
    // sums of squares: over the 32 columns of a half wave by a fixed butterfly, then the four waves in ascending order
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) sp[r] += __shfl_xor(sp[r], m, 64);
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) sm[r] += __shfl_xor(sm[r], m, 64);
    if (l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * h;   // 0 .. 31
            sRed[(wave * ROWS + i) * 2] = sp[r];
            sRed[(wave * ROWS + i) * 2 + 1] = r >= 8 ? sm[r - 8] : 0.0;
        }
    }
    __syncthreads();
    if (tid < ROWS) {
        const int64_t k = k0 + (tid & 15);
        if (k < B) {
            double s0 = 0.0, s1 = 0.0;
            for (int w = 0; w < 4; ++w) {
                s0 += sRed[(w * ROWS + tid) * 2];
                s1 += sRed[(w * ROWS + tid) * 2 + 1];
            }
            double *o = a.lpart + ((int64_t)(pt.px0 + pl) * a.N + (tid < 16 ? k : B + k)) * 2;
            o[0] = s0;
            o[1] = s1;
        }
    }
}

__global__ __launch_bounds__(THREADS) void objective_kernel(ObjArgs a) {
    extern __shared__ float4 sObj[];
    float *smem = reinterpret_cast<float *>(sObj);
    const int px = blockIdx.x;
    if (a.nparts == 2 && px >= a.part[1].px0) objective_body<true>(a, a.part[1], px - a.part[1].px0, smem);
    else objective_body<false>(a, a.part[0], px, smem);
}

// rec[r] = (ps, ms, pr, mr): the partitions of a part added in ascending order; one thread per row and part (the loads of
// eight partitions are requested together, the additions keep their order)
__global__ __launch_bounds__(256) void objective_rec_kernel(ObjArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * a.N) return;
    const int64_t r = idx >> 1;
    const int p = (int)(idx & 1);
    double s0 = 0.0, s1 = 0.0;
    if (p < a.nparts) {
        const ObjPart &pt = a.part[p];
        const double *q = a.lpart + ((int64_t)pt.px0 * a.N + r) * 2;
#pragma unroll 8
        for (int j = 0; j < pt.P; ++j) {
            s0 += q[(int64_t)j * a.N * 2];
            s1 += q[(int64_t)j * a.N * 2 + 1];
        }
    }
    a.rec[r * 4 + 2 * p] = s0;
    a.rec[r * 4 + 2 * p + 1] = r >= a.B ? s1 : 0.0;
}

// grad[term][r][i] = fl(c_term[r] * sum over the partitions, ascending, in double)
__global__ __launch_bounds__(256) void objective_grad_kernel(ObjArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = a.N * a.Kc;
    if (idx >= 2 * per) return;
    const int term = (int)(idx / per);
    const int64_t r = (idx - term * per) / a.Kc;
    const int i = (int)(idx - term * per - r * a.Kc);
    const ObjPart &pt = a.part[a.nparts == 2 && i >= a.part[1].koff ? 1 : 0];
    const int64_t k = r < a.B ? r : r - a.B;
    const int64_t trow = (k / PAIRS) * ROWS + k % PAIRS + (r < a.B ? 0 : PAIRS);
    const int64_t stride = 2 * (int64_t)a.rowtiles * ROWS * pt.KS;
    const float *g = a.gpart + pt.gpart_off + ((int64_t)term * a.rowtiles * ROWS + trow) * pt.KS + (i - pt.koff);
    double s = 0.0;
#pragma unroll 8
    for (int j = 0; j < pt.P; ++j) s += (double)g[j * stride];
    const double c = term == 0 ? 2.0 * (double)a.weight[r] / ((double)a.N * a.n)
                               : 2.0 * (double)fadd_exact(a.weight[k], a.weight[a.B + k]) / ((double)a.B * a.n);
    a.grad[idx] = (float)(s * c);
}

// loss = (ps, ms, pr, mr): one workgroup, rows strided over the threads, then a fixed tree
__global__ __launch_bounds__(256) void objective_loss_kernel(ObjArgs a) {
    __shared__ double sL[256][4];
    const int tid = threadIdx.x;
    double l[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = tid; r < a.N; r += 256) {
        const double w = (double)a.weight[r];
        l[0] += w * a.rec[r * 4];
        l[2] += w * a.rec[r * 4 + 2];
        if (r >= a.B) {
            const double hk = (double)fadd_exact(a.weight[r - a.B], a.weight[r]);
            l[1] += hk * a.rec[r * 4 + 1];
            l[3] += hk * a.rec[r * 4 + 3];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sL[tid][i] = l[i];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int i = 0; i < 4; ++i) sL[tid][i] += sL[tid + s][i];
        __syncthreads();
    }
    if (tid < 4) a.loss[tid] = (float)(sL[0][tid] / (((tid & 1) ? (double)a.B : (double)a.N) * a.n));
}

}  // namespace

size_t objective_lds_bytes(int KPmax) {
    return (size_t)(COLS + ROWS) * KPmax * sizeof(float) + 2 * ROWS * GP * sizeof(float) + 4 * ROWS * 2 * sizeof(double);
}

hipError_t objective_launch(const ObjArgs &a, hipStream_t st) {
    int kp = a.part[0].KP, px = a.part[0].P;
    if (a.nparts == 2) {
        kp = a.part[1].KP > kp ? a.part[1].KP : kp;
        px += a.part[1].P;
    }
    const size_t lds = objective_lds_bytes(kp);
    // the kernel's dynamic-LDS limit is raised once per device and again only when a call needs more: no runtime call per launch
    static std::atomic<int> granted[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool kept = dev >= 0 && dev < 64;
    if (!kept || granted[dev].load(std::memory_order_relaxed) < (int)lds) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(objective_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (kept) granted[dev].store((int)lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(objective_kernel, dim3((unsigned)px, (unsigned)a.rowtiles), dim3(THREADS), lds, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(objective_rec_kernel, dim3((unsigned)((2 * a.N + 255) / 256)), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t ng = 2 * a.N * a.Kc;
    hipLaunchKernelGGL(objective_grad_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(objective_loss_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}
