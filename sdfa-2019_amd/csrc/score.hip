// Validation losses (include/sdfa_score.h): per-frame sums of squares of PLoss and MLoss from the
// prediction rows and the ground-truth track, the blended truth formed on the fly.
//
// Grid: x = column slab (SCORE_COLS columns), y = run of SCORE_RUN consecutive frames.  A thread owns 36 columns of its slab
// and walks the run, keeping e(p) and e(t) of the previous frame in registers, so the motion terms cost no second read.
// Its columns are strided so that every load instruction of a wavefront reads consecutive memory: with rows that are 16-byte
// aligned (dgrad with T % 4 == 0, FLAME's 9,976) quad q of thread i is quad 256 q + i of the slab, one float4 load (VEC = 4);
// otherwise column 256 k + i, a dword load (VEC = 1: other T, and the offsets head, whose 60,276-byte rows are not aligned).
// dgrad: whether a register holds a scale or a rotat value (column % 9 >= 6) then differs from lane to lane.  It is a bit
// mask formed once per thread; expf runs under it.  (Four whole triangles per thread would make the role a compile-time
// constant and expf a third as frequent, but put the lanes of a load 144 B apart: measured 8 x slower)
// Each wavefront adds its squares by a fixed butterfly and writes one partial per frame; score_sum_kernel adds the partials
// of a frame in ascending order.  No atomics, no LDS, no barrier.
#include "common.h"
#include "score.h"

#include <math.h>

namespace {

constexpr int COLS = SDFA_SCORE_COLS, RUN = SDFA_SCORE_RUN, PARTS = SDFA_SCORE_PARTS, PER = 36, THREADS = 256;
static_assert(COLS == THREADS * PER && COLS % 9 == 0 && PER % 9 == 0 && PER % 4 == 0 && PARTS == THREADS / 64, "tiling");

__device__ __forceinline__ float fsub_exact(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The plan entry of one frame, the same in every lane.
struct Blend {
    const float *r0, *r1;
    float w0, w1;
    bool ok;
};

__device__ __forceinline__ Blend plan_of(const ScoreArgs &a, int64_t f) {
    Blend b;
    const int64_t s0 = a.src[2 * f], s1 = a.src[2 * f + 1];
    b.ok = s0 >= 0 && s0 < a.n_track && s1 >= 0 && s1 < a.n_track;
    b.r0 = a.track + (b.ok ? s0 : 0) * a.W;
    b.r1 = a.track + (b.ok ? s1 : 0) * a.W;
    b.w0 = a.w[2 * f];
    b.w1 = a.w[2 * f + 1];
    return b;
}

// Column of register k of a thread whose first column is col0: VEC = 4: quad q = k / 4 of the thread is quad q * 256 + tid of
// the slab; VEC = 1: column k * 256 + tid of the slab.  Either way a load instruction of a wavefront reads consecutive memory.
template <int VEC>
__device__ __forceinline__ constexpr int col_step(int k) {
    return VEC == 4 ? (k / 4) * THREADS * 4 + k % 4 : k * THREADS;
}

// Bit k: register k holds a rotat value (column % 9 >= 6).  A slab starts at a multiple of 9, so the bits depend on the
// thread alone and are formed once, before the frame loop.
template <int LAYOUT, int VEC>
__device__ __forceinline__ uint64_t rotat_bits(int first_col_in_slab) {
    uint64_t bits = 0;
    if (LAYOUT == SDFA_SCORE_LAYOUT_DGRAD) {
        const int r = first_col_in_slab % 9;
#pragma unroll
        for (int k = 0; k < PER; ++k) bits |= (uint64_t)((r + col_step<VEC>(k) % 9) % 9 >= 6) << k;
    }
    return bits;
}

// e(p) and e(t) of one frame for this thread's columns.  Columns at or past W are left untouched (they are never used).
template <int LAYOUT, int VEC>
__device__ __forceinline__ void load_frame(const ScoreArgs &a, int64_t f, const Blend &b, int64_t col0, uint64_t rot, float (&ep)[PER], float (&et)[PER]) {
    const float *__restrict__ p = a.pred + f * a.W;
    const float nan = __builtin_nanf("");
    if (VEC == 4) {
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const int64_t c = col0 + col_step<4>(4 * q);
            if (c < a.W) {                                   // W % 4 == 0 here: the whole quad is inside
                const float4 x = ld4(p + c);
                float4 t = make_float4(nan, nan, nan, nan);
                if (b.ok) {
                    const float4 u = ld4(b.r0 + c), v = ld4(b.r1 + c);
                    t = make_float4(fadd_exact(fmul_exact(b.w0, u.x), fmul_exact(b.w1, v.x)), fadd_exact(fmul_exact(b.w0, u.y), fmul_exact(b.w1, v.y)),
                                    fadd_exact(fmul_exact(b.w0, u.z), fmul_exact(b.w1, v.z)), fadd_exact(fmul_exact(b.w0, u.w), fmul_exact(b.w1, v.w)));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * q + e;
                    const bool r = LAYOUT == SDFA_SCORE_LAYOUT_DGRAD && ((rot >> k) & 1);
                    ep[k] = r ? expf(f4c(x, e)) : f4c(x, e);
                    et[k] = r ? expf(f4c(t, e)) : f4c(t, e);
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t c = col0 + col_step<1>(k);
            if (c < a.W) {
                const float x = p[c];
                const float t = b.ok ? fadd_exact(fmul_exact(b.w0, b.r0[c]), fmul_exact(b.w1, b.r1[c])) : nan;
                const bool r = LAYOUT == SDFA_SCORE_LAYOUT_DGRAD && ((rot >> k) & 1);
                ep[k] = r ? expf(x) : x;
                et[k] = r ? expf(t) : t;
            }
        }
    }
}

template <int LAYOUT, int VEC>
__global__ __launch_bounds__(THREADS) void score_kernel(ScoreArgs a) {
    const int tid = threadIdx.x;
    const int64_t slab = blockIdx.x;
    const int64_t f0 = (int64_t)blockIdx.y * RUN, f1 = f0 + RUN < a.F ? f0 + RUN : a.F;
    const int64_t col0 = slab * COLS + tid * VEC;            // first column of this thread
    const uint64_t rot = rotat_bits<LAYOUT, VEC>(tid * VEC);
    const double qnan = __builtin_nan("");

    float pp[PER], pt[PER];                                  // e(p), e(t) of the previous frame (NaN truth after a bad plan entry)
    if (!a.first[f0]) load_frame<LAYOUT, VEC>(a, f0 - 1, plan_of(a, f0 - 1), col0, rot, pp, pt);      // the run continues a clip
    for (int64_t f = f0; f < f1; ++f) {
        const bool first = a.first[f] != 0;
        const Blend b = plan_of(a, f);
        float ep[PER], et[PER];
        load_frame<LAYOUT, VEC>(a, f, b, col0, rot, ep, et);
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (col0 + col_step<VEC>(k) < a.W) {
                // a term joins the scale or the rotat sum; the other sum takes an exact 0
                const bool r = LAYOUT == SDFA_SCORE_LAYOUT_DGRAD && ((rot >> k) & 1);
                const float d = fsub_exact(ep[k], et[k]);
                const double ds = (double)(r ? 0.0f : d);
                s[0] += ds * ds;
                if (LAYOUT == SDFA_SCORE_LAYOUT_DGRAD) {
                    const double dr = (double)(r ? d : 0.0f);
                    s[1] += dr * dr;
                }
                if (!first) {
                    const float m = fsub_exact(fsub_exact(ep[k], pp[k]), fsub_exact(et[k], pt[k]));
                    const double ms = (double)(r ? 0.0f : m);
                    s[2] += ms * ms;
                    if (LAYOUT == SDFA_SCORE_LAYOUT_DGRAD) {
                        const double mr = (double)(r ? m : 0.0f);
                        s[3] += mr * mr;
                    }
                }
                pp[k] = ep[k];
                pt[k] = et[k];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
        if ((tid & 63) == 0) {
            double *o = a.part + ((f * a.nslab + slab) * PARTS + (tid >> 6)) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = b.ok ? s[i] : qnan;      // plain: slots 1 and 3 would stay 0
        }
    }
}

// out[f][slot] = the frame's nslab * PARTS partials added in ascending order
__global__ __launch_bounds__(256) void score_sum_kernel(const double *__restrict__ part, int64_t n, int64_t nper, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t f = i >> 2;
    const int slot = (int)(i & 3);
    const double *__restrict__ p = part + f * nper * 4 + slot;
    double s = 0.0;
    for (int64_t j = 0; j < nper; ++j) s += p[j * 4];
    out[i] = s;
}

// first[off[i]] = 1 for the clip starts of one chunk, which arrives by value
__global__ __launch_bounds__(256) void score_mark_kernel(ScoreMarks m, unsigned char *first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m.n) first[m.off[i]] = 1;
}

}  // namespace

hipError_t score_mark(const ScoreMarks &m, unsigned char *first, hipStream_t st) {
    hipLaunchKernelGGL(score_mark_kernel, dim3((m.n + 255) / 256), dim3(256), 0, st, m, first);
    return hipGetLastError();
}

hipError_t score_launch(const ScoreArgs &a, int layout, hipStream_t st) {
    const dim3 grid((unsigned)a.nslab, (unsigned)((a.F + RUN - 1) / RUN));
    if (layout == SDFA_SCORE_LAYOUT_PLAIN) {
        hipLaunchKernelGGL((score_kernel<SDFA_SCORE_LAYOUT_PLAIN, 1>), grid, dim3(THREADS), 0, st, a);
    } else {
        const bool vec = a.W % 4 == 0 && (((uintptr_t)a.pred | (uintptr_t)a.track) & 15) == 0;
        if (vec) hipLaunchKernelGGL((score_kernel<SDFA_SCORE_LAYOUT_DGRAD, 4>), grid, dim3(THREADS), 0, st, a);
        else hipLaunchKernelGGL((score_kernel<SDFA_SCORE_LAYOUT_DGRAD, 1>), grid, dim3(THREADS), 0, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n = a.F * 4;
    hipLaunchKernelGGL(score_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, n, a.nslab * PARTS, a.out);
    return hipGetLastError();
}
