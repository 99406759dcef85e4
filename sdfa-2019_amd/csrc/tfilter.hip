// Temporal track filters (include/sdfa_tfilter.h): a symmetric FIR with scipy's reflect boundaries
// and the reference's bilateral filter, both along the frames of each clip of a batch of rows, evaluated in double.
//
// Grid: x = column slab (COLS columns), y = run of RUN consecutive frames of the launch.  A thread owns 4 columns of its slab,
// strided so that every load instruction of a wavefront reads consecutive memory: with 16-byte aligned rows (W % 4 == 0,
// dgrad) one float4 at quad tid (VEC = 4); otherwise columns 256 k + tid, dword loads (VEC = 1: the offsets rows).
// Two forms of each filter, the same expression in the same order:
//   R >= 1  register window: the thread keeps frames f - R .. f + R of its columns (reflected into the clip for the FIR,
//           absent outside it for the bilateral) in registers, shifts them and fetches one frame per output frame.  A run
//           and a clip that begins inside a run fill the window afresh.
//   R <  0  generic: every output frame re-reads its 2 r + 1 neighbours, which the other frames of the run keep in cache.
// No atomics, no LDS, no barrier.  The clip table and the weights are kernel arguments.
#include "common.h"
#include "tfilter.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256, PER = 4, COLS = SDFA_TFILTER_COLS, RUN = SDFA_TFILTER_RUN;
static_assert(COLS == THREADS * PER, "tiling");

// scipy's reflect, d c b a | a b c d | d c b a, for a clip of n frames; i may lie several reflections outside.
__device__ __forceinline__ int refl(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    int j = i % p;
    if (j < 0) j += p;
    return j < n ? j : p - 1 - j;
}

template <int VEC>
__device__ __forceinline__ int64_t first_col(int64_t slab, int tid) {
    return slab * COLS + (VEC == 4 ? tid * 4 : tid);
}

template <int VEC>
__device__ __forceinline__ constexpr int col_step(int k) {
    return VEC == 4 ? k : k * THREADS;
}

// The thread's four columns of one row; columns at or past W read as 0 and are never stored.
template <int VEC>
__device__ __forceinline__ void load_cols(const float *__restrict__ row, int64_t col0, int64_t W, float (&v)[PER]) {
    if (VEC == 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col0 < W) t = ld4(row + col0);                   // W % 4 == 0 here: the whole quad is inside
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t c = col0 + col_step<1>(k);
            v[k] = c < W ? row[c] : 0.f;
        }
    }
}

template <int VEC>
__device__ __forceinline__ void store_cols(float *__restrict__ row, int64_t col0, int64_t W, const float (&v)[PER]) {
    if (VEC == 4) {
        if (col0 < W) st4(row + col0, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t c = col0 + col_step<1>(k);
            if (c < W) row[c] = v[k];
        }
    }
}

// One term of the FIR: acc + (lo + hi) w, three separately rounded double operations.
__device__ __forceinline__ double fir_term(double acc, float lo, float hi, double w) {
    return dadd_exact(acc, dmul_exact(dadd_exact((double)lo, (double)hi), w));
}

// One neighbour of the bilateral filter.
__device__ __forceinline__ void bilateral_term(double xc, float xn_, double dw, double factor, double range_sigma, double &ws, double &mean) {
    const double xn = (double)xn_;
    const double delta = dsub_exact(xc, xn);
    const double s = sqrt(dmul_exact(delta, delta)) / range_sigma;
    const double sw = exp(dmul_exact(dmul_exact(s, s), factor));
    const double wt = dmul_exact(dw, sw);
    ws = dadd_exact(ws, wt);
    mean = dadd_exact(mean, dmul_exact(wt, xn));
}

// The clip of frame f: the c with off[c] <= f < off[c + 1].
__device__ __forceinline__ int clip_of(const TFilterArgs &a, int f) {
    int lo = 0, hi = a.n_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.off[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <int KIND, int VEC, int R>
__global__ __launch_bounds__(THREADS) void tfilter_kernel(TFilterArgs a) {
    const int tid = threadIdx.x;
    const int f0 = a.fa + (int)blockIdx.y * RUN, f1 = f0 + RUN < a.fb ? f0 + RUN : a.fb;
    const int64_t col0 = first_col<VEC>(blockIdx.x, tid);
    const int64_t W = a.W;
    int c = clip_of(a, f0);
    int cs = a.off[c], ce = a.off[c + 1];

    if constexpr (R >= 1) {
        float win[2 * R + 1][PER];                           // slot j: frame pos - R + j of the clip
        bool fresh = true;
        for (int f = f0; f < f1; ++f) {
            if (f == ce) {
                ++c;
                cs = ce;
                ce = a.off[c + 1];
                fresh = true;
            }
            const int n = ce - cs, pos = f - cs;
            const float *__restrict__ base = a.x + (int64_t)cs * W;
            if (fresh) {
#pragma unroll
                for (int j = 0; j <= 2 * R; ++j) {
                    const int p = pos - R + j;
                    if (KIND == TFILTER_FIR) load_cols<VEC>(base + (int64_t)refl(p, n) * W, col0, W, win[j]);
                    else if (p >= 0 && p < n) load_cols<VEC>(base + (int64_t)p * W, col0, W, win[j]);
                }
                fresh = false;
            } else {
#pragma unroll
                for (int j = 0; j < 2 * R; ++j)
#pragma unroll
                    for (int k = 0; k < PER; ++k) win[j][k] = win[j + 1][k];
                const int p = pos + R;
                if (KIND == TFILTER_FIR) load_cols<VEC>(base + (int64_t)refl(p, n) * W, col0, W, win[2 * R]);
                else if (p < n) load_cols<VEC>(base + (int64_t)p * W, col0, W, win[2 * R]);
            }
            float o[PER];
            if (KIND == TFILTER_FIR) {
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    double acc = dmul_exact((double)win[R][k], a.w[R]);
#pragma unroll
                    for (int i = -R; i < 0; ++i) acc = fir_term(acc, win[R + i][k], win[R - i][k], a.w[i + R]);
                    o[k] = (float)acc;
                }
            } else {
                double ws[PER], mean[PER];
#pragma unroll
                for (int k = 0; k < PER; ++k) ws[k] = mean[k] = 0.0;
#pragma unroll
                for (int d = -R; d <= R; ++d) {
                    if (pos + d >= 0 && pos + d < n) {
#pragma unroll
                        for (int k = 0; k < PER; ++k)
                            bilateral_term((double)win[R][k], win[R + d][k], a.w[d + R], a.factor, a.range_sigma, ws[k], mean[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < PER; ++k) o[k] = (float)(mean[k] / ws[k]);
            }
            store_cols<VEC>(a.out + (int64_t)f * W, col0, W, o);
        }
    } else {
        const int r = a.radius;
        for (int f = f0; f < f1; ++f) {
            if (f == ce) {
                ++c;
                cs = ce;
                ce = a.off[c + 1];
            }
            const int n = ce - cs, pos = f - cs;
            const float *__restrict__ base = a.x + (int64_t)cs * W;
            float xc[PER], o[PER];
            load_cols<VEC>(base + (int64_t)pos * W, col0, W, xc);
            if (KIND == TFILTER_FIR) {
                double acc[PER];
#pragma unroll
                for (int k = 0; k < PER; ++k) acc[k] = dmul_exact((double)xc[k], a.w[r]);
                for (int i = -r; i < 0; ++i) {
                    float lo[PER], hi[PER];
                    load_cols<VEC>(base + (int64_t)refl(pos + i, n) * W, col0, W, lo);
                    load_cols<VEC>(base + (int64_t)refl(pos - i, n) * W, col0, W, hi);
                    const double w = a.w[i + r];
#pragma unroll
                    for (int k = 0; k < PER; ++k) acc[k] = fir_term(acc[k], lo[k], hi[k], w);
                }
#pragma unroll
                for (int k = 0; k < PER; ++k) o[k] = (float)acc[k];
            } else {
                double ws[PER], mean[PER];
#pragma unroll
                for (int k = 0; k < PER; ++k) ws[k] = mean[k] = 0.0;
                const int d0 = pos < r ? -pos : -r, d1 = n - 1 - pos < r ? n - 1 - pos : r;
                for (int d = d0; d <= d1; ++d) {
                    float xn[PER];
                    load_cols<VEC>(base + (int64_t)(pos + d) * W, col0, W, xn);
                    const double dw = a.w[d + r];
#pragma unroll
                    for (int k = 0; k < PER; ++k) bilateral_term((double)xc[k], xn[k], dw, a.factor, a.range_sigma, ws[k], mean[k]);
                }
#pragma unroll
                for (int k = 0; k < PER; ++k) o[k] = (float)(mean[k] / ws[k]);
            }
            store_cols<VEC>(a.out + (int64_t)f * W, col0, W, o);
        }
    }
}

template <int KIND, int R>
hipError_t launch_form(const TFilterArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.W + COLS - 1) / COLS), (unsigned)((a.fb - a.fa + RUN - 1) / RUN));
    const bool vec = a.W % 4 == 0 && (((uintptr_t)a.x | (uintptr_t)a.out) & 15) == 0;
    if (vec) hipLaunchKernelGGL((tfilter_kernel<KIND, 4, R>), grid, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((tfilter_kernel<KIND, 1, R>), grid, dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

template <int KIND>
hipError_t launch_kind(const TFilterArgs &a, bool generic, hipStream_t st) {
    static_assert(SDFA_TFILTER_WINDOW_RADIUS == 8, "the switch below lists the window radii");
    if (!generic) {
        switch (a.radius) {
            case 1: return launch_form<KIND, 1>(a, st);
            case 2: return launch_form<KIND, 2>(a, st);
            case 3: return launch_form<KIND, 3>(a, st);
            case 4: return launch_form<KIND, 4>(a, st);
            case 5: return launch_form<KIND, 5>(a, st);
            case 6: return launch_form<KIND, 6>(a, st);
            case 7: return launch_form<KIND, 7>(a, st);
            case 8: return launch_form<KIND, 8>(a, st);
            default: break;
        }
    }
    return launch_form<KIND, -1>(a, st);
}

}  // namespace

hipError_t tfilter_launch(const TFilterArgs &a, int kind, bool generic, hipStream_t st) {
    return kind == TFILTER_FIR ? launch_kind<TFILTER_FIR>(a, generic, st) : launch_kind<TFILTER_BILATERAL>(a, generic, st);
}
