// Audio ingest next row: band-limited sample-rate conversion, the arithmetic of
// librosa.resample(res_type="kaiser_best") = resampy.resample that the reference runs on every input file
// (speech_anime/model/eval_utils.py:76-86: decode at 44.1 kHz, then 44.1 kHz -> hparams.audio.sample_rate;
// saber/data/audio/io.py:9-15).  librosa / resampy are third-party and absent from the reference tree: the published
// algorithm is restated (resampy/interpn.py resample_f; filter kaiser_best = Kaiser-windowed sinc, 64 zero crossings, 512
// table entries per crossing) -- parity unpinned, see oracle/resample_oracle.py.
//
// One thread per output sample, offline (resample_kernel: a whole clip) and live (stream_resample_kernel: the outputs of a step that
// have become final, from each stream's input ring into its model ring); both run resample_taps.  Output t reads the time register treg[t] (accumulated sequentially in float64 on the
// host, as the reference accumulates it), walks the left wing of the filter from the fractional offset in steps of
// `step` table entries, then the right wing; every tap is  weight = win[k] + eta * delta[k]  (float64), product with the
// float32 sample in float64, added to the running sum, which is ROUNDED TO FLOAT32 AFTER EVERY TAP (resampy accumulates
// into the float32 output array).  All operations are issued with explicit rounding intrinsics: no FMA contraction.
// The table (2 x 256 KiB) is L2-resident; a 10 s clip is 80-441 k outputs x 128-712 taps -- an ingest step, not a hot loop.
#include "common.h"
#include "kernels.h"

namespace {

// Where the input samples of one signal live.  ClipIn: a whole clip, linear.  RingIn: a live stream's input ring of 2^r_in samples
// (include/sdfa_stream.h), absolute position p at p & mask.  Both wings stop at the signal's ends through `n_in` below: the clip's
// length offline, the number of samples the stream has received so far (its length once it has ended) live.
struct ClipIn {
    const float *__restrict__ x;
    __device__ __forceinline__ float at(int64_t p) const { return x[p]; }
};
struct RingIn {
    const float *__restrict__ ring;
    int64_t mask;
    __device__ __forceinline__ float at(int64_t p) const { return ring[p & mask]; }
};

// Output sample with time register `tr`: left wing, then right wing, the sum rounded to float32 after every tap.
template <class In>
__device__ __forceinline__ float resample_taps(const In X, int64_t n_in, double tr, const double *__restrict__ win,
                                               const double *__restrict__ delta, int64_t nwin, int64_t step, double scale, int num_table) {
    const int64_t n = (int64_t)tr;
    double frac = dmul_exact(scale, dsub_exact(tr, (double)n));
    float acc = 0.f;
#pragma unroll 1
    for (int wing = 0; wing < 2; ++wing) {
        if (wing) frac = dsub_exact(scale, frac);
        const double index_frac = dmul_exact(frac, (double)num_table);
        const int64_t offset = (int64_t)index_frac;
        const double eta = dsub_exact(index_frac, (double)offset);
        const int64_t room = (nwin - offset) / step;
        const int64_t have = wing ? n_in - n - 1 : n + 1;
        const int64_t kmax = have < room ? have : room;
        const double *__restrict__ wp = win + offset, *__restrict__ dp = delta + offset;
        const int64_t x0 = wing ? n + 1 : n, xs = wing ? 1 : -1;
        // eight taps' loads in flight at once: the sum itself is one chain of float32 roundings, and without this each tap waits for its own
        // table entries (measured on the live step)
#pragma unroll 8
        for (int64_t i = 0; i < kmax; ++i) {
            const double w = dadd_exact(wp[i * step], dmul_exact(eta, dp[i * step]));
            acc = (float)dadd_exact((double)acc, dmul_exact(w, (double)X.at(x0 + i * xs)));
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_out) return;
    if (t >= a.n_res) { a.y[t] = 0.f; return; }          // librosa util.fix_length: zero padding up to ceil(n * ratio)
    a.y[t] = resample_taps(ClipIn{a.x}, a.n_in, a.treg[t], a.win, a.delta, a.nwin, a.step, a.scale, a.num_table);
}

// Live streams (include/sdfa_stream.h): every stream's new outputs of a step in one launch.  blockIdx.y is the segment
// seg[8 j .. 8 j + 7] = (input ring, model ring, t0, count, n_in, t_zero, offset in treg, rate index | gain bits << 32), blockIdx.x the
// block of 256 outputs in it.  Output t = t0 + i goes to position t & (R - 1) of the model ring (and into the mirror when that is below
// RING_MIRROR, as ring_append_kernel keeps it), multiplied by the gain in float32 and clamped to +-0.999.  t < 0 (the zeros ahead of an
// ensembling stream) and t >= t_zero (fix_length's zeros once the stream has ended) are zeros; treg[off + i] is the register of output
// max(t0, 0) + i.  A rate whose step is 0 copies (input rate = model rate).  A segment that names a ring or a rate outside its table,
// a count outside [0, R] or register values outside [0, n_treg) is skipped whole; an output whose register lies outside [0, n_in)
// is skipped (the taps then stay inside the filter table, and every sample address is masked into its ring).
__global__ __launch_bounds__(256) void stream_resample_kernel(StreamResampleArgs a) {
    const int64_t *__restrict__ sg = a.seg + 8 * (int64_t)blockIdx.y;
    const int64_t in_ring = sg[0], out_ring = sg[1], t0 = sg[2], count = sg[3], n_in = sg[4], t_zero = sg[5], off = sg[6];
    const int64_t rate = sg[7] & 0xffffffff;
    const float gain = __uint_as_float((uint32_t)((uint64_t)sg[7] >> 32));
    const int64_t R = (int64_t)1 << a.r, R_in = (int64_t)1 << a.r_in;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count || count > R || (uint64_t)in_ring >= (uint64_t)a.n_in_rings || (uint64_t)out_ring >= (uint64_t)a.n_rings ||
        (uint64_t)rate >= (uint64_t)a.n_rates || n_in < 0 || off < 0)
        return;
    const int64_t first = t0 < 0 ? 0 : t0;                // the first output that has a register
    const int64_t stop = t0 + count < t_zero ? t0 + count : t_zero;
    const StreamRate rt = a.rate[rate];
    if (rt.step != 0 && stop > first && off > a.n_treg - (stop - first)) return;      // (a copy reads no registers)
    const RingIn X{a.in_rings + in_ring * (R_in + STREAM_RING_MIRROR), R_in - 1};
    const int64_t t = t0 + i;
    float v = 0.f;
    if (t >= 0 && t < t_zero) {
        if (rt.step == 0) {
            if (t >= n_in) return;
            v = X.at(t);
        } else {
            const double tr = a.treg[off + (t - first)];
            if (!(tr >= 0.0 && tr < (double)n_in)) return;
            v = resample_taps(X, n_in, tr, rt.win, rt.win + a.nwin, a.nwin, rt.step, rt.scale, a.num_table);
        }
        v = fmul_exact(v, gain);
        v = __builtin_fminf(__builtin_fmaxf(v, -0.999f), 0.999f);
    }
    float *__restrict__ dst = a.rings + out_ring * (R + STREAM_RING_MIRROR);
    const int64_t q = t & (R - 1);
    dst[q] = v;
    if (q < STREAM_RING_MIRROR) dst[R + q] = v;
}

}  // namespace

hipError_t sdfa_launch_resample(const ResampleArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((a.n_out + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t sdfa_launch_stream_resample(const StreamResampleArgs &a, int n_seg, int64_t max_count, hipStream_t s) {
    if (n_seg <= 0 || max_count <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_resample_kernel, dim3((unsigned)((max_count + 255) / 256), (unsigned)n_seg), dim3(256), 0, s, a);
    return hipGetLastError();
}
