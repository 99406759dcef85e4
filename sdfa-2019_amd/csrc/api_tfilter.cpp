// Host side of the temporal track filters (include/sdfa_tfilter.h): the refusals and the launches of
// tfilter.hip, SDFA_TFILTER_CLIPS clips per launch.  Nothing here copies or synchronises.
#include "host.h"
#include "tfilter.h"

#include <math.h>
#include <string.h>

namespace {

int check_frame(const char *who, const float *rows, const float *out, int64_t F, int64_t W, const int64_t *off, int64_t n_clips, int radius, int flags) {
    if (!rows || !out) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    if (F < 1 || F > 65535ll * SDFA_TFILTER_RUN) return sdfa_fail(SDFA_EINVAL, "%s: %lld frames outside 1 .. %lld", who, (long long)F, 65535ll * SDFA_TFILTER_RUN);
    if (W < 1 || W > (1ll << 30)) return sdfa_fail(SDFA_EINVAL, "%s: row width %lld outside 1 .. 2^30", who, (long long)W);
    if (radius < 0 || radius > SDFA_TFILTER_MAX_RADIUS) return sdfa_fail(SDFA_EINVAL, "%s: radius %d outside 0 .. %d", who, radius, SDFA_TFILTER_MAX_RADIUS);
    if (flags & ~SDFA_TFILTER_GENERIC) return sdfa_fail(SDFA_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~SDFA_TFILTER_GENERIC));
    const uintptr_t a = (uintptr_t)rows, b = (uintptr_t)out, bytes = (uintptr_t)F * (uintptr_t)W * sizeof(float);
    if (a < b + bytes && b < a + bytes) return sdfa_fail(SDFA_EINVAL, "%s: rows and out overlap", who);
    if (off) {
        if (n_clips < 1 || off[0] != 0 || off[n_clips] != F)
            return sdfa_fail(SDFA_EINVAL, "%s: the offsets of %lld clips do not run from 0 to %lld", who, (long long)n_clips, (long long)F);
        for (int64_t c = 0; c < n_clips; ++c)
            if (off[c + 1] <= off[c] || off[c + 1] > F)
                return sdfa_fail(SDFA_EINVAL, "%s: clip %lld is empty or its offsets descend (%lld .. %lld)", who, (long long)c, (long long)off[c], (long long)off[c + 1]);
    }
    return SDFA_OK;
}

// a holds everything but the clip table: one launch per SDFA_TFILTER_CLIPS clips.
int launch_all(TFilterArgs &a, int kind, int64_t F, const int64_t *off, int64_t n_clips, int flags, hipStream_t st) {
    const int64_t one[2] = {0, F};
    if (!off) off = one, n_clips = 1;
    for (int64_t c = 0; c < n_clips; c += SDFA_TFILTER_CLIPS) {
        a.n_clips = (int)(n_clips - c < SDFA_TFILTER_CLIPS ? n_clips - c : SDFA_TFILTER_CLIPS);
        for (int i = 0; i <= a.n_clips; ++i) a.off[i] = (int)off[c + i];
        a.fa = a.off[0];
        a.fb = a.off[a.n_clips];
        HIP_TRY(tfilter_launch(a, kind, (flags & SDFA_TFILTER_GENERIC) != 0, st));
    }
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_tfilter_abi_version(void) { return SDFA_TFILTER_ABI_VERSION; }

int sdfa_track_fir(const float *d_rows, float *d_out, int64_t F, int64_t W, const int64_t *clip_frame_off, int64_t n_clips,
                   const double *taps, int radius, int flags, void *stream) {
    const int rc = check_frame("track_fir", d_rows, d_out, F, W, clip_frame_off, n_clips, radius, flags);
    if (rc < 0) return rc;
    if (!taps) return sdfa_fail(SDFA_EINVAL, "track_fir: null taps");
    for (int i = 0; i < radius; ++i)
        if (memcmp(&taps[i], &taps[2 * radius - i], sizeof(double)) != 0)
            return sdfa_fail(SDFA_EINVAL, "track_fir: taps %d and %d differ, the filter is symmetric", i, 2 * radius - i);
    TFilterArgs a;
    memset(&a, 0, sizeof(a));
    a.x = d_rows;
    a.out = d_out;
    a.W = W;
    a.radius = radius;
    memcpy(a.w, taps, sizeof(double) * (size_t)(2 * radius + 1));
    return launch_all(a, TFILTER_FIR, F, clip_frame_off, n_clips, flags, (hipStream_t)stream);
}

int sdfa_track_bilateral(const float *d_rows, float *d_out, int64_t F, int64_t W, const int64_t *clip_frame_off, int64_t n_clips,
                         double factor, double distance_sigma, double range_sigma, int radius, const double *dist_w, int flags,
                         void *stream) {
    const int rc = check_frame("track_bilateral", d_rows, d_out, F, W, clip_frame_off, n_clips, radius, flags);
    if (rc < 0) return rc;
    if (!isfinite(distance_sigma) || distance_sigma <= 0.0 || !isfinite(range_sigma) || range_sigma <= 0.0)
        return sdfa_fail(SDFA_EINVAL, "track_bilateral: sigmas (%g, %g) must be finite and positive", distance_sigma, range_sigma);
    if (!isfinite(factor)) return sdfa_fail(SDFA_EINVAL, "track_bilateral: factor %g is not finite", factor);
    TFilterArgs a;
    memset(&a, 0, sizeof(a));
    a.x = d_rows;
    a.out = d_out;
    a.W = W;
    a.radius = radius;
    a.factor = factor;
    a.range_sigma = range_sigma;
    for (int d = -radius; d <= radius; ++d) {
        const double delta = (double)d / distance_sigma;
        a.w[d + radius] = dist_w ? dist_w[d + radius] : exp(delta * delta * factor);
    }
    return launch_all(a, TFILTER_BILATERAL, F, clip_frame_off, n_clips, flags, (hipStream_t)stream);
}

}  // extern "C"
