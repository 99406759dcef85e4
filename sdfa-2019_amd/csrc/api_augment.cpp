// Host side of the augmented training-window front end (include/sdfa_augment.h): the refusals and the
// launch of frontend_augment_kernel (frontend.hip).  Nothing here copies or synchronises.
#include "../../include/sdfa_augment.h"
#include "host.h"
#include "kernels.h"

#include <cmath>

static_assert(sizeof(sdfa_augment_desc) == 48, "sdfa_augment_desc is uploaded as an array of 48-byte records");

namespace {

int geometry(const char *who, int sample_rate, int *win, int *hop) {
    if (sample_rate != 8000 && sample_rate != 16000)
        return sdfa_fail(SDFA_EINVAL, "%s: sample_rate %d unsupported: the FFT kernels cover 8000 (win 512) and 16000 (win 1024)", who, sample_rate);
    *win = sample_rate == 8000 ? 512 : 1024;
    *hop = *win / 8;
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_augment_abi_version(void) { return SDFA_AUGMENT_ABI_VERSION; }

int64_t sdfa_augment_noise_samples(int sample_rate) {
    int win, hop;
    if (int rc = geometry("augment_noise_samples", sample_rate, &win, &hop)) return rc;
    return (int64_t)(64 + 2 * SDFA_AUGMENT_EX_TIME_MAX - 1) * hop + win;
}

int sdfa_augment_check(const sdfa_augment_desc *h_desc, int64_t n, const int64_t *h_clip_len, int32_t n_clips) {
    if (n < 0 || (n > 0 && !h_desc)) return sdfa_fail(SDFA_EINVAL, "augment_check: null descriptors or a negative count");
    if (h_clip_len) {
        if (n_clips <= 0) return sdfa_fail(SDFA_EINVAL, "augment_check: clip lengths given for %d clips", (int)n_clips);
        // the clip's samples are addressed as the rest of the front end addresses them (sdfa_frame_index refuses the same lengths)
        for (int32_t c = 0; c < n_clips; ++c)
            if (h_clip_len[c] < 0 || h_clip_len[c] > 0x1fffffff)
                return sdfa_fail(SDFA_EINVAL, "augment_check: clip %d has %lld samples, outside 0 .. 2^29 - 1", (int)c, (long long)h_clip_len[c]);
    }
    const uint32_t known = SDFA_AUGMENT_LOWER_FREQ | SDFA_AUGMENT_TRUNCK | SDFA_AUGMENT_PAD_REFLECT;
    for (int64_t i = 0; i < n; ++i) {
        const sdfa_augment_desc &d = h_desc[i];
        if (d.ex_time < -SDFA_AUGMENT_EX_TIME_MAX || d.ex_time > SDFA_AUGMENT_EX_TIME_MAX)
            return sdfa_fail(SDFA_EINVAL, "augment_check: window %lld: ex_time %d outside -%d .. %d", (long long)i, (int)d.ex_time, SDFA_AUGMENT_EX_TIME_MAX, SDFA_AUGMENT_EX_TIME_MAX);
        if (d.ex_feat < -SDFA_AUGMENT_EX_FEAT_MAX || d.ex_feat > SDFA_AUGMENT_EX_FEAT_MAX)
            return sdfa_fail(SDFA_EINVAL, "augment_check: window %lld: ex_feat %d outside -%d .. %d", (long long)i, (int)d.ex_feat, SDFA_AUGMENT_EX_FEAT_MAX, SDFA_AUGMENT_EX_FEAT_MAX);
        if (d.flags & ~known) return sdfa_fail(SDFA_EINVAL, "augment_check: window %lld: unknown flag bits 0x%x", (long long)i, (unsigned)(d.flags & ~known));
        if (d.reserved != 0) return sdfa_fail(SDFA_EINVAL, "augment_check: window %lld: reserved word is not 0", (long long)i);
        if (!std::isfinite(d.preemph)) return sdfa_fail(SDFA_EINVAL, "augment_check: window %lld: preemph is not finite", (long long)i);
        if (d.clip < 0 || (h_clip_len && d.clip >= n_clips))
            return sdfa_fail(SDFA_EINVAL, "augment_check: window %lld: clip %d outside 0 .. %d", (long long)i, (int)d.clip, (int)n_clips - 1);
    }
    return SDFA_OK;
}

int sdfa_augment_frontend(const float *d_pcm, const int64_t *d_clip_off, const int64_t *d_clip_len, int32_t n_clips,
                          const sdfa_augment_desc *d_desc, int64_t n, int sample_rate, const float *d_noise, int64_t noise_stride,
                          const float *d_scale, float *d_audio_feat, void *stream) {
    int win, hop;
    if (int rc = geometry("augment_frontend", sample_rate, &win, &hop)) return rc;
    if (n < 0 || n > 0x7fffffffll) return sdfa_fail(SDFA_EINVAL, "augment_frontend: %lld windows outside 0 .. 2^31 - 1", (long long)n);
    if (d_noise && noise_stride < sdfa_augment_noise_samples(sample_rate))
        return sdfa_fail(SDFA_EINVAL, "augment_frontend: noise_stride %lld, at least %lld (71 hop + win) needed", (long long)noise_stride,
                         (long long)sdfa_augment_noise_samples(sample_rate));
    if (n == 0) return SDFA_OK;
    if (!d_pcm || !d_clip_off || !d_clip_len || !d_desc || !d_audio_feat || n_clips <= 0)
        return sdfa_fail(SDFA_EINVAL, "augment_frontend: null pointer or bad count");
    FrontendConsts c;
    if (int rc = sdfa_frontend_consts(sample_rate, c)) return rc;
    HIP_TRY(sdfa_launch_augment(c, d_pcm, d_clip_off, d_clip_len, n_clips, d_desc, n, d_noise, noise_stride, d_scale, d_audio_feat,
                                (hipStream_t)stream));
    return SDFA_OK;
}

}  // extern "C"
