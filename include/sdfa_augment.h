/* C ABI of the augmented training-window front end in libsdfa_hip.so (sdfa-2019_amd/csrc/frontend.hip
 * frontend_augment_kernel, api_augment.cpp): the TRAINING branch of the reference's windowed_features
 * (speech_anime/datasets/get_features.py:8-223) -- sdfa_hip.h covers its inference branch.  One workgroup builds one
 * (64, 128, 3) feature image from a window at an arbitrary sample offset.  DESIGN.md section 14.
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative SDFA_E* code on failure,
 * sdfa_last_error() describes the failure.  The surface is stateless.  It is versioned on its own
 * (SDFA_AUGMENT_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Stages of one window (hop = 0.008 sr, win = 0.064 sr, sliding = 63 hop + win):
 *   1  cut [start - ex_time hop, start + sliding + ex_time hop) from the clip, zeros outside it; add noise[i] to sample i
 *      of the cut (float32, one rounding); pre-emphasise y[i] = x[i] - preemph x[i-1] in float32 with y[0] = x[0]
 *      (get_features.py:57-87, saber/data/audio/features/misc.py:8-17).
 *   2  T = 64 + 2 ex_time STFT columns -> power -> mel -> dB -> (dB - 20 + 80) / 80 clamped to [0, 1]: the arithmetic of
 *      sdfa_mel_frontend, its columns paired by the absolute hop index of the cut's first sample.
 *   3  frequency edit (get_features.py:125-140), never materialised: ex_feat < 0 drops |ex_feat| mel rows, the low ones
 *      with lower_freq, else the high ones; ex_feat > 0 pads ex_feat rows, zeros below with lower_freq, else above --
 *      np.pad's "reflect" (extended row 128 + j = row 126 - j) with pad_reflect, zeros without --, and with trunck the
 *      same number of rows is cut from the other end.  R = 128 - |ex_feat|, 128 or 128 + ex_feat rows.
 *   4  bilinear resize (R x T) -> (128 x 64) by OpenCV's INTER_LINEAR rule for float images: source coordinate
 *      (d + 0.5) (n_in / n_out) - 0.5 in double, rounded to float32; floor; the fraction in float32; both ends clamped
 *      with fraction 0; time axis first, v[x0] (1 - fx) + v[x1] fx, then the frequency axis; every product and sum
 *      rounded on its own.  No antialiasing.  R = 128, T = 64 is the identity.
 *   5  times scale[row] in float32; then the rows of `drop` are set to 0.
 *   6  deltas of width 9 over the 64 columns and the [64][128][3] store of sdfa_mel_frontend.
 * A neutral descriptor (ex_time = ex_feat = 0, preemph = 0.65f, empty drop, no noise, no scale) gives sdfa_mel_frontend's
 * rows bit for bit.
 *
 * Deviations from the reference's NumPy, on purpose:
 *   - `feat *= feat_scale` multiplies in double there (the scale array is float64) and rounds once; here the scale is
 *     rounded to float32 first and the product is a float32 one.
 *   - drop_mode == "max" does nothing in the reference: `feat[mask_idx][where] = mask_thres` assigns into the copy that
 *     the fancy index made (get_features.py:191-192).  The host therefore passes an empty mask for it.
 * Not built: feat_tremolo, feat_noise and pink noise (both model configurations leave them off), phoneme labels, and
 * the reverberated / pitch-shifted sources, which are precomputed audio, not an operation.
 */
#ifndef SDFA_AUGMENT_H
#define SDFA_AUGMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_AUGMENT_ABI_VERSION 1

#define SDFA_AUGMENT_EX_TIME_MAX 4        /* |ex_time| <= 4: 56 .. 72 STFT columns */
#define SDFA_AUGMENT_EX_FEAT_MAX 5        /* |ex_feat| <= 5: 123 .. 133 mel rows */
#define SDFA_AUGMENT_LOWER_FREQ  1u       /* flags: edit the low end of the mel axis */
#define SDFA_AUGMENT_TRUNCK      2u       /* flags: after padding, cut as many rows from the other end */
#define SDFA_AUGMENT_PAD_REFLECT 4u       /* flags: pad above by reflection (else zeros) */

/* One window; 48 bytes, uploaded as an array. */
typedef struct sdfa_augment_desc {
    int32_t clip;        /* clip index, 0 .. n_clips - 1 */
    int32_t ex_time;     /* -4 .. 4 */
    int64_t start;       /* the unextended window's first sample `l` in the clip's samples; may be negative */
    float preemph;       /* pre-emphasis coefficient; 0 = none */
    int32_t ex_feat;     /* -5 .. 5 */
    uint32_t flags;      /* SDFA_AUGMENT_LOWER_FREQ | SDFA_AUGMENT_TRUNCK | SDFA_AUGMENT_PAD_REFLECT */
    uint32_t reserved;   /* 0 */
    uint32_t drop[4];    /* bit (r & 31) of drop[r >> 5]: output mel row r is zeroed */
} sdfa_augment_desc;

int sdfa_augment_abi_version(void);

/* Samples of the longest cut (ex_time = 4): 71 hop + win.  noise_stride must be at least this.  SDFA_EINVAL for a rate
 * other than 8000 / 16000. */
int64_t sdfa_augment_noise_samples(int sample_rate);

/* Host check of descriptors before they are uploaded: SDFA_EINVAL for ex_time or ex_feat out of range, unknown flag
 * bits, a non-zero reserved word, a non-finite preemph, a negative clip index, and -- when h_clip_len [n_clips] (HOST
 * memory) is given -- a clip index >= n_clips or a clip of more than 2^29 - 1 samples.  h_clip_len may be null. */
int sdfa_augment_check(const sdfa_augment_desc *h_desc, int64_t n, const int64_t *h_clip_len, int32_t n_clips);

/* The feature images.  d_pcm, d_clip_off [n_clips], d_clip_len [n_clips] as for sdfa_mel_frontend; d_desc [n];
 * d_noise [n][noise_stride] float32 or null; d_scale [n][128] float32 or null; d_audio_feat [n][64][128][3].  All device
 * memory.  Stream-ordered, no workspace, nothing is copied and nothing synchronises.
 * SDFA_EINVAL before any launch: a rate other than 8000 / 16000, null pointers, n < 0 or n > 2^31 - 1, n_clips <= 0,
 * d_noise with noise_stride < sdfa_augment_noise_samples(sample_rate).  The descriptors are device memory and are not
 * read by the host (sdfa_augment_check does that before the upload); the kernel itself clamps ex_time and ex_feat into
 * their ranges and treats a clip index outside 0 .. n_clips - 1 as an empty clip, so that no descriptor can make it
 * read or write out of bounds. */
int sdfa_augment_frontend(const float *d_pcm, const int64_t *d_clip_off, const int64_t *d_clip_len, int32_t n_clips,
                          const sdfa_augment_desc *d_desc, int64_t n, int sample_rate, const float *d_noise,
                          int64_t noise_stride, const float *d_scale, float *d_audio_feat, void *stream);

#ifdef __cplusplus
}
#endif
#endif
