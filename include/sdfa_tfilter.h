/* C ABI of the temporal track filters in libsdfa_hip.so (sdfa-2019_amd/csrc/tfilter.hip, api_tfilter.cpp): a thread walks a
 * column of a batch of per-frame rows through time with a window of neighbouring frames.  Two filters:
 *   sdfa_track_fir        a symmetric FIR with reflect boundaries, bit for bit scipy.ndimage.correlate1d(mode="reflect") on
 *                         float32 input with symmetric float64 weights, hence gaussian_filter1d -- the smoothing step of the
 *                         reference's generate_dgrad (speech_anime/datasets/vocaset/preload.py:819);
 *   sdfa_track_bilateral  the reference's BilateralFilter1D (saber/utils/bilateral.py:56-73), evaluated in double.
 * DESIGN.md section 13.
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative SDFA_E* code on failure,
 * sdfa_last_error() describes the failure.  The surface is stateless.  It is versioned on its own
 * (SDFA_TFILTER_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Rows      rows and out are device float32 [F][W], row stride W; the frames of all clips one after the other.  They
 *           must not overlap (refused).
 * Clips     clip_frame_off[n_clips + 1], HOST memory, ascending from 0 to F, no empty clip: clip c owns frames
 *           clip_frame_off[c] .. clip_frame_off[c + 1] - 1.  NULL: one clip of F frames (n_clips is ignored).  Host memory,
 *           like sdfa_score_rows's: every refusal is decided before anything is launched.  The offsets reach the device
 *           inside kernel arguments, SDFA_TFILTER_CLIPS clips per launch; no copy is enqueued.  A filter never reads
 *           across a clip boundary.
 * Flags     bit 0 (SDFA_TFILTER_GENERIC): use the generic form.  Any other bit is refused.
 * Forms     a register-window form (radius a compile-time parameter, 1 .. SDFA_TFILTER_WINDOW_RADIUS: a thread keeps the
 *           2 r + 1 frames of its columns in registers and fetches one new frame per output frame) and a generic form (any
 *           radius up to SDFA_TFILTER_MAX_RADIUS: every output frame re-reads its neighbours through the cache).  Both
 *           evaluate the same expression in the same order and agree bit for bit.
 * Tiling    grid = (slabs of SDFA_TFILTER_COLS columns) x (runs of SDFA_TFILTER_RUN consecutive frames of the batch).  A
 *           run starts its window afresh, re-reading up to 2 r halo frames; a clip that begins inside a run restarts the
 *           window there.  No atomics, no LDS, no barrier, no workgroup waits on another: the same inputs give the same bits.
 * Stream    nothing is copied, nothing synchronises.
 */
#ifndef SDFA_TFILTER_H
#define SDFA_TFILTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_TFILTER_ABI_VERSION 1

#define SDFA_TFILTER_MAX_RADIUS    32     /* taps: at most 65 */
#define SDFA_TFILTER_WINDOW_RADIUS 8      /* largest radius of the register-window form */
#define SDFA_TFILTER_COLS          1024   /* columns per slab: 256 threads x 4 columns */
#define SDFA_TFILTER_RUN           32     /* frames per run */
#define SDFA_TFILTER_CLIPS         512    /* clips per launch */
#define SDFA_TFILTER_GENERIC       1      /* flags bit 0 */

int sdfa_tfilter_abi_version(void);

/* Symmetric FIR, reflect boundaries (d c b a | a b c d | d c b a) inside each clip.  taps: HOST memory, 2 radius + 1
 * doubles, bitwise symmetric.  Per element, everything in double, no multiply and add contracted:
 *     acc = x[f] w[r];   for i = -r .. -1:  acc = acc + (x[refl(f + i)] + x[refl(f - i)]) w[i + r];   out = float32(acc)
 *     refl(i) = (j = i mod 2 F_c) < F_c ? j : 2 F_c - 1 - j     with F_c the clip's length (any depth of reflection)
 * radius 0 is x[f] w[0].  NaN and Inf propagate as the arithmetic dictates.
 * Refused with SDFA_EINVAL before any launch: null rows / out / taps, F outside 1 .. 65535 SDFA_TFILTER_RUN, W outside
 * 1 .. 2^30, radius outside 0 .. SDFA_TFILTER_MAX_RADIUS, taps that are not bitwise symmetric, overlapping rows and out,
 * offsets that do not run from 0 to F, an empty clip, unknown flag bits. */
int sdfa_track_fir(const float *d_rows, float *d_out, int64_t F, int64_t W, const int64_t *clip_frame_off, int64_t n_clips,
                   const double *taps, int radius, int flags, void *stream);

/* The reference's bilateral filter.  Per element, in double, for d = -radius .. radius ascending, skipping f + d outside
 * the clip (truncation, no reflection), nothing contracted:
 *     delta = x[f] - x[f + d];  s = sqrt(delta delta) / range_sigma;  sw = exp(s s factor);  wt = dw[d + radius] sw
 *     ws = ws + wt;  mean = mean + wt x[f + d];                       out = float32(mean / ws)
 * dist_w: HOST memory, 2 radius + 1 doubles dw[d + radius] = exp((d / distance_sigma)^2 factor), as the caller's own exp
 * forms them (sdfa_amd.tfilter passes Python's math.exp values, the reference's table); NULL: formed here with the C
 * library's exp.
 * Refused with SDFA_EINVAL before any launch: what sdfa_track_fir refuses (without the taps), a distance_sigma or range_sigma
 * that is not finite and positive, a factor that is not finite. */
int sdfa_track_bilateral(const float *d_rows, float *d_out, int64_t F, int64_t W, const int64_t *clip_frame_off, int64_t n_clips,
                         double factor, double distance_sigma, double range_sigma, int radius, const double *dist_w, int flags,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
