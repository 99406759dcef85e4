/* C ABI of the validation losses in libsdfa_hip.so (sdfa-2019_amd/csrc/score.hip, api_score.cpp): what the reference's
 * get_loss (speech_anime/model/model.py:261-330) computes with PLoss and MLoss (speech_anime/model/criterion.py:7-73) for
 * prediction_type "face_data", as per-frame sums of squares that one kernel forms from the prediction rows and the
 * ground-truth track.  The truth rows never exist in memory.  DESIGN.md section 12.
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative SDFA_E* code on failure,
 * sdfa_last_error() describes the failure.  The surface is stateless.  It is versioned on its own
 * (SDFA_SCORE_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Track     R: device float32 rows [n_track][W], row stride W: a clip's animation frames at the track's rate.
 * Pred      p: device float32 rows [F][W], row stride W, as sdfa_regress_forward writes them; the frames of all clips one
 *           after the other.
 * Clips     clip_frame_off[n_clips + 1], HOST memory, ascending from 0 to F: clip c owns frames clip_frame_off[c] ..
 *           clip_frame_off[c + 1] - 1.  (Host memory, like sdfa_pca_fit's chunk_rows: the refusals below are decided
 *           before anything is launched.  The offsets reach the device inside kernel arguments; no copy is enqueued.)
 * Truth     a plan in the layout of sdfa_seek_plan: src[f][2] int64 and w[f][2] float32, both on the device.
 *               t[f][j] = fl(fl(w0 * R[s0][j]) + fl(w1 * R[s1][j]))
 *           three separately rounded float32 operations, never contracted: bit for bit what sdfa_seek_rows writes.
 *           The plan restates the reference's get_anime (datasets/sliding_window.py:205-227) for the window (l, r) =
 *           (start, start + sliding) of a frame, every operation in float32 as NumPy evaluates that code on float32 scalars:
 *               ts = float32((l + r) / 2 * 1000 / sr) - ts_delta + start_ts        pos = ts * fps / 1000
 *               lower = floor(pos), upper = lower + 1; lower < anime_minfi: both = anime_minfi; else upper > anime_maxfi:
 *               both = anime_maxfi;  a = pos - lower (with the clamped lower);  w = (float32(1 - a), float32(a)), 1 - a in double
 *           sdfa_amd.score.truth_plan computes it on the host.
 * Record    double out[F][4].  e(x) = expf(x) on the columns j % 9 >= 6 (rotat) of layout dgrad -- the accurate expf,
 *           never the hardware approximation -- and e(x) = x everywhere else.  Every difference is one float32
 *           subtraction, as the reference forms it; its square and every sum are double.
 *               out[f][0] = sum over scale columns (all columns for plain) of fl(p - t)^2
 *               out[f][1] = sum over rotat columns of fl(e(p) - e(t))^2                                  (0 for plain)
 *               out[f][2], out[f][3] = the same two column sets of
 *                           fl( fl(e(p_f) - e(p_f-1)) - fl(e(t_f) - e(t_f-1)) )^2, 0 on a clip's first frame
 * Bad plan  a src index outside 0 .. n_track - 1 is never read: all four slots of that frame are NaN, and so are the
 *           motion slots (2 and, for dgrad, 3) of the next frame of its clip, which has no predecessor truth.
 *           (sdfa_mesh_deform_grad treats a bad face index the same way.)
 * Sums      a frame's columns are cut into slabs of SDFA_SCORE_COLS, a slab into 4 parts (one per wavefront); every part
 *           adds its squares in a fixed order, the parts go to the workspace as double and a second kernel adds them in
 *           ascending order.  No atomics: the same inputs give the same bits.  No workgroup waits on another.
 * Tiling    grid = (column slabs) x (runs of SDFA_SCORE_RUN consecutive frames of the batch).  A thread keeps e(p) and
 *           e(t) of the previous frame of its columns in registers; only a run's first frame fetches its predecessor again
 *           (unless it starts a clip).  A clip that begins inside a run restarts the chain there.
 * Scalars   the reference's scalar_* values follow from the records in float64 on the host (sdfa_amd.score.clip_scalars).
 * Absent    ELoss (this model emits no evector) and DynamicLossScaler (its state is not in a checkpoint).
 */
#ifndef SDFA_SCORE_H
#define SDFA_SCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_SCORE_ABI_VERSION 1

#define SDFA_SCORE_LAYOUT_DGRAD 0      /* W = 9 T: per triangle six scale and three rotat values */
#define SDFA_SCORE_LAYOUT_PLAIN 1      /* any W: the offsets head */

#define SDFA_SCORE_COLS  9216          /* columns per slab: 256 threads x 36 columns; a multiple of 9 */
#define SDFA_SCORE_RUN   32            /* frames per run */
#define SDFA_SCORE_PARTS 4             /* partial sums per slab and frame */

int sdfa_score_abi_version(void);

/* Device workspace of one sdfa_score_rows call, a multiple of 256 bytes; SDFA_EINVAL for F < 2, W < 1, an unknown layout
 * or W % 9 != 0 for dgrad. */
int64_t sdfa_score_workspace_bytes(int64_t F, int64_t W, int layout);

/* Scores.  d_pred [F][W], d_track [n_track][W], d_src [F][2], d_w [F][2] and d_out [F][4] are device memory, d_ws is
 * 256-byte aligned device memory of at least sdfa_score_workspace_bytes(F, W, layout); clip_frame_off is host memory.
 * Stream-ordered: nothing is copied, nothing synchronises.
 * Refused with SDFA_EINVAL before any launch: a clip with fewer than 2 frames, offsets that do not run from 0 to F,
 * W % 9 != 0 for dgrad, an unknown layout, n_track < 1, null pointers, a short or misaligned workspace. */
int sdfa_score_rows(const float *d_pred, int64_t F, int64_t W, int layout, const float *d_track, int64_t n_track,
                    const int64_t *d_src, const float *d_w, const int64_t *clip_frame_off, int64_t n_clips, double *d_out,
                    void *d_ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
