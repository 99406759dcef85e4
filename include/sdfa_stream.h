/* C ABI of live streaming inference in libsdfa_hip.so: audio that arrives in pieces, per stream, on the device.
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative SDFA_E* code on failure,
 * sdfa_last_error() describes the failure, device work is enqueued on `stream` and nothing here synchronises.
 * This surface is versioned on its own (SDFA_STREAM_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Contract.  Frame k of a clip covers the samples [s_k, e_k), e_k = s_k + sliding,
 * sliding = 63 hop + win (568 ms at 8 and 16 kHz).  A stream that has received n samples has made final exactly the frames
 * with e_k < n, none while n - 1 < sliding, and each is bit-identical to the same frame of the offline call on the whole
 * signal.  Why e_k < n and not e_k <= n: the offline front end transforms a column that ends exactly at the end of its clip
 * in another instruction form (clamped requests instead of one unclamped run), and at 16 kHz the two forms do not round
 * alike; one sample past the window settles which form the offline call takes.  Before n - 1 >= sliding the reference's
 * short-clip assert (SDFA_ESHORTCLIP) may still fire when the stream ends; after it cannot, so a final frame is never
 * withdrawn.  A frame stamped ts needs audio up to ts + 100 ms + sliding / 2 (+ one sample) = ts + 384 ms: that lag is set
 * by the model.  When a stream ends after n samples, its frame count is sdfa_frame_index(n) and the frames past the last
 * final one read zeros beyond n, as offline.
 *
 * Rings.  The samples of a stream live on the device in a ring of R = 2^r floats: absolute stream position p is
 * stored at p & (R - 1), and the first SDFA_STREAM_RING_MIRROR floats are repeated right behind the ring (so that the
 * samples of one STFT column are always contiguous).  The rings of a session are one array, ring i at
 * d_rings + i * (R + SDFA_STREAM_RING_MIRROR); sdfa_stream_ring_append keeps the mirror.  A VIEW of a ring is what a clip
 * is offline: (ring, delay, valid_hi) with frame starts in the ring's stream coordinates; a sample at position g reads as
 * zero outside [0, valid_hi).  The main signal of a stream that has received n samples (n = its length once it has
 * ended) is the view (ring, 0, n).  Its ensembling copy np.pad(signal[:-pad], [[pad, 0]]) (model.py:373-384) is the
 * view (ring, pad, max(n - pad, 0)) with frame starts s_k - pad: no copy of the samples is made.  Positions -pad .. -1
 * of a ring must hold zeros (append them ahead of a stream's first samples).  The caller keeps every sample a frame of
 * the call needs in its ring: [s - 1, valid_hi) of a frame at start s must not have been overwritten.
 *
 * A step costs one host -> device copy (new samples + segment table + frame table), sdfa_stream_ring_append and
 * sdfa_mel_frontend_ring, whatever the number of streams; the encoder and the regressor are the sdfa_hip.h calls.
 *
 * Capture-rate streams.  A stream may arrive at another rate than the model's (44.1 kHz, 48 kHz, ...).  Its samples are appended
 * to an INPUT ring (a second ring array with its own r_in, filled by sdfa_stream_ring_append) and sdfa_stream_resample converts
 * them into the stream's model ring with the arithmetic of sdfa_resample (sdfa_hip.h), one float32 multiply by a gain and a
 * clamp to +-0.999 on the store.  With tr(t) the time register of output t (0 for t = 0, += 1 / ratio per output, accumulated
 * sequentially in float64), n = int(tr(t)) and wing(t) = (nwin - offset) / step the taps of its right wing, output t is FINAL
 * after n_in received samples when n(t') + 1 + wing(t') <= n_in for every t' <= t: its right wing is complete and later samples
 * cannot change it.  A step converts exactly the final outputs not yet produced, and their count is the stream's model-rate
 * length for the frame rule above; when the stream ends after n_in samples the outputs up to int(n_in * ratio) are produced
 * with the truncated wings of the offline call, zeros follow up to ceil(n_in * ratio), and that is its model-rate length.  The
 * model ring then holds, position by position, clip(sdfa_resample(whole signal) * gain, -0.999, 0.999).  The input ring must
 * keep [n(t) - wing, n_in) for the first output t not yet produced: R_in >= 2 (nwin / step + 1) + samples between two steps + 1.
 */
#ifndef SDFA_STREAM_H
#define SDFA_STREAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_STREAM_ABI_VERSION 1
#define SDFA_STREAM_RING_MIRROR 2048   /* floats repeated behind each ring: >= win + 2 at 8 and 16 kHz */
#define SDFA_STREAM_MAX_RATES 8        /* distinct input rates one sdfa_stream_resample call takes */

int sdfa_stream_abi_version(void);

/* Window starts and timestamps of frames k0 .. k0 + count - 1 of any clip at this rate: the float32 arithmetic of
 * sdfa_frame_index (speech_anime/datasets/sliding_window.py:324-377: frame_to_sample, the window cut and sample_to_ms)
 * as a function of k alone, bit-equal to sdfa_frame_index's entries.  Either output may be NULL.  Returns count. */
int64_t sdfa_stream_frame_positions(int64_t k0, int64_t count, int sample_rate, int fps, int win, int hop, int ts_delta_ms,
                                    int64_t *h_starts, int32_t *h_tslist);

/* Number of FINAL frames of a stream that has received n_samples samples: #{k : e_k < n_samples}, 0 while
 * n_samples - 1 < sliding (sliding_window.py:324-377 with the short-clip assert of sliding_window.py:356-362 still open).
 * n_samples above 2^29 - 1 returns SDFA_EINVAL with sdfa_frame_index's message. */
int64_t sdfa_stream_final_frames(int64_t n_samples, int sample_rate, int fps, int win, int hop);

/* Ring append: d_seg holds n_seg segments of four int64 (ring, first absolute position, count, offset in d_src).  Segment
 * i writes d_src[off .. off + count) to ring `ring` at positions pos .. pos + count - 1 (each at position & (R - 1), and
 * into the mirror too when that is below SDFA_STREAM_RING_MIRROR); pos may be negative (the zeros ahead of a stream).
 * A segment whose ring lies outside [0, n_rings), whose count lies outside [0, R] or whose source range leaves
 * [0, n_src) is skipped.  Segments must not overlap in the same ring.  (No counterpart in the reference: it reads a
 * whole clip, speech_anime/model/model.py:373-384.) */
int sdfa_stream_ring_append(float *d_rings, int r, int32_t n_rings, const int64_t *d_seg, int32_t n_seg, const float *d_src,
                            int64_t n_src, void *stream);

/* The spectral-stream front end of sdfa_mel_frontend_gather over ring views: features (n_frames, 64, 128, 3) bit-equal to
 * sdfa_mel_frontend_gather's for the same samples (sliding_window.py:356-362 window cut, get_features.py:199-215).
 *   d_rings        n_rings rings of 2^r + SDFA_STREAM_RING_MIRROR floats, 2^r >= sliding, r <= 28
 *   d_view_ring    [n_views] int64 ring index | delay << 32        d_view_hi  [n_views] int64 valid_hi (< 2^29)
 *   d_frame_view   [n_frames] int32 view of each frame            d_frame_start [n_frames] int64 window start (stream coordinates)
 * The frames of a view should be consecutive and in increasing start order: hop-aligned frames of one view then share their
 * STFT columns, as frames of one clip do (Engine.last_frame_table: (d_frame_view, d_frame_start, hop) is the table the
 * column-sharing encoder takes).  d_workspace: sdfa_frontend_workspace_bytes(n_frames) bytes, 16-byte aligned; its status
 * word and repair pass are those of sdfa_mel_frontend_gather (sdfa_debug_frontend_status reads it).  Bit-equality holds for
 * the default offline transform (bitwise also the "frontend_two_kernel" / "frontend_t_major" forms); with the thread-local
 * "mel_fft_radix4" switch on at 16 kHz the call returns SDFA_EINVAL. */
int sdfa_mel_frontend_ring(const float *d_rings, int r, int32_t n_rings, const int64_t *d_view_ring, const int64_t *d_view_hi,
                           int32_t n_views, const int32_t *d_frame_view, const int64_t *d_frame_start, int64_t n_frames,
                           int sample_rate, float *d_audio_feat, void *d_workspace, int64_t workspace_bytes, void *stream);

/* Number of FINAL outputs of a stream at sr_in that has received n_in samples, at the model rate sr_out (the rule above); n_in when
 * the rates are equal.  Host only.  A rate pair that sdfa_resample refuses returns SDFA_EINVAL with its message. */
int64_t sdfa_stream_resample_final(int64_t n_in, int sr_in, int sr_out);

/* Time registers of `count` consecutive outputs: h_treg[i] (may be NULL) = the register of the i-th of them, *h_state = the register
 * of the first on entry (0.0 for output 0) and of the one after the last on return.  The sequential float64 accumulation of
 * sdfa_resample, so the register is a function of the output index alone however the calls are cut.  Host only.  Returns count. */
int64_t sdfa_stream_resample_register(int64_t count, int sr_in, int sr_out, double *h_state, double *h_treg);

/* Lengths of a stream that ended after n_in samples: returns n_out = sdfa_resample_out_len, *h_n_res = the outputs that are filtered
 * (zeros from there to n_out).  The refusals of sdfa_resample with their messages ("too small to resample").  Host only. */
int64_t sdfa_stream_resample_close(int64_t n_in, int sr_in, int sr_out, int64_t *h_n_res);

/* nwin / step of a rate pair: no wing of an output reaches further than this many input samples (+ 1 on the left, the sample at
 * n itself); 0 when the rates are equal.  Host only; the refusals of sdfa_resample_final. */
int64_t sdfa_stream_resample_wing(int sr_in, int sr_out);

/* Input rings -> model rings, every stream of a step in one launch.  d_seg holds n_seg segments of eight int64:
 *   input ring, model ring, t0, count, n_in, t_zero, offset in d_treg, rate index | (float32 bits of the gain) << 32
 * Segment j writes outputs t0 .. t0 + count - 1 of its stream to its model ring (each at t & (2^r - 1), and into the mirror when
 * that is below SDFA_STREAM_RING_MIRROR): zeros for t < 0 (the zeros ahead of an ensembling stream) and for t >= t_zero (pass n_res
 * once the stream has ended, INT64_MAX before), else the resampled sample from the n_in samples received so far, times the gain,
 * clamped.  d_treg[offset + i] is the register of output max(t0, 0) + i (sdfa_stream_resample_register), for the outputs below
 * t_zero.  h_rates (HOST) lists the n_rates <= SDFA_STREAM_MAX_RATES input rates the segments index; a rate equal to sr_out copies.
 * max_count >= every segment's count.  A segment with an index, count or register range outside its array is skipped.  Outputs
 * must be final (or the stream ended), and [n(t0) - wing, n_in) still in the input ring.  Never synchronises -- except that the
 * first call with a rate pair on a device builds and uploads that pair's filter table (sdfa_resample shares the tables). */
int sdfa_stream_resample(const float *d_in_rings, int r_in, int32_t n_in_rings, float *d_rings, int r, int32_t n_rings, const int64_t *d_seg,
                         int32_t n_seg, int64_t max_count, const double *d_treg, int64_t n_treg, const int32_t *h_rates, int32_t n_rates,
                         int sr_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
