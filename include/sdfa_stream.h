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
 */
#ifndef SDFA_STREAM_H
#define SDFA_STREAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_STREAM_ABI_VERSION 1
#define SDFA_STREAM_RING_MIRROR 2048   /* floats repeated behind each ring: >= win + 2 at 8 and 16 kHz */

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

#ifdef __cplusplus
}
#endif
#endif
