/* C ABI of the batched baseline-JPEG encoder in libsdfa_hip.so (sdfa-2019_amd/csrc/jpeg.hip).
 *
 * It turns n (H, W, 3) uint8 RGB frames on the device (row 0 at the top, the layout sdfa_render_frames writes) into n
 * complete JPEG files, SOI to EOI, in one contiguous device buffer.  Each file is byte for byte the one PIL writes with
 * quality=q and every other option at its default (speech_anime.video.encode_jpeg, libjpeg-turbo underneath).
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative SDFA_E* code on failure,
 * sdfa_last_error() describes the failure, work is enqueued on `stream` and only the constructor synchronises.
 * This surface is versioned on its own (SDFA_JPEG_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Format contract (DESIGN.md "GPU JPEG"; tests/jpeg_oracle.py restates it in numpy):
 *   markers  SOI, APP0 JFIF 1.01 (density 1 x 1, unit 0), DQT 0, DQT 1, SOF0 (8-bit, components 1/2/3 sampled 2x2 /
 *            1x1 / 1x1 with tables 0/1/1), DHT DC0, AC0, DC1, AC1 (T.81 Annex K), SOS (3 components, 0..63), data, EOI;
 *            no restart interval
 *   quant    Annex K tables scaled by 5000/q % (q < 50) or 200 - 2q %, (base * scale + 50) / 100 clamped to 1 .. 255
 *   colour   Y = (19595 R + 38470 G + 7471 B + 2^15) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 2^15 - 1)
 *            >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 2^15 - 1) >> 16
 *   planes   Y by edge replication to whole 16 x 16 MCUs; chroma (sum of a 2 x 2 quad + 1, 2, 1, 2, ... along the row)
 *            >> 2 of the image padded to even height and whole MCU columns by replication, chroma rows past
 *            ceil(H / 2) repeating the last one; luma blocks outside ceil(W / 8) x ceil(H / 8) are "dummy": AC zero,
 *            DC that of the block before them in the MCU (Y01 -> Y00; Y10, Y11 below the image -> Y01; Y11 right of
 *            the image -> Y10)
 *   DCT      integer "islow" (13-bit constants, 2 pass bits) of the samples - 128; coefficient / (8 q) rounded half
 *            away from zero
 *   entropy  MCU raster, Y00 Y01 Y10 Y11 Cb Cr; DC difference to the previous block of the same component; AC run /
 *            size with ZRL and EOB; 0xFF followed by 0x00; the last byte padded with 1-bits
 *
 * Capacity.  A block codes to at most 1660 bits: a DC difference needs at most 11 magnitude bits and an 11-bit code
 * (chroma), an AC coefficient (|c| < 1024, the DCT of 8-bit samples) at most 10 bits and a 16-bit code, and 63 nonzero
 * coefficients (no ZRL, no EOB) is the longest block, 22 + 63 * 26.  Byte stuffing at most doubles the data, so
 *   sdfa_jpeg_max_frame_bytes = header + 2 * (ceil(1660 * n_blocks / 8) + 1) + 2,   n_blocks = 6 * MCUs.
 */
#ifndef SDFA_JPEG_H
#define SDFA_JPEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_JPEG_ABI_VERSION 1

#define SDFA_JPEG_MAX_SIDE        8192
#define SDFA_JPEG_MAX_BLOCK_BITS  1660    /* the worst-case coded length of one block (above) */
#define SDFA_JPEG_MAX_FRAMES      65535   /* frames per sdfa_jpeg_encode call */

typedef struct sdfa_jpeg_encoder sdfa_jpeg_encoder;

int sdfa_jpeg_abi_version(void);

/* width, height 1 .. 8192, quality 1 .. 100.  Builds the header and the tables and uploads them (synchronises
 * `stream`).  NULL on failure (sdfa_last_error()). */
sdfa_jpeg_encoder *sdfa_jpeg_create(int width, int height, int quality, void *stream);
void sdfa_jpeg_destroy(sdfa_jpeg_encoder *enc);

/* The header every file of this encoder starts with (SOI .. SOS): returns its length and copies
 * min(length, capacity) bytes into h_out unless h_out is NULL. */
int64_t sdfa_jpeg_header(const sdfa_jpeg_encoder *enc, uint8_t *h_out, int64_t capacity);

/* The per-frame capacity bound (above). */
int64_t sdfa_jpeg_max_frame_bytes(const sdfa_jpeg_encoder *enc);

/* Device workspace of one sdfa_jpeg_encode call of n frames. */
int64_t sdfa_jpeg_workspace_bytes(const sdfa_jpeg_encoder *enc, int64_t n);

/* d_rgb (n, height, width, 3) uint8 -> n JPEG files packed back to back into d_out, file i at byte d_offsets[i] and
 * d_lengths[i] bytes long (int64, device).  out_capacity must be at least n * sdfa_jpeg_max_frame_bytes; d_ws
 * (256-byte aligned) at least sdfa_jpeg_workspace_bytes(enc, n).  n == 0 is a no-op. */
int sdfa_jpeg_encode(sdfa_jpeg_encoder *enc, const uint8_t *d_rgb, int64_t n, uint8_t *d_out, int64_t out_capacity,
                     int64_t *d_offsets, int64_t *d_lengths, void *d_ws, int64_t ws_bytes, void *stream);

/* The transform stage alone: d_coefs (n, MCUs, 6, 64) int16, the quantised coefficients of each block in zigzag order,
 * MCUs in raster order and blocks Y00 Y01 Y10 Y11 Cb Cr, dummy blocks as coded. */
int sdfa_jpeg_debug_coefs(sdfa_jpeg_encoder *enc, const uint8_t *d_rgb, int64_t n, int16_t *d_coefs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
