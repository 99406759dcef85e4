/* C ABI of the conv stack's training step in libsdfa_hip.so (sdfa-2019_amd/csrc/convtrain.hip, api_convtrain.cpp): layers 1, 3 and
 * 5 of the reference's audio encoder (speech_anime/config/model/dgrad.py:62-64) -- three weight-normed convolutions along frequency,
 * each followed by LeakyReLU(0.2) and BatchNorm, with a max-pool of two behind the first two -- as a training forward that keeps
 * what the backward needs, the backward from dC down to the 15 parameter gradients, and one step of torch.optim.Adam (amsgrad off,
 * weight decay 0).  The stage that consumes the dC of an sdfa_freqtrain handle.  DESIGN.md section 22.
 *
 * Conventions are those of sdfa_hip.h and sdfa_freqtrain.h: every call returns >= 0 on success and a negative SDFA_E* code on
 * failure, sdfa_last_error() describes the failure.  Everything after finalize is stream-ordered; every refusal is decided before
 * any launch.  Versioned on its own (SDFA_CONVTRAIN_ABI_VERSION); SDFA_ABI_VERSION does not change.
 *
 * Shape     a frame has 64 columns (n, t); a column is 128 frequency bins of 3 channels; R = 64 N columns in a batch of N frames.
 *           Layer L of "_audio_encoder._layers" has (co, ci, kf) = (32, 3, 3) [L = 1], (64, 32, 3) [3], (64, 64, 1) [5]; frequency
 *           goes 128 -> 64 -> 32.
 * Tensors   named as the reference names them with "_model." stripped, per layer L in this order:
 *               "_audio_encoder._layers.L.weight_g"              [co][1][1][1]
 *               "_audio_encoder._layers.L.weight_v"              [co][ci][kf][1]
 *               "_audio_encoder._layers.L.bias"                  [co]
 *               "_audio_encoder._layers.L._ext_post_bn.weight"   [co]
 *               "_audio_encoder._layers.L._ext_post_bn.bias"     [co]
 *           15 trainable tensors, 11,168 elements, layer 1's five first.  Constants, required by finalize, held outside the flat
 *           buffers and never stepped:
 *               "_audio_encoder._layers.L._ext_post_bn.running_mean", "..._ext_post_bn.running_var"   [co]
 *           get_tensor(PARAM) returns a constant; every other `what`, set_grad and set_state on a constant is SDFA_EINVAL by name.
 * BatchNorm runs with its running statistics and eps 1e-3 (the inference form): the reference's train() mode, which normalises by
 *           batch statistics and moves the running ones with momentum 0.01, is not built.
 * State     flat float32 device buffers of parameters, gradients, exp_avg, exp_avg_sq (one layout: the tensors in the order
 *           above) and the step count on the host.  finalize uploads once; after it the parameters live on the device.
 * Forward   d_feat [N][64][128][3] row-major in (row (n, t) is 384 floats f 3 + c), d_C [N][64][32][64] out, the layout
 *           sdfa_encoder_conv writes and sdfa_freqtrain_forward reads.  Every column is evaluated.  Per layer, every step:
 *               W = g v / ||v||  (the norm over (ci, kf) per output channel; the fold launch of sdfa_headtrain.h)
 *               rstd = 1 / sqrtf(var + 1e-3f) ;  s = gamma rstd ;  t = fma(-mean, s, beta)
 *               a[f][co] = sum_{d, ci} W[co][ci][d] Xpad[f + d - kf/2][ci] + b[co]     (one chain, tap d outermost, ci ascending;
 *                                                                                       zero padding along frequency; then + b)
 *               y = a >= 0 ? a : 0.2f a ;  z = fma(y, s, t)
 *               layers 1 and 3:  p[f'] = z[2f' + 1] > z[2f'] ? z[2f' + 1] : z[2f']     (on equal values the first row wins)
 *           Layer 5's z is C.  Kept in the workspace, per frame: a of every layer (1 MiB, 1 MiB, 512 KiB) and the pooled p of
 *           layers 1 and 3 (512 KiB each).
 * Backward  given d_dC [N][64][32][64]; there is no input gradient.  Per layer from the top, dp being dC or the dX of the layer above:
 *               the winner of a pair and the side of the kink are RECOMPUTED from the kept a with the forward's own function on
 *               the forward's own operands (a, s, t): bit for bit the forward's decisions
 *               dz = dp at the row that won, 0 at the other ;  dbeta = sum dz ;  dgamma = sum dz ((y - mean) rstd)
 *               da = (dz s) (a > 0 ? 1 : 0.2f)       (slope 0.2 at a == 0) ;  db = sum da
 *               dW[co][ci][d] = sum_{column, f} da[f][co] Xpad[f + d - kf/2][ci]
 *               dX[f][ci] = sum_{d, co} W[co][ci][d] da_pad[f - d + kf/2][co]           (layers 3 and 5)
 *               dg = <dW, v> / ||v|| ;  dv = (g / ||v||)(dW - dg v / ||v||)             (the weight-norm launch of sdfa_headtrain.h)
 *           da overwrites the kept a.  The backward adds, per frame, dp of layers 1 and 3 and dz (y - mean) rstd of the three
 *           layers, 512 KiB each: 6 MiB per frame in all, 12 GiB at SDFA_CONVTRAIN_MAX_FRAMES.  Every index is formed in 64 bits.
 *           The call OVERWRITES the gradient buffer.  It consumes the kept a: a second backward needs a new forward.
 * Sums      no atomics, no workgroup waits on another.  All 15 gradients contract over the 64 N columns times the layer's
 *           frequency rows: they are formed per row block of SDFA_CONVTRAIN_BLOCK_FRAMES frames (a constant of the shape, not of
 *           the device) as float32 partials, every one an fp32 MFMA chain with its row index ascending (the bias and BatchNorm
 *           sums against a matrix of ones, layer 1's 32 x 9 dW included as three tiles), and added in ascending block order by a
 *           second launch.  Every sum's order depends on N alone: the same inputs give the same bits, and a frame's C does not
 *           depend on the other frames of the batch.
 * Adam      the kernel and the host arithmetic of sdfa_headtrain.h, through one shared launcher.
 * Launches  4 (forward: fold, layers 1, 3, 5) + 6 (backward: layer 5's da; dX of layer 5 with layer 3's da; dX of layer 3 with
 *           layer 1's da; products; reduce; weight norm) + 1 (Adam).
 */
#ifndef SDFA_CONVTRAIN_H
#define SDFA_CONVTRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_CONVTRAIN_ABI_VERSION 1

/* `what` of get_tensor / set_state */
#define SDFA_CONVTRAIN_PARAM      0
#define SDFA_CONVTRAIN_GRAD       1
#define SDFA_CONVTRAIN_EXP_AVG    2
#define SDFA_CONVTRAIN_EXP_AVG_SQ 3

#define SDFA_CONVTRAIN_COLUMNS 64            /* columns (n, t) of a frame */
#define SDFA_CONVTRAIN_BINS    128           /* frequency bins of a column of audio_feat */
#define SDFA_CONVTRAIN_IN      3             /* channels of a bin */
#define SDFA_CONVTRAIN_OUT_BINS 32           /* frequency rows of C */
#define SDFA_CONVTRAIN_OUT     64            /* channels of C */
#define SDFA_CONVTRAIN_NUMEL   11168         /* trainable elements */
#define SDFA_CONVTRAIN_BN_EPS  1e-3f
/* frames (512 columns) of one partial of the summed gradients.  The frequency trainer's: layer 1's chains then run over 65,536
 * rows (1,024 chunks of the tile routine), a batch of 100 frames is 13 row blocks of 16 tiles, about one workgroup per compute
 * unit, and a partial is 44 KB. */
#define SDFA_CONVTRAIN_BLOCK_FRAMES 8
#define SDFA_CONVTRAIN_MAX_FRAMES 2048       /* 6 MiB kept per frame: 12 GiB */

typedef struct sdfa_convtrain sdfa_convtrain;

int sdfa_convtrain_abi_version(void);

sdfa_convtrain *sdfa_convtrain_create(void);
void sdfa_convtrain_destroy(sdfa_convtrain *h);

/* Host float32 data of one tensor, trainable or constant, before finalize.  SDFA_EINVAL: unknown name, wrong numel, null;
 * SDFA_ESTATE: finalised. */
int sdfa_convtrain_set_tensor(sdfa_convtrain *h, const char *name, const float *h_src, int64_t numel);
/* Uploads the parameters and the constants, zeroes the gradients and both moments, step count 0.  SDFA_ESTATE names the first
 * missing tensor, the trainable ones first. */
int sdfa_convtrain_finalize(sdfa_convtrain *h, void *stream);

int64_t sdfa_convtrain_numel(const sdfa_convtrain *h);
/* Bytes of workspace a batch of up to max_frames frames needs; a multiple of 256. */
int64_t sdfa_convtrain_workspace_bytes(const sdfa_convtrain *h, int64_t max_frames);

/* Training forward: d_feat float32 [N][64][128][3] row-major, d_C float32 [N][64][32][64].  d_ws is 256-byte aligned device memory
 * of at least workspace_bytes(h, N). */
int sdfa_convtrain_forward(sdfa_convtrain *h, const float *d_feat, int64_t N, float *d_C, void *d_ws, int64_t ws_bytes, void *stream);
/* Backward of the last forward on this workspace and N, with the same d_feat: d_dC float32 [N][64][32][64]. */
int sdfa_convtrain_backward(sdfa_convtrain *h, const float *d_feat, const float *d_dC, int64_t N, void *d_ws, int64_t ws_bytes,
                            void *stream);
/* One optimiser step on the gradients the handle holds. */
int sdfa_convtrain_adam(sdfa_convtrain *h, double lr, double beta1, double beta2, double eps, void *stream);
int sdfa_convtrain_zero_grad(sdfa_convtrain *h, void *stream);

/* Access for tests and resume; these synchronise the device.  `name` as in set_tensor. */
int sdfa_convtrain_get_tensor(sdfa_convtrain *h, const char *name, int what, float *h_dst, int64_t numel);
int sdfa_convtrain_set_grad(sdfa_convtrain *h, const char *name, const float *h_src, int64_t numel);
int sdfa_convtrain_set_state(sdfa_convtrain *h, const char *name, int what, const float *h_src, int64_t numel);
int64_t sdfa_convtrain_step_count(const sdfa_convtrain *h);
int sdfa_convtrain_set_step_count(sdfa_convtrain *h, int64_t t);

/* Refused with SDFA_EINVAL before any launch: N < 1 or N > SDFA_CONVTRAIN_MAX_FRAMES, null pointers, a short or misaligned
 * workspace, backward without a forward on the same workspace and N, lr / betas / eps outside their ranges, anything but
 * get_tensor(PARAM) on a constant; with SDFA_ESTATE: a handle that is not finalised (finalize names the first missing tensor),
 * set_tensor after finalize. */

#ifdef __cplusplus
}
#endif
#endif
