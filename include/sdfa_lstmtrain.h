/* C ABI of one bidirectional LSTM layer's training step in libsdfa_hip.so (sdfa-2019_amd/csrc/lstmtrain.hip, api_lstmtrain.cpp):
 * a layer of the reference's torch.nn.LSTM(256, 256, num_layers=2, bias=False, bidirectional=True) (speech_anime/layers/rnn.py,
 * layer 9 of the audio encoder) as a training forward that keeps what the backward needs, back-propagation through time down to
 * dX, and one step of torch.optim.Adam (amsgrad off, weight decay 0).  The layer that consumes the dH of sdfa_attntrain.h.
 * DESIGN.md section 18.
 *
 * Conventions are those of sdfa_hip.h and sdfa_attntrain.h: every call returns >= 0 on success and a negative SDFA_E* code on
 * failure, sdfa_last_error() describes the failure.  Everything after finalize is stream-ordered; every refusal is decided before
 * any launch.  Versioned on its own (SDFA_LSTMTRAIN_ABI_VERSION); SDFA_ABI_VERSION does not change.
 *
 * Shape     T = 64 steps per frame, 256 hidden units per direction, input width I = 256 (layer 0) or 512 (layer 1), fixed at
 *           create.  No biases, gate order i, f, g, o, h_{-1} = c_{-1} = 0.  No dropout: the caller applies the inter-layer mask.
 * Tensors   named as the reference names them with "_model." stripped, layer = 0 for I = 256 and 1 for I = 512:
 *               "_audio_encoder._layers.9.weight_ih_l{layer}", "..._reverse"   [1024][I]
 *               "_audio_encoder._layers.9.weight_hh_l{layer}", "..._reverse"   [1024][256]
 *           1,048,576 elements for layer 0 and 1,572,864 for layer 1.
 * State     flat float32 device buffers of parameters, gradients, exp_avg, exp_avg_sq (one layout: W_ih, W_ih reverse, W_hh, W_hh
 *           reverse) and the step count on the host.  finalize uploads once; after it the parameters live on the device.
 * Forward   d_X [N][64][I] row-major in, d_Y [N][64][512] out: the forward direction's h in columns 0 .. 255, the reverse
 *           direction's in 256 .. 511 (nn.LSTM's layout).
 *               pre[d]  = X W_ih[d]^T
 *               per direction, over its own step order (forward: t = 0 .. 63, reverse: t = 63 .. 0):
 *                   pre_t += W_hh[d] h_prev ;  i, f, o = sigmoid, g = tanh (sigmoidf_acc / tanhf_acc of csrc/common.h)
 *                   c_t = fma(f, c_prev, i g) ;  h_t = o tanh(c_t)
 *           Kept in the workspace: the activated gates [2][N][64][1024] and c [2][N][64][256], 640 KiB per frame.  Every
 *           contraction is an fp32 MFMA chain with its index ascending; a step's chain starts from pre_t.
 * Backward  given d_dY [N][64][512]; per direction in reverse step order, dh_t = dY_t + dh_rec and a carried dc:
 *               do = dh tanh(c_t) o(1 - o) ;  dc += dh o fma(-tanh(c_t), tanh(c_t), 1)
 *               di = dc g i(1 - i) ;  df = dc c_{t-1} f(1 - f) ;  dg = dc i fma(-g, g, 1)
 *               dh_rec = W_hh^T [di|df|dg|do] ;  dc <- dc f
 *           c_{t-1} is 0 at a direction's first step.  The pre-activation gradients dG overwrite the kept gates.  Then
 *               dW_ih[d] = sum_{n,t} dG_t X_t^T ;  dW_hh[d] = sum_{n,t} dG_t h_{prev(t)}^T ;  dX = sum_d dG[d] W_ih[d]
 *           h_{prev(t)} is read from Y one step back in the direction's order and is zero at its first step.  dX contracts over
 *           both directions' 2,048 gate rows in one chain, forward direction first.  The parameter gradients are summed over the N
 *           frames; the call OVERWRITES the gradient buffer.  A null d_dX skips the dX tiles and changes no other output.  The
 *           backward consumes the kept gates: a second backward needs a new forward.
 * Sums      no atomics, no workgroup waits on another: one workgroup per (direction, tile of SDFA_LSTMTRAIN_TILE_FRAMES frames)
 *           in both recurrences.  dW_ih and dW_hh contract over all 64 N rows: they are formed per row block of
 *           SDFA_LSTMTRAIN_BLOCK_FRAMES frames (a constant of the shape, not of the device) as float32 partials and added in
 *           ascending block order by a second launch.  Every sum's order depends on N alone: the same inputs give the same bits,
 *           and a frame's Y and dX do not depend on the other frames of the batch.
 * Adam      the kernel and the host arithmetic of sdfa_headtrain.h, through one shared launcher.
 * Launches  3 (forward: weight images, pre, recurrence) + 3 (backward: recurrence, products, reduce) + 1 (Adam) = 7.
 */
#ifndef SDFA_LSTMTRAIN_H
#define SDFA_LSTMTRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_LSTMTRAIN_ABI_VERSION 1

/* `what` of get_tensor / set_state */
#define SDFA_LSTMTRAIN_PARAM      0
#define SDFA_LSTMTRAIN_GRAD       1
#define SDFA_LSTMTRAIN_EXP_AVG    2
#define SDFA_LSTMTRAIN_EXP_AVG_SQ 3

#define SDFA_LSTMTRAIN_STEPS  64            /* time steps of a frame */
#define SDFA_LSTMTRAIN_HIDDEN 256           /* hidden units of a direction */
#define SDFA_LSTMTRAIN_GATES  1024          /* gate rows of a direction: i, f, g, o */
#define SDFA_LSTMTRAIN_TILE_FRAMES 32       /* frames of one workgroup of a recurrence */
#define SDFA_LSTMTRAIN_BLOCK_FRAMES 32      /* frames (2,048 rows) of one partial of dW_ih, dW_hh: a partial is 4 - 6 MB */
#define SDFA_LSTMTRAIN_MAX_FRAMES 3072      /* 640 KiB kept per frame: 1.9 GiB, offsets of a tile stay below 2^31 floats */

typedef struct sdfa_lstmtrain sdfa_lstmtrain;

int sdfa_lstmtrain_abi_version(void);

/* in_dim 256 (layer 0) or 512 (layer 1); anything else: null, SDFA_EINVAL in sdfa_last_error(). */
sdfa_lstmtrain *sdfa_lstmtrain_create(int in_dim);
void sdfa_lstmtrain_destroy(sdfa_lstmtrain *h);

/* Host float32 data of one tensor, before finalize.  SDFA_EINVAL: unknown name, wrong numel, null; SDFA_ESTATE: finalised. */
int sdfa_lstmtrain_set_tensor(sdfa_lstmtrain *h, const char *name, const float *h_src, int64_t numel);
/* Uploads the parameters, zeroes the gradients and both moments, step count 0.  SDFA_ESTATE names the first missing tensor. */
int sdfa_lstmtrain_finalize(sdfa_lstmtrain *h, void *stream);

int64_t sdfa_lstmtrain_numel(const sdfa_lstmtrain *h);
/* Bytes of workspace a batch of up to max_frames frames needs; a multiple of 256. */
int64_t sdfa_lstmtrain_workspace_bytes(const sdfa_lstmtrain *h, int64_t max_frames);

/* Training forward: d_X float32 [N][64][I] row-major, d_Y float32 [N][64][512].  d_ws is 256-byte aligned device memory of at
 * least workspace_bytes(h, N). */
int sdfa_lstmtrain_forward(sdfa_lstmtrain *h, const float *d_X, int64_t N, float *d_Y, void *d_ws, int64_t ws_bytes, void *stream);
/* Backward of the last forward on this workspace and N, with the same d_X and its d_Y: d_dY float32 [N][64][512]; d_dX float32
 * [N][64][I] or null. */
int sdfa_lstmtrain_backward(sdfa_lstmtrain *h, const float *d_X, const float *d_Y, const float *d_dY, int64_t N, float *d_dX,
                            void *d_ws, int64_t ws_bytes, void *stream);
/* One optimiser step on the gradients the handle holds. */
int sdfa_lstmtrain_adam(sdfa_lstmtrain *h, double lr, double beta1, double beta2, double eps, void *stream);
int sdfa_lstmtrain_zero_grad(sdfa_lstmtrain *h, void *stream);

/* Access for tests and resume; these synchronise the device.  `name` as in set_tensor. */
int sdfa_lstmtrain_get_tensor(sdfa_lstmtrain *h, const char *name, int what, float *h_dst, int64_t numel);
int sdfa_lstmtrain_set_grad(sdfa_lstmtrain *h, const char *name, const float *h_src, int64_t numel);
int sdfa_lstmtrain_set_state(sdfa_lstmtrain *h, const char *name, int what, const float *h_src, int64_t numel);
int64_t sdfa_lstmtrain_step_count(const sdfa_lstmtrain *h);
int sdfa_lstmtrain_set_step_count(sdfa_lstmtrain *h, int64_t t);

/* The frozen encoder's forward (sdfa_encoder_memory of sdfa_attntrain.h, same arguments and refusals) up to and including layer 0 of
 * the BiLSTM: d_X1 float32 [n_frames][64][512] row-major, what layer 1 reads, for every frame.  No layer 1 and no attention are
 * launched.  Not a debug route: it needs no sdfa_debug_keep_intermediates, runs the default shared-column path, and works across
 * workspace chunks: each chunk's layer-0 output is copied out of its K4 region before the region is reused. */
typedef struct sdfa_model sdfa_model;
int sdfa_encoder_layer0(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_X1, void *d_ws, int64_t ws_bytes,
                        void *stream);

/* Refused with SDFA_EINVAL before any launch: N < 1 or N > SDFA_LSTMTRAIN_MAX_FRAMES, null pointers (d_dX may be null), a short or
 * misaligned workspace, backward without a forward on the same workspace and N, lr / betas / eps outside their ranges; with
 * SDFA_ESTATE: a handle that is not finalised (finalize names the first missing tensor), set_tensor after finalize. */

#ifdef __cplusplus
}
#endif
#endif
