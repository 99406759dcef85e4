/* C ABI of the frequency LSTM's training step in libsdfa_hip.so (sdfa-2019_amd/csrc/freqtrain.hip, api_freqtrain.cpp): the
 * reference's FreqLstm (speech_anime/layers/freq_lstm.py, layer 6 of the audio encoder) -- a bidirectional
 * torch.nn.LSTM(64, 128, bias=True) that runs along the 32 frequency bins of every column, and _proj, a Linear(8192, 256) with bias --
 * as a training forward that keeps what the backward needs, back-propagation through the 32 steps down to dC, and one step of
 * torch.optim.Adam (amsgrad off, weight decay 0).  The stage that consumes the dX of an sdfa_lstmtrain handle of width 256; its dC
 * is what an sdfa_convtrain handle (sdfa_convtrain.h) reads.
 * DESIGN.md section 21.
 *
 * Conventions are those of sdfa_hip.h and sdfa_lstmtrain.h: every call returns >= 0 on success and a negative SDFA_E* code on
 * failure, sdfa_last_error() describes the failure.  Everything after finalize is stream-ordered; every refusal is decided before
 * any launch.  Versioned on its own (SDFA_FREQTRAIN_ABI_VERSION); SDFA_ABI_VERSION does not change.
 *
 * Shape     a frame has 64 columns (n, t); a column is one sequence of F = 32 steps (frequency bins) of 64 channels; 128 hidden
 *           units per direction; R = 64 N sequences in a batch of N frames.  Gate order i, f, g, o, h_{-1} = c_{-1} = 0.
 * Tensors   named as the reference names them with "_model." stripped:
 *               "_audio_encoder._layers.6._lstm.weight_ih_l0", "..._reverse"   [512][64]
 *               "_audio_encoder._layers.6._lstm.weight_hh_l0", "..._reverse"   [512][128]
 *               "_audio_encoder._layers.6._lstm.bias_ih_l0",   "..._reverse"   [512]
 *               "_audio_encoder._layers.6._lstm.bias_hh_l0",   "..._reverse"   [512]
 *               "_audio_encoder._layers.6._proj.weight"                        [256][8192]
 *               "_audio_encoder._layers.6._proj.bias"                          [256]
 *           2,296,064 elements.  bias_ih and bias_hh are two parameters, as in the reference's state dict: they receive the same
 *           gradient and each has its own Adam moments.
 * State     flat float32 device buffers of parameters, gradients, exp_avg, exp_avg_sq (one layout: the tensors in the order
 *           above) and the step count on the host.  finalize uploads once; after it the parameters live on the device.
 * Forward   d_C [N][64][32][64] row-major in: row (n, t) is a column, [f][channel] its 32 steps -- what FreqLstm.forward makes with
 *           permute(0, 3, 2, 1).view(B T, F, C).  d_X0 [N][64][256] out, the layout sdfa_encoder_x0 writes.
 *               pre[d]  = C W_ih[d]^T + (b_ih[d] + b_hh[d])        (the contraction, then one addition of the float32 sum of the biases)
 *               per direction, over its own step order (forward: f = 0 .. 31, reverse: f = 31 .. 0):
 *                   pre_f += W_hh[d] h_prev ;  i, f, o = sigmoid, g = tanh (sigmoidf_acc / tanhf_acc of csrc/common.h)
 *                   c_f = fma(f, c_prev, i g) ;  h_f = o tanh(c_f)
 *               HF[(n, t)][f 256 + d 128 + u] = h        (nn.LSTM's batch-first output viewed as (B T, 8192))
 *               X0 = HF Wp^T + bp
 *           Kept in the workspace, per frame: the activated gates [2][64][32][512] (8 MiB), c [2][64][32][128] (2 MiB),
 *           HF [64][8192] (2 MiB); the backward adds dHF [64][8192] (2 MiB): 14 MiB per frame, 28 GiB at SDFA_FREQTRAIN_MAX_FRAMES.
 *           Offsets pass 2^31 floats from 1,024 frames on: every index is formed in 64 bits.  Every contraction is an fp32 MFMA
 *           chain with its index ascending; a step's chain starts from pre_f.
 * Backward  given d_dX0 [N][64][256]:
 *               dbp = sum_rows dX0 ;  dWp = dX0^T HF ;  dHF = dX0 Wp
 *               per direction against its step order, dh_f = dHF_f + dh_rec and a carried dc:
 *                   do = dh tanh(c_f) o(1 - o) ;  dc += dh o fma(-tanh(c_f), tanh(c_f), 1)
 *                   di = dc g i(1 - i) ;  df = dc c_{f-1} f(1 - f) ;  dg = dc i fma(-g, g, 1)
 *                   dh_rec = W_hh^T [di|df|dg|do] ;  dc <- dc f
 *               c_{f-1} is 0 at a direction's first step.  The pre-activation gradients dG overwrite the kept gates.  Then
 *               dW_ih[d] = sum dG_f C_f^T ;  dW_hh[d] = sum dG_f h_{prev(f)}^T ;  db_ih[d] = db_hh[d] = sum dG_f
 *               dC = sum_d dG[d] W_ih[d]        (one chain over both directions' 1,024 gate rows, forward direction first)
 *           h_{prev(f)} is read from HF one step back in the direction's order and is zero at its first step.  The call OVERWRITES
 *           the gradient buffer.  A null d_dC skips the dC tiles and changes no other output.  The backward consumes the kept
 *           gates: a second backward needs a new forward.
 * Sums      no atomics, no workgroup waits on another: one workgroup per (direction, tile of SDFA_FREQTRAIN_TILE_COLUMNS columns)
 *           in both recurrences.  dWp, dbp, dW_ih, dW_hh and db contract over all 64 N columns: they are formed per row block of
 *           SDFA_FREQTRAIN_BLOCK_FRAMES frames (a constant of the shape, not of the device) as float32 partials and added in
 *           ascending block order by a second launch.  Every sum's order depends on N alone: the same inputs give the same bits,
 *           and a column's X0 and dC do not depend on the other columns of the batch.
 * Adam      the kernel and the host arithmetic of sdfa_headtrain.h, through one shared launcher.
 * Launches  4 (forward: weight images, pre, recurrence, projection) + 4 (backward: dHF, recurrence, products, reduce) + 1 (Adam).
 */
#ifndef SDFA_FREQTRAIN_H
#define SDFA_FREQTRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_FREQTRAIN_ABI_VERSION 1

/* `what` of get_tensor / set_state */
#define SDFA_FREQTRAIN_PARAM      0
#define SDFA_FREQTRAIN_GRAD       1
#define SDFA_FREQTRAIN_EXP_AVG    2
#define SDFA_FREQTRAIN_EXP_AVG_SQ 3

#define SDFA_FREQTRAIN_COLUMNS 64            /* columns (n, t) of a frame: sequences */
#define SDFA_FREQTRAIN_STEPS   32            /* frequency bins: steps of a sequence */
#define SDFA_FREQTRAIN_IN      64            /* channels of a step */
#define SDFA_FREQTRAIN_HIDDEN  128           /* hidden units of a direction */
#define SDFA_FREQTRAIN_GATES   512           /* gate rows of a direction: i, f, g, o */
#define SDFA_FREQTRAIN_OUT     256           /* features of X0 */
#define SDFA_FREQTRAIN_TILE_COLUMNS 32       /* columns of one workgroup of a recurrence: a frame is two tiles per direction */
#define SDFA_FREQTRAIN_BLOCK_FRAMES 8        /* frames (512 columns) of one partial of the summed gradients: a partial is 9.2 MB */
#define SDFA_FREQTRAIN_MAX_FRAMES 2048       /* 14 MiB kept per frame: 28 GiB */

typedef struct sdfa_freqtrain sdfa_freqtrain;

int sdfa_freqtrain_abi_version(void);

sdfa_freqtrain *sdfa_freqtrain_create(void);
void sdfa_freqtrain_destroy(sdfa_freqtrain *h);

/* Host float32 data of one tensor, before finalize.  SDFA_EINVAL: unknown name, wrong numel, null; SDFA_ESTATE: finalised. */
int sdfa_freqtrain_set_tensor(sdfa_freqtrain *h, const char *name, const float *h_src, int64_t numel);
/* Uploads the parameters, zeroes the gradients and both moments, step count 0.  SDFA_ESTATE names the first missing tensor. */
int sdfa_freqtrain_finalize(sdfa_freqtrain *h, void *stream);

int64_t sdfa_freqtrain_numel(const sdfa_freqtrain *h);
/* Bytes of workspace a batch of up to max_frames frames needs; a multiple of 256. */
int64_t sdfa_freqtrain_workspace_bytes(const sdfa_freqtrain *h, int64_t max_frames);

/* Training forward: d_C float32 [N][64][32][64] row-major, d_X0 float32 [N][64][256].  d_ws is 256-byte aligned device memory of at
 * least workspace_bytes(h, N). */
int sdfa_freqtrain_forward(sdfa_freqtrain *h, const float *d_C, int64_t N, float *d_X0, void *d_ws, int64_t ws_bytes, void *stream);
/* Backward of the last forward on this workspace and N, with the same d_C: d_dX0 float32 [N][64][256]; d_dC float32
 * [N][64][32][64] or null. */
int sdfa_freqtrain_backward(sdfa_freqtrain *h, const float *d_C, const float *d_dX0, int64_t N, float *d_dC, void *d_ws,
                            int64_t ws_bytes, void *stream);
/* One optimiser step on the gradients the handle holds. */
int sdfa_freqtrain_adam(sdfa_freqtrain *h, double lr, double beta1, double beta2, double eps, void *stream);
int sdfa_freqtrain_zero_grad(sdfa_freqtrain *h, void *stream);

/* Access for tests and resume; these synchronise the device.  `name` as in set_tensor. */
int sdfa_freqtrain_get_tensor(sdfa_freqtrain *h, const char *name, int what, float *h_dst, int64_t numel);
int sdfa_freqtrain_set_grad(sdfa_freqtrain *h, const char *name, const float *h_src, int64_t numel);
int sdfa_freqtrain_set_state(sdfa_freqtrain *h, const char *name, int what, const float *h_src, int64_t numel);
int64_t sdfa_freqtrain_step_count(const sdfa_freqtrain *h);
int sdfa_freqtrain_set_step_count(sdfa_freqtrain *h, int64_t t);

/* The frozen encoder's forward (sdfa_encoder_x0 of sdfa_bilstm.h: the same arguments, the same workspace and the same refusals; a
 * null d_C is SDFA_EINVAL, decided first) up to and including the conv stack: d_C float32 [n_frames][64][32][64] row-major, what
 * sdfa_freqtrain_forward reads, for every column of every frame.  No frequency LSTM and nothing after it is launched.  Not a
 * debug route: it runs the default shared-column path, on which the conv stack evaluates a chunk's distinct columns only and the
 * copy goes through the chunk's share map, and works across workspace chunks. */
typedef struct sdfa_model sdfa_model;
int sdfa_encoder_conv(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_C, void *d_ws, int64_t ws_bytes,
                      void *stream);

/* Refused with SDFA_EINVAL before any launch: N < 1 or N > SDFA_FREQTRAIN_MAX_FRAMES, null pointers (d_dC may be null), a short or
 * misaligned workspace, backward without a forward on the same workspace and N, lr / betas / eps outside their ranges; with
 * SDFA_ESTATE: a handle that is not finalised (finalize names the first missing tensor), set_tensor after finalize. */

#ifdef __cplusplus
}
#endif
#endif
