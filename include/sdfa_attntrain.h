/* C ABI of the attention layer's training step in libsdfa_hip.so (sdfa-2019_amd/csrc/attntrain.hip, api_attntrain.cpp): the
 * reference's Bahdanau attention (speech_anime/layers/attentions.py, ("attn", "bah", 512, 128, 2) in both model configurations,
 * called as layers/__init__.py calls it: query = H[:, 31:34], key = H, training mode) as a training forward that keeps what the
 * backward needs, the analytic backward down to dH, and one step of torch.optim.Adam (amsgrad off, weight decay 0).  The layer that
 * consumes the dz of sdfa_headtrain.h.  DESIGN.md section 17.
 *
 * Conventions are those of sdfa_hip.h and sdfa_headtrain.h: every call returns >= 0 on success and a negative SDFA_E* code on
 * failure, sdfa_last_error() describes the failure.  Everything after finalize is stream-ordered; every refusal is decided before
 * any launch.  Versioned on its own (SDFA_ATTNTRAIN_ABI_VERSION); SDFA_ABI_VERSION does not change.
 *
 * Input     per frame n, H = H[n] is [64][512]: the 2-layer BiLSTM's output at the time steps t = 0 .. 63 (layer 9 of the
 *           encoder; the layout of debug tap 3).  The recurrent stack below is frozen and runs in its inference form, without
 *           dropout between the BiLSTM layers, as the frozen encoder of sdfa_headtrain.h does.
 * Tensors   plain parameters, no weight norm (create_self_atten swallows the key), named as the reference names them with
 *           "_model." stripped:
 *               Wc = "_audio_encoder._layers.10._conv_query.weight"  [512 o][512 c][3 k]
 *               Wq = "_audio_encoder._layers.10.proj_qry.weight"     [128][512]
 *               Wk = "_audio_encoder._layers.10.proj_key.weight"     [128][512]
 *               v  = "_audio_encoder._layers.10.v.weight"            [1][128]
 *               b  = "_audio_encoder._layers.10.b"                   [1][1][128]
 *           917,760 elements.
 * State     flat float32 device buffers of parameters, gradients, exp_avg, exp_avg_sq (one layout: Wc, Wq, Wk, v, b) and the step
 *           count on the host.  finalize uploads once; after it the parameters live on the device.
 * Forward   training mode (scale_score_at_eval acts in eval mode only, and is 1.0 in both configurations):
 *               qc[o]  = sum_{c,k} Wc[o][c][k] H[31 + k][c]        (Conv1d, stride 3, no bias, over the window H[31 .. 33])
 *               qp     = Wq qc                                     [128]
 *               u_t    = tanhf((Wk H[t] + qp) + b)                 [128], t = 0 .. 63
 *               s_t    = v . u_t ;  a = softmax_t(s) ;  z = sum_t a_t H[t]          outputs: z [512], align a [64]
 *           The products are fp32 MFMA chains with the contraction index ascending (qc contracts in the order k, then c); s and z
 *           are fma chains, m and t ascending; the softmax is the plain two-pass one (max, expf, sum, divide).
 *           Kept in the workspace: qc, qp, u (32 KiB per frame: storing it costs 64 KiB of traffic per frame, recomputing it
 *           8.4 MFLOP and a second pass over H) and align.
 * Backward  given dz [512] per frame:
 *               da_t   = dz . H[t] ;   ds_t = a_t (da_t - sum_j a_j da_j)
 *               dv    += sum_t ds_t u_t ;   dpre_t = (ds_t v) * fma(-u_t, u_t, 1) ;   db += sum_t dpre_t ;   dqp = sum_t dpre_t
 *               dWk   += sum_t dpre_t H[t]^T ;   dWq += dqp qc^T ;   dqc = Wq^T dqp ;   dWc[o][c][k] += dqc[o] H[31 + k][c]
 *               dH[t]  = fma(a_t, dz, Wk^T dpre_t)  (+ sum_o Wc[o][:][t - 31] dqc[o]  for t = 31, 32, 33, added last)
 *           The parameter gradients are summed over the N frames; the call OVERWRITES the gradient buffer.  A null d_dH skips
 *           the dH tiles and changes no other output.
 * Sums      no atomics, no workgroup waits on another.  dWk, dv and db contract over all 64 N rows: they are formed per row block
 *           of SDFA_ATTNTRAIN_BLOCK_FRAMES frames (a constant of the shape, not of the device) as float32 partials and added in
 *           ascending block order by a second launch.  dWc and dWq are one chain over n per output tile.  Every sum's order
 *           depends on N alone: the same inputs give the same bits, and a frame's z, align and dH do not depend on the other
 *           frames of the batch.
 * Adam      the kernel and the host arithmetic of sdfa_headtrain.h, through one shared launcher.
 * Launches  3 (forward: qc, qp, frames) + 5 (backward: frames, dqc, dHq, products, reduce) + 1 (Adam) = 9.
 */
#ifndef SDFA_ATTNTRAIN_H
#define SDFA_ATTNTRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_ATTNTRAIN_ABI_VERSION 1

/* `what` of get_tensor / set_state */
#define SDFA_ATTNTRAIN_PARAM      0
#define SDFA_ATTNTRAIN_GRAD       1
#define SDFA_ATTNTRAIN_EXP_AVG    2
#define SDFA_ATTNTRAIN_EXP_AVG_SQ 3

#define SDFA_ATTNTRAIN_STEPS 64             /* time steps of a frame */
#define SDFA_ATTNTRAIN_DIM   512            /* width of H and z */
#define SDFA_ATTNTRAIN_ATT   128            /* width of the score space */
#ifndef SDFA_ATTNTRAIN_BLOCK_FRAMES         /* (tools/attntrain_bench.py measures against a build with one block: the unsplit chain) */
#define SDFA_ATTNTRAIN_BLOCK_FRAMES 16      /* frames (1,024 rows) of one partial of dWk, dv, db */
#endif
#define SDFA_ATTNTRAIN_MAX_FRAMES 32768     /* 2^21 key rows */

typedef struct sdfa_attntrain sdfa_attntrain;

int sdfa_attntrain_abi_version(void);

sdfa_attntrain *sdfa_attntrain_create(void);
void sdfa_attntrain_destroy(sdfa_attntrain *h);

/* Host float32 data of one tensor, before finalize.  SDFA_EINVAL: unknown name, wrong numel, null; SDFA_ESTATE: finalised. */
int sdfa_attntrain_set_tensor(sdfa_attntrain *h, const char *name, const float *h_src, int64_t numel);
/* Uploads the parameters, zeroes the gradients and both moments, step count 0.  SDFA_ESTATE names the first missing tensor. */
int sdfa_attntrain_finalize(sdfa_attntrain *h, void *stream);

int64_t sdfa_attntrain_numel(const sdfa_attntrain *h);
/* Bytes of workspace a batch of up to max_frames frames needs; a multiple of 256. */
int64_t sdfa_attntrain_workspace_bytes(const sdfa_attntrain *h, int64_t max_frames);

/* Training forward: d_H float32 [N][64][512] row-major, d_z float32 [N][512], d_align float32 [N][64].  d_ws is 256-byte aligned
 * device memory of at least workspace_bytes(h, N). */
int sdfa_attntrain_forward(sdfa_attntrain *h, const float *d_H, int64_t N, float *d_z, float *d_align, void *d_ws, int64_t ws_bytes,
                           void *stream);
/* Backward of the last forward on this workspace and N, with the same d_H: d_dz float32 [N][512]; d_dH float32 [N][64][512] or null. */
int sdfa_attntrain_backward(sdfa_attntrain *h, const float *d_H, const float *d_dz, int64_t N, float *d_dH, void *d_ws,
                            int64_t ws_bytes, void *stream);
/* One optimiser step on the gradients the handle holds. */
int sdfa_attntrain_adam(sdfa_attntrain *h, double lr, double beta1, double beta2, double eps, void *stream);
int sdfa_attntrain_zero_grad(sdfa_attntrain *h, void *stream);

/* Access for tests and resume; these synchronise the device.  `name` as in set_tensor. */
int sdfa_attntrain_get_tensor(sdfa_attntrain *h, const char *name, int what, float *h_dst, int64_t numel);
int sdfa_attntrain_set_grad(sdfa_attntrain *h, const char *name, const float *h_src, int64_t numel);
int sdfa_attntrain_set_state(sdfa_attntrain *h, const char *name, int what, const float *h_src, int64_t numel);
int64_t sdfa_attntrain_step_count(const sdfa_attntrain *h);
int sdfa_attntrain_set_step_count(sdfa_attntrain *h, int64_t t);

/* The frozen encoder's forward (sdfa_encoder_forward of sdfa_hip.h, same arguments and refusals) that also writes the attention
 * layer's memory: d_H float32 [n_frames][64][512] row-major, the layout of debug tap 3, for every frame.  Not a debug route: it
 * needs no sdfa_debug_keep_intermediates.  It works across workspace chunks: each chunk's H is copied out of the K4 region
 * before the region is reused.  d_z and d_align may be null; where given they are bitwise those of sdfa_encoder_forward. */
typedef struct sdfa_model sdfa_model;
int sdfa_encoder_memory(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_H, float *d_z, float *d_align,
                        void *d_ws, int64_t ws_bytes, void *stream);

/* Refused with SDFA_EINVAL before any launch: N < 1 or N > SDFA_ATTNTRAIN_MAX_FRAMES, null pointers (d_dH may be null), a short or
 * misaligned workspace, backward without a forward on the same workspace and N, lr / betas / eps outside their ranges; with
 * SDFA_ESTATE: a handle that is not finalised (finalize names the first missing tensor), set_tensor after finalize. */

#ifdef __cplusplus
}
#endif
#endif
