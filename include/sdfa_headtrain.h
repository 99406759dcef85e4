/* C ABI of the regressor head's training step in libsdfa_hip.so (sdfa-2019_amd/csrc/headtrain.hip, api_headtrain.cpp): the
 * reference's output module (speech_anime/modules/output_module.py with config/model/{dgrad,offsets}.py) as a training
 * forward that keeps what the backward needs, the backward through the fully connected stack and its weight normalisation,
 * the gradient with respect to the encoder output z, and one step of torch.optim.Adam (amsgrad off, weight decay 0) as
 * saber_model.configure_optimizers builds it.  DESIGN.md section 16.
 *
 * Conventions are those of sdfa_hip.h and sdfa_objective.h: every call returns >= 0 on success and a negative SDFA_E* code
 * on failure, sdfa_last_error() describes the failure.  Everything after finalize is stream-ordered; every refusal is decided
 * before any launch.  Versioned on its own (SDFA_HEADTRAIN_ABI_VERSION); SDFA_ABI_VERSION does not change.
 *
 * Head      x0 = [z (512) | onehot(speaker) (8)].
 *           DGRAD:   trunk h0 = lrelu_0.2(W_t x0 + b_t) 520 -> 512, then per branch (scale, rotat) x1 = [h0 | onehot],
 *                    h1 = lrelu_0.2(W_1 x1 + b_1) 520 -> 512, h2 = tanh(W_2 h1 + b_2) 512 -> 256, c = W_3 h2 + b_3 256 -> 85 | 180;
 *                    coef = [c_scale | c_rotat], Kc = 265.  Seven layers.
 *           OFFSETS: 520 -> 512 lrelu (with the one-hot), 512 -> 256 tanh, 256 -> 59 linear; Kc = 59.  Three layers.
 * Tensors   every layer carries torch.nn.utils.weight_norm(dim = 0): W[p, :] = g[p] v[p, :] / ||v[p, :]||.  Its trainable
 *           tensors are weight_g [P][1], weight_v [P][K], bias [P], named as the reference names them with "_model."
 *           stripped: "_output_module._layers.0.weight_g", "_output_module._scale_layers.2.bias", ...
 * State     flat float32 device buffers of parameters, gradients, exp_avg, exp_avg_sq (one layout: per layer g, v, bias) and
 *           the step count on the host.  finalize uploads once; after it the parameters live on the device.
 * Forward   1. fold: ss = sum_k v^2, inv = 1 / sqrt(ss), s = g inv, W = s v, all float32; a wave per row, every layer in one launch.
 *           2. per depth one launch (both dgrad branches in it): pre = sum_k x_k W[p][k] (fp32 MFMA, k ascending), then + b[p],
 *              then + W[p][512 + speaker] where the layer takes the one-hot; lrelu is max(x, 0.2f x), tanh is tanhf.
 *           The one-hot columns are never materialised.  Kept in the workspace: z, the speaker ids, the layer outputs.
 * Backward  per depth one launch; block index tells a layer's dW + db tiles from its dX tiles.
 *               dW[p][k] = sum_n dPre[n][p] x[n][k] (n ascending in one fp32 MFMA chain per row block of 4,096 rows; a batch of
 *               more than 4,096 rows leaves float32 partials, and one more launch adds them in ascending block order);
 *               dW[p][512 + s] = sum over the rows of speaker s of dPre[n][p];  db[p] = sum_n dPre[n][p]
 *               dX[n][k] = sum_p dPre[n][p] W[p][k], k < 512 (the one-hot part is discarded)
 *               dPre of the layer below = dX * (y > 0 ? 1 : 0.2f) for lrelu, dX * fma(-y, y, 1) for tanh, y the kept output;
 *               dh0 = (scale branch's dX) + (rotat branch's dX), two accumulators added in that order.
 *           then one launch through the weight norm, a wave per row:
 *               dg[p] = <dW[p, :], v[p, :]> inv,   dv[p, :] = s (dW[p, :] - (dg inv) v[p, :]).
 *           It OVERWRITES the gradient buffer.  dz = columns 0 .. 511 of the first layer's dX; skipped when d_dz is null.
 * Adam      one launch over the whole flat buffer; t-1 -> t on the host, both bias corrections formed in double there:
 *               m <- m + (g - m)(1 - beta1);  v <- beta2 v + ((1 - beta2) g) g;
 *               p <- p - (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)).
 *           An element whose gradient has been exactly 0 at every step keeps its bits.
 * Sums      no atomics, no workgroup waits on another.  Every sum's order depends on the shape alone: the same inputs give
 *           the same bits, and a row's coef and dz do not depend on the other rows of the batch.
 * Launches  DGRAD: 1 + 4 (forward) + 4 + 1 (backward) + 1 (Adam) = 11;  OFFSETS: 1 + 3 + 3 + 1 + 1 = 9;  one more in the backward of
 *           a batch of more than 4,096 rows (the row blocks' reduce).
 */
#ifndef SDFA_HEADTRAIN_H
#define SDFA_HEADTRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_HEADTRAIN_ABI_VERSION 1

#define SDFA_HEADTRAIN_HEAD_DGRAD   0
#define SDFA_HEADTRAIN_HEAD_OFFSETS 1

/* `what` of get_tensor / set_state */
#define SDFA_HEADTRAIN_PARAM      0
#define SDFA_HEADTRAIN_GRAD       1
#define SDFA_HEADTRAIN_EXP_AVG    2
#define SDFA_HEADTRAIN_EXP_AVG_SQ 3

#define SDFA_HEADTRAIN_Z        512   /* width of the encoder output */
#define SDFA_HEADTRAIN_SPEAKERS 8     /* one-hot columns */
#define SDFA_HEADTRAIN_TILE     64    /* rows and columns of an output tile of every product */
#define SDFA_HEADTRAIN_MAX_ROWS (1 << 21) /* 32,768 row tiles: inside the grid limit */

typedef struct sdfa_headtrain sdfa_headtrain;

int sdfa_headtrain_abi_version(void);

/* An empty handle for one head; NULL (and sdfa_last_error) for an unknown head. */
sdfa_headtrain *sdfa_headtrain_create(int head);
void sdfa_headtrain_destroy(sdfa_headtrain *h);

/* Host float32 data of one tensor, before finalize.  SDFA_EINVAL: unknown name, wrong numel, null; SDFA_ESTATE: finalised. */
int sdfa_headtrain_set_tensor(sdfa_headtrain *h, const char *name, const float *h_src, int64_t numel);
/* Uploads the parameters, zeroes the gradients and both moments, step count 0.  SDFA_ESTATE names the first missing tensor. */
int sdfa_headtrain_finalize(sdfa_headtrain *h, void *stream);

/* Coefficients per row (265 | 59) and the number of trainable elements. */
int sdfa_headtrain_coef_dim(const sdfa_headtrain *h);
int64_t sdfa_headtrain_numel(const sdfa_headtrain *h);

/* Bytes of workspace a batch of up to max_rows rows needs; a multiple of 256. */
int64_t sdfa_headtrain_workspace_bytes(const sdfa_headtrain *h, int64_t max_rows);

/* Training forward: d_z float32 [N][512], d_speaker_id int64 [N] (values outside 0 .. 7 select no column: the caller
 * validates them), d_coef float32 [N][Kc].  d_ws is 256-byte aligned device memory of at least workspace_bytes(h, N). */
int sdfa_headtrain_forward(sdfa_headtrain *h, const float *d_z, const int64_t *d_speaker_id, int64_t N, float *d_coef,
                           void *d_ws, int64_t ws_bytes, void *stream);
/* Backward of the last forward on this workspace and N: d_dcoef float32 [N][Kc]; d_dz float32 [N][512] or null. */
int sdfa_headtrain_backward(sdfa_headtrain *h, const float *d_dcoef, int64_t N, float *d_dz, void *d_ws, int64_t ws_bytes, void *stream);
/* One optimiser step on the gradients the handle holds. */
int sdfa_headtrain_adam(sdfa_headtrain *h, double lr, double beta1, double beta2, double eps, void *stream);
int sdfa_headtrain_zero_grad(sdfa_headtrain *h, void *stream);

/* Access for tests and resume; these synchronise the device.  `name` as in set_tensor. */
int sdfa_headtrain_get_tensor(sdfa_headtrain *h, const char *name, int what, float *h_dst, int64_t numel);
int sdfa_headtrain_set_grad(sdfa_headtrain *h, const char *name, const float *h_src, int64_t numel);
int sdfa_headtrain_set_state(sdfa_headtrain *h, const char *name, int what, const float *h_src, int64_t numel);
int64_t sdfa_headtrain_step_count(const sdfa_headtrain *h);
int sdfa_headtrain_set_step_count(sdfa_headtrain *h, int64_t t);

/* Refused with SDFA_EINVAL before any launch: odd N, N < 2 or N > SDFA_HEADTRAIN_MAX_ROWS, null pointers (d_dz may be null),
 * a short or misaligned workspace, backward without a forward on the same workspace and N, lr / betas / eps outside their
 * ranges; with SDFA_ESTATE: a handle that is not finalised. */

#ifdef __cplusplus
}
#endif
#endif
