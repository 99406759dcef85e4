/* C ABI of the training objective in libsdfa_hip.so (sdfa-2019_amd/csrc/objective.hip, api_objective.cpp): what the
 * reference's get_loss (speech_anime/model/model.py:261-330) computes as an objective with PcaInversion
 * (speech_anime/modules/output_module.py:94-116), PLoss and MLoss (speech_anime/model/criterion.py:7-73) for
 * prediction_type "face_data" and pca_trainable = False: the four losses of a collated training batch [a; b] and their
 * gradients with respect to the PCA coefficients, in one pass over the basis and the targets.  The predicted rows and the
 * residual rows never exist in memory.  DESIGN.md section 15.
 *
 * Conventions are those of sdfa_hip.h and sdfa_score.h: every call returns >= 0 on success and a negative SDFA_E* code on
 * failure, sdfa_last_error() describes the failure.  The surface is stateless, stream-ordered, copies nothing and never
 * synchronises; every refusal is decided before any launch.  It is versioned on its own (SDFA_OBJECTIVE_ABI_VERSION); it
 * does not change SDFA_ABI_VERSION.  All buffers are device float32 unless said otherwise.
 *
 * Batch     N = 2 B rows.  Row k < B is window a of sample k, row B + k the next window b, as train_batch collates.
 * Coef      coef [N][Kc], row stride Kc.
 * Layout    DGRAD: Kc = Ks + Kr, scale coefficients first (as sdfa_regress_forward writes d_coef); compT_s [6T][Ks],
 *                  means_s [6T], compT_r [3T][Kr], means_r [3T] -- the reference's .npy layout, the one sdfa_pca_transform
 *                  takes; a row is W = 9 T values, [6 scale | 3 rotat] per triangle.
 *           PLAIN: compT_s [W][K], means_s [W], any W (the offsets head); compT_r, means_r and Kr are ignored.
 * Truth     truth [N][W] (train_batch's face_data), weight [N] (anime_weight).
 * Rows      p = means + coef . compT^T in float32 (fp32 MFMA; the order of the K additions is the kernel's).
 *           e(x) = expf(x) -- the accurate one -- on the rotat columns of DGRAD, the identity elsewhere; e' = e there, 1 elsewhere.
 *           n = T for DGRAD, W for PLAIN (the criterion sums a triangle's 6 or 3 values and averages the triangles).
 *           h_k = fl(weight[k] + weight[B + k]).  Column sets: scale (every column of PLAIN) and rotat.
 * Record    double rec[N][4], unweighted column sums, slots in the order of the losses (ps, ms, pr, mr):
 *               rec[r][0], rec[r][2] = sum over the scale / rotat columns of fl(e(p) - e(t))^2
 *               rec[B + k][1], rec[B + k][3] = the same two column sets of
 *                            fl( fl(e(p_b) - e(p_a)) - fl(e(t_b) - e(t_a)) )^2, a = k, b = B + k;  0 on rows < B
 *           Every difference is one float32 subtraction, never contracted, as the reference forms it; squares and sums are
 *           double.  Slots 2 and 3 are 0 for PLAIN.
 * Losses    float loss[4] = (ps, ms, pr, mr):
 *               L_p = 1 / N sum_r weight[r] / n rec[r][p slot]        L_m = 1 / B sum_k h_k / n rec[B + k][m slot]
 *           summed in double and rounded once by a finishing kernel: nothing is read back.
 * Grads     float grad[2][N][Kc]: d L_p / d coef and d L_m / d coef (scale and rotat together: scale columns only reach
 *           coef[:, :Ks], rotat columns only coef[:, Ks:]), unscaled:
 *               grad[term][r][i] = c_term[r] sum_cols g_term[r][col] compT[col][i]
 *               g_p[r] = fl(e(p) - e(t)) e'(p)          c_p[r] = 2 weight[r] / (N n)
 *               g_m[b] = m e'(p_b), g_m[a] = -m e'(p_a) c_m[a] = c_m[b] = 2 h_k / (B n)          m: the motion difference above
 *           g and the contraction are float32 (fp32 MFMA); the partial sums over column partitions are added in double, in
 *           ascending order, multiplied by c in double and rounded once.  The two terms stay apart because the reference
 *           divides each by its own DynamicLossScaler.scale.
 * Tiling    a workgroup owns SDFA_OBJECTIVE_PAIRS whole pairs (32 rows: a rows, then their b rows) and a contiguous range of
 *           column blocks of SDFA_OBJECTIVE_COLS basis columns of one basis.  The number of column partitions depends on the
 *           shape alone (sdfa_objective_workspace_bytes), never on the device.
 * Sums      no atomics, no workgroup waits on another: partial sums go to the workspace, finishing kernels add them in
 *           ascending order.  The same inputs give the same bits.
 * Absent    ELoss (this model emits no evector).  DynamicLossScaler is host state (sdfa_amd.objective.DynamicLossScaler).
 */
#ifndef SDFA_OBJECTIVE_H
#define SDFA_OBJECTIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_OBJECTIVE_ABI_VERSION 1

#define SDFA_OBJECTIVE_LAYOUT_DGRAD 0  /* W = 9 T: per triangle six scale and three rotat values */
#define SDFA_OBJECTIVE_LAYOUT_PLAIN 1  /* any W: the offsets head */

#define SDFA_OBJECTIVE_MAX_K 192       /* coefficients per basis (the shipped heads: 85 / 180 / 59) */
#define SDFA_OBJECTIVE_COLS  128       /* basis columns per column block */
#define SDFA_OBJECTIVE_PAIRS 16        /* pairs (k, B + k) per row tile */
#define SDFA_OBJECTIVE_KSTEP 8         /* the expansion contracts k in steps of this; in LDS a basis row is K rounded up to 32, zeros past K */

int sdfa_objective_abi_version(void);

/* Device workspace of one sdfa_objective call, a multiple of 256 bytes; SDFA_EINVAL for the shapes sdfa_objective refuses. */
int64_t sdfa_objective_workspace_bytes(int64_t N, int64_t W, int64_t Ks, int64_t Kr, int layout);

/* Losses, records and gradients.  d_ws is 256-byte aligned device memory of at least sdfa_objective_workspace_bytes(...).
 * Stream-ordered: nothing is copied, nothing synchronises.
 * Refused with SDFA_EINVAL before any launch: odd N or N < 2, W < 1, W % 9 != 0 for DGRAD, Ks (and Kr for DGRAD) outside
 * 1 .. SDFA_OBJECTIVE_MAX_K, an unknown layout, null pointers (compT_r and means_r may be null for PLAIN), a short or
 * misaligned workspace. */
int sdfa_objective(const float *d_coef, int64_t N, int64_t W, int64_t Ks, int64_t Kr, int layout, const float *d_compT_s,
                   const float *d_means_s, const float *d_compT_r, const float *d_means_r, const float *d_truth,
                   const float *d_weight, float *d_loss, double *d_rec, float *d_grad, void *d_ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
