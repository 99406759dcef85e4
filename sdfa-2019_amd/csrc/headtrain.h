// Launchers of headtrain.hip for api_headtrain.cpp.
#pragma once
#include "../../include/sdfa_headtrain.h"
#include "trainstate.h"      // HtAdamArgs, headtrain_adam, headtrain_adam_step: the three trainers share the Adam kernel

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

constexpr int HT_MAX_LAYERS = 7;
constexpr int HT_BLOCK_ROWS = 4096;  // rows of one row block of the dW | db contraction: 64 row tiles
enum { HT_ACT_LINEAR = 0, HT_ACT_LRELU = 1, HT_ACT_TANH = 2 };

// One fully connected layer inside the flat buffers.  Parameters, gradients and both moments share one layout (per layer
// g [P], v [P][K], bias [P]); the effective weights W and their gradients dW share another ([P][K] per layer); inv and s are
// per row of all layers.
struct HtLayer {
    int P, K, Kin;                   // outputs; inputs with the one-hot columns; inputs without them
    int cond, act;                   // 1: the layer takes the one-hot; HT_ACT_*
    int row0;                        // first row among all layers' rows
    int64_t og, ov, ob;              // offsets (floats) of g, v, bias in a parameter-shaped buffer
    int64_t ow;                      // offset (floats) of W / dW
};

struct HtTable {
    HtLayer l[HT_MAX_LAYERS];
    int nl, rows;
};

// A forward layer of one branch: Y = act(X W[:, :Kin]^T + b + W[:, Kin + speaker])
struct HtFwdJob {
    const float *X, *W, *bias;
    float *Y;
    int ldx, ldw, ldy, P, Kin, cond, act;
};

struct HtFwdArgs {
    HtFwdJob b[2];
    int nb;
    int64_t N;
    const int64_t *sid;
    float *zcopy;                    // first layer only: z [N][512] and the ids are kept for the backward
    int *sidcopy;
};

// The backward of one layer of one branch: dW | db from D and the layer's input X, and the branch's share of dX.
struct HtBwdJob {
    const float *D;                  // dPre [N][P], row stride ldd
    const float *X;                  // the layer's input [N][Kin], row stride ldx
    const float *W;                  // [P][K]
    float *dW, *db;                  // [P][K], [P]
    float *pW, *pb;                  // the row blocks' partials of dW and db, block strides psw and psb (more than one row block only)
    const float *Yprev;              // output of the layer below (what X is), for its activation's derivative
    float *Dprev;                    // dPre of the layer below [N][Kin], or dz
    int ldd, ldx, ldp, P, K, Kin, cond;
    int tp, tk, ndw;                 // dW tiles along p and along k (K + 1 columns: the last one is db); tp * tk
};

enum { HT_DX_NONE = 0, HT_DX_BRANCH = 1, HT_DX_MERGE = 2, HT_DX_PLAIN = 3 };

struct HtBwdArgs {
    HtBwdJob b[2];
    int nb;
    int64_t N;
    const int *sid;
    int dx_mode;                     // NONE: no dX tiles; BRANCH: each branch's own, times act'; MERGE: both branches into one, times act'; PLAIN: dz
    int act_prev;
    int rowtiles, tkx;               // dX tiles along n and along k (Kin / 64)
    int nblk;                        // row blocks of HT_BLOCK_ROWS rows; 1: the dW tiles write dW and db themselves
    int64_t psw, psb;                // floats between two row blocks' partials of dW (all layers' W) and of db (all layers' rows)
};

struct HtReduceArgs {
    HtTable t;
    const float *pW, *pb;            // [nblk][wnumel], [nblk][rows]
    float *dW, *grads;               // dW [wnumel]; db goes to its place in the gradient buffer
    int64_t wnumel;
    int nblk;
};

hipError_t headtrain_fold(const HtTable &t, const float *params, float *W, float *inv, float *sc, hipStream_t st);
hipError_t headtrain_forward_layer(const HtFwdArgs &a, hipStream_t st);
hipError_t headtrain_backward_layer(const HtBwdArgs &a, hipStream_t st);
hipError_t headtrain_reduce(const HtReduceArgs &a, hipStream_t st);
hipError_t headtrain_wnorm_backward(const HtTable &t, const float *params, const float *dW, const float *inv, const float *sc, float *grads, hipStream_t st);
