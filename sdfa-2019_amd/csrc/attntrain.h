// Launchers of attntrain.hip for api_attntrain.cpp.
#pragma once
#include "../../include/sdfa_attntrain.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int AT_T = SDFA_ATTNTRAIN_STEPS, AT_D = SDFA_ATTNTRAIN_DIM, AT_A = SDFA_ATTNTRAIN_ATT, AT_W0 = 31, AT_KW = 3;
constexpr int AT_BLOCK_FRAMES = SDFA_ATTNTRAIN_BLOCK_FRAMES;        // frames of one row block of the split dWk contraction

// An operand of a product: element (i, c) -- i the tile's row or column index, c the contraction index -- lies at
// p + f(i) si + g(c) sc, i < ni, c < nc; f and g are the identity or one of the two index maps of attntrain.hip.
struct AtOp {
    const float *p;
    int64_t si, sc, ni;
    int nc;
};

enum { AT_PROD_QC = 0, AT_PROD_QP = 1, AT_PROD_DQC = 2, AT_PROD_DHQ = 3 };

// out[i][j] = sum_c A(i, c) B(j, c), i < A.ni, j < B.ni
struct AtProdArgs {
    AtOp A, B;
    float *out;
    int64_t ldo;
};

struct AtFwdArgs {
    const float *H, *Wk, *v, *b, *qp;
    float *u, *al, *z, *align;       // kept: u [N][64][128], al [N][64]; outputs z [N][512], align [N][64]
    int64_t N;
};

struct AtFrameBwdArgs {
    const float *H, *dz, *al, *u, *v;
    float *dpre, *dvp, *dqp;         // [N][64][128], [N][128], [N][128]
    int64_t N;
};

struct AtBwdArgs {
    const float *H, *dz, *al, *dpre, *dvp, *dqp, *dqc, *qc, *dHq, *Wk;
    float *gWc, *gWq;                // gradient buffer: written here
    float *part, *partv;             // [nblk][128][512], [nblk][dv 128 | db 128]: added by the reduce launch
    float *dH;                       // [N][64][512] or null
    int64_t N;
    int nblk;
};

struct AtReduceArgs {
    const float *part, *partv;
    float *gWk, *gv, *gb;
    int nblk;
};

hipError_t attntrain_product(int which, const AtProdArgs &a, hipStream_t st);
hipError_t attntrain_frame_forward(const AtFwdArgs &a, hipStream_t st);
hipError_t attntrain_frame_backward(const AtFrameBwdArgs &a, hipStream_t st);
hipError_t attntrain_backward(const AtBwdArgs &a, hipStream_t st);
hipError_t attntrain_reduce(const AtReduceArgs &a, hipStream_t st);
