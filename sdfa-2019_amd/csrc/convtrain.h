// Launchers of convtrain.hip for api_convtrain.cpp.
#pragma once
#include "../../include/sdfa_convtrain.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int CT_COLS = SDFA_CONVTRAIN_COLUMNS, CT_BLOCK_FRAMES = SDFA_CONVTRAIN_BLOCK_FRAMES;
constexpr int CT_F1 = SDFA_CONVTRAIN_BINS, CT_F3 = CT_F1 / 2, CT_F5 = SDFA_CONVTRAIN_OUT_BINS;     // frequency rows of a layer's a
constexpr int CT_C0 = SDFA_CONVTRAIN_IN, CT_C1 = 32, CT_C3 = 64, CT_C5 = SDFA_CONVTRAIN_OUT;        // channels: input, layers 1, 3, 5
constexpr int CT_KF1 = 3, CT_KF3 = 3, CT_KF5 = 1;
constexpr int CT_K1 = CT_C0 * CT_KF1, CT_K3 = CT_C1 * CT_KF3, CT_K5 = CT_C3 * CT_KF5;               // a weight row: [ci][kf]
constexpr int CT_ROWS = CT_C1 + CT_C3 + CT_C5;                                                      // output channels of the stack
static_assert(CT_F5 == CT_F3 / 2, "two pools");

// The flat parameter layout, which the gradient buffer, the folded weights, dW and every row block's partial share; per layer
//   g [co] | v [co][ci][kf] | bias [co] | gamma [co] | beta [co]
constexpr int64_t ct_layer_numel(int co, int k) { return (int64_t)co * (k + 4); }
constexpr int64_t CT_OFF1 = 0, CT_OFF3 = CT_OFF1 + ct_layer_numel(CT_C1, CT_K1), CT_OFF5 = CT_OFF3 + ct_layer_numel(CT_C3, CT_K3);
constexpr int64_t CT_NUMEL = CT_OFF5 + ct_layer_numel(CT_C5, CT_K5);
static_assert(CT_NUMEL == SDFA_CONVTRAIN_NUMEL, "the reference's conv stack holds 11,168 trainable parameters");
// the constants: per layer mean [co] | var [co]
constexpr int CT_CONST1 = 0, CT_CONST3 = 2 * CT_C1, CT_CONST5 = CT_CONST3 + 2 * CT_C3, CT_CONSTS = CT_CONST5 + 2 * CT_C5;

// R = 64 N columns; a pair (column, bin) is row g = F column + f of a [.][F][channels] buffer
struct CtArgs {
    const float *feat;               // [R][128][3]
    const float *P, *K, *W;          // the parameters, the constants, the folded weights (parameter layout, at v's place)
    float *a1, *a3, *a5;             // [R][128][32], [R][64][64], [R][32][64]: a, then da
    float *p1, *p3;                  // [R][64][32], [R][32][64]: the pooled outputs
    float *dp1, *dp3;                // their gradients
    float *q1, *q3, *q5;             // dz (y - mean) rstd at the pooled positions (layer 5: every position)
    float *C;                        // [R][32][64] out (forward)
    const float *dC;                 // (backward)
    float *part;                     // [nblk][CT_NUMEL]
    float *dW, *grad;                // reduce: v's slots go to dW (parameter layout), the 1-D ones to the gradient buffer
    int64_t N;
    int nblk;
};

hipError_t convtrain_forward(const CtArgs &a, hipStream_t st);         // three launches
hipError_t convtrain_backward(const CtArgs &a, hipStream_t st);        // three launches: down to da1
hipError_t convtrain_products(const CtArgs &a, hipStream_t st);
hipError_t convtrain_reduce(const CtArgs &a, hipStream_t st);
