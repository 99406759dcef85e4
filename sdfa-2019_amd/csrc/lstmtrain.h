// Launchers of lstmtrain.hip for api_lstmtrain.cpp.
#pragma once
#include "../../include/sdfa_lstmtrain.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int LT_T = SDFA_LSTMTRAIN_STEPS, LT_H = SDFA_LSTMTRAIN_HIDDEN, LT_G = SDFA_LSTMTRAIN_GATES, LT_Y = 2 * LT_H;
constexpr int LT_TILE_FRAMES = SDFA_LSTMTRAIN_TILE_FRAMES;          // frames of one workgroup of a recurrence
constexpr int LT_BLOCK_FRAMES = SDFA_LSTMTRAIN_BLOCK_FRAMES;        // frames of one row block of the split dW contractions
constexpr int64_t LT_IMG = 2 * (int64_t)LT_G * LT_H;                // floats of one image of both directions' W_hh

// The flat parameter layout: W_ih [2][1024][I] (forward, reverse), then W_hh [2][1024][256].  The gradient buffer and every row
// block's partial have the same layout.
struct LtImagesArgs {
    const float *Whh;                // [2][1024][256]
    float *img, *imgT;               // [2][64 k-quads][1024 rows] float4;  [2][256 row-quads][256 units] float4
};

struct LtPreArgs {
    const float *X, *Wih;            // [N][64][I], [2][1024][I]
    float *gates;                    // [2][N][64][1024]: pre goes where the recurrence leaves the activated gates
    int64_t N;
    int I;
};

struct LtFwdArgs {
    const float *img;
    float *gates, *c, *Y;            // [2][N][64][1024], [2][N][64][256], [N][64][512]
    int64_t N;
};

struct LtBwdArgs {
    const float *imgT, *c, *dY;
    float *gates;                    // activated gates in, dG out
    int64_t N;
};

struct LtProdArgs {
    const float *X, *Y, *gates, *Wih;
    float *part;                     // [nblk][numel]: added by the reduce launch
    float *dX;                       // [N][64][I] or null
    int64_t N;
    int I, nblk;
};

struct LtReduceArgs {
    const float *part;
    float *grad;
    int64_t numel;
    int nblk;
};

hipError_t lstmtrain_images(const LtImagesArgs &a, hipStream_t st);
hipError_t lstmtrain_pre(const LtPreArgs &a, hipStream_t st);
hipError_t lstmtrain_forward(const LtFwdArgs &a, hipStream_t st);
hipError_t lstmtrain_backward(const LtBwdArgs &a, hipStream_t st);
hipError_t lstmtrain_products(const LtProdArgs &a, hipStream_t st);
hipError_t lstmtrain_reduce(const LtReduceArgs &a, hipStream_t st);
