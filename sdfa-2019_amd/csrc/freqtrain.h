// Launchers of freqtrain.hip for api_freqtrain.cpp.
#pragma once
#include "../../include/sdfa_freqtrain.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int FT_COLS = SDFA_FREQTRAIN_COLUMNS, FT_S = SDFA_FREQTRAIN_STEPS, FT_I = SDFA_FREQTRAIN_IN, FT_H = SDFA_FREQTRAIN_HIDDEN;
constexpr int FT_G = SDFA_FREQTRAIN_GATES, FT_O = SDFA_FREQTRAIN_OUT, FT_Y = 2 * FT_H, FT_K = FT_S * FT_Y;   // FT_K: features of HF, 8,192
constexpr int FT_TILE_COLS = SDFA_FREQTRAIN_TILE_COLUMNS;           // columns of one workgroup of a recurrence
constexpr int FT_BLOCK_FRAMES = SDFA_FREQTRAIN_BLOCK_FRAMES;        // frames of one row block of the summed gradients
constexpr int64_t FT_IMG = 2 * (int64_t)FT_G * FT_H;                // floats of one image of both directions' W_hh

// The flat parameter layout, which the gradient buffer and every row block's partial share:
//   W_ih [2][512][64] | W_hh [2][512][128] | b_ih [2][512] | b_hh [2][512] | Wp [256][8192] | bp [256]        (forward, reverse)
constexpr int64_t FT_OFF_WIH = 0, FT_OFF_WHH = FT_OFF_WIH + 2 * (int64_t)FT_G * FT_I, FT_OFF_BIH = FT_OFF_WHH + 2 * (int64_t)FT_G * FT_H;
constexpr int64_t FT_OFF_BHH = FT_OFF_BIH + 2 * FT_G, FT_OFF_WP = FT_OFF_BHH + 2 * FT_G, FT_OFF_BP = FT_OFF_WP + (int64_t)FT_O * FT_K;
constexpr int64_t FT_NUMEL = FT_OFF_BP + FT_O;
static_assert(FT_NUMEL == 2296064 && FT_NUMEL % 256 == 0, "the reference's FreqLstm holds 2,296,064 parameters");

// R = 64 N columns; a pair (column, step) is row g = 32 column + f of every [.][32][.] buffer
struct FtImagesArgs {
    const float *Whh;                // [2][512][128]
    float *img, *imgT;               // [2][32 k-quads][512 rows] float4;  [2][128 row-quads][128 units] float4
};

struct FtPreArgs {
    const float *C, *P;              // [R][32][64]; the parameters
    float *gates;                    // [2][R][32][512]: pre goes where the recurrence leaves the activated gates
    int64_t N;
};

struct FtFwdArgs {
    const float *img;
    float *gates, *c, *HF;           // [2][R][32][512], [2][R][32][128], [R][8192]
    int64_t N;
};

struct FtProjArgs {
    const float *HF, *P;
    float *X0;                       // [R][256]
    int64_t N;
};

struct FtDhfArgs {
    const float *dX0, *P;
    float *dHF;                      // [R][8192]
    int64_t N;
};

struct FtBwdArgs {
    const float *imgT, *c, *dHF;
    float *gates;                    // activated gates in, dG out
    int64_t N;
};

struct FtProdArgs {
    const float *C, *HF, *dX0, *gates, *P;
    float *part;                     // [nblk][FT_NUMEL]: added by the reduce launch
    float *dC;                       // [R][32][64] or null
    int64_t N;
    int nblk;
};

struct FtReduceArgs {
    const float *part;
    float *grad;
    int nblk;
};

hipError_t freqtrain_images(const FtImagesArgs &a, hipStream_t st);
hipError_t freqtrain_pre(const FtPreArgs &a, hipStream_t st);
hipError_t freqtrain_forward(const FtFwdArgs &a, hipStream_t st);
hipError_t freqtrain_proj(const FtProjArgs &a, hipStream_t st);
hipError_t freqtrain_dhf(const FtDhfArgs &a, hipStream_t st);
hipError_t freqtrain_backward(const FtBwdArgs &a, hipStream_t st);
hipError_t freqtrain_products(const FtProdArgs &a, hipStream_t st);
hipError_t freqtrain_reduce(const FtReduceArgs &a, hipStream_t st);
