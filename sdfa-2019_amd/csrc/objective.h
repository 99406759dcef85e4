// Launcher of objective.hip for api_objective.cpp.
#pragma once
#include "../../include/sdfa_objective.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

// One basis: the scale or the rotat part of a dgrad head, or the whole of a plain head.
struct ObjPart {
    const float *compT, *means;      // [C][K], [C]
    int64_t C;                       // basis columns
    int K, KP, KS;                   // coefficients; LDS row stride (KS + 4); K rounded up to 32
    int koff;                        // first coefficient column of this basis in a coef row
    int G, S, OFF;                   // basis column q is truth column (q / G) * S + OFF + q % G
    int exp;                         // 1: e(x) = expf(x) on these columns
    int ncb, P, px0;                 // column blocks; column partitions; index of the first one among both parts'
    int64_t gpart_off;               // floats: this part's [P][2][rowtiles * 32][KS] partial gradients in gpart
};

struct ObjArgs {
    ObjPart part[2];
    int nparts;
    const float *coef, *truth, *weight;
    int64_t N, B, W;
    int Kc, rowtiles;
    double n;                        // T for dgrad, W for plain
    double *lpart;                   // [PX][N][2]: per row (sum of p squares, sum of m squares)
    float *gpart;
    float *loss;                     // [4]
    double *rec;                     // [N][4]
    float *grad;                     // [2][N][Kc]
};

size_t objective_lds_bytes(int KPmax);
hipError_t objective_launch(const ObjArgs &a, hipStream_t st);
