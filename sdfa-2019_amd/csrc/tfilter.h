// Launcher of tfilter.hip for api_tfilter.cpp.
#pragma once
#include "../../include/sdfa_tfilter.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int TFILTER_FIR = 0, TFILTER_BILATERAL = 1;

// One launch: frames fa .. fb - 1 of the batch, which are whole clips.  The clip table and the weights travel by value.
struct TFilterArgs {
    const float *x;
    float *out;
    int64_t W;
    int fa, fb;                                       // the launch's frames; runs tile fa .. fb
    int n_clips;                                      // clips of this launch
    int radius;
    int off[SDFA_TFILTER_CLIPS + 1];                  // their frame offsets in the batch: off[0] = fa, off[n_clips] = fb
    double w[2 * SDFA_TFILTER_MAX_RADIUS + 1];        // FIR: the taps; bilateral: the distance weights
    double factor, range_sigma;                       // bilateral
};

hipError_t tfilter_launch(const TFilterArgs &a, int kind, bool generic, hipStream_t st);
