// Launchers of score.hip for api_score.cpp.
#pragma once
#include "../../include/sdfa_score.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

struct ScoreArgs {
    const float *pred, *track;
    const int64_t *src;
    const float *w;
    const unsigned char *first;      // [F]: 1 on a clip's first frame
    double *part;                    // [F][nslab][SDFA_SCORE_PARTS][4]
    double *out;                     // [F][4]
    int64_t F, W, n_track, nslab;
};

// A chunk of clip starts, passed to the marking kernel by value: the host's offsets reach the device without a copy.
constexpr int SCORE_MARKS = 448;
struct ScoreMarks {
    int64_t off[SCORE_MARKS];
    int n;
};

hipError_t score_mark(const ScoreMarks &m, unsigned char *first, hipStream_t st);
hipError_t score_launch(const ScoreArgs &a, int layout, hipStream_t st);
