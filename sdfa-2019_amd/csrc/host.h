// Host-side helpers shared by the api_*.cpp files and the host parts of render.hip / jpeg.hip / obj.hip: the error path and round_up.
#pragma once
#include "../../include/sdfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>

// Record the message sdfa_last_error() returns (api_core.cpp) and return `code`.
int sdfa_fail(int code, const char *fmt, ...);
int sdfa_failv(int code, const char *fmt, va_list ap);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) return sdfa_fail(SDFA_EHIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
