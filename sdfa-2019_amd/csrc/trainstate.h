// The flat training state under the three GPU trainers (api_headtrain.cpp, api_attntrain.cpp, api_lstmtrain.cpp; DESIGN.md
// section 20): parameters, gradients and both Adam moments as four device buffers of one layout, the step count and what is known
// of the kept forward.  A module embeds one TrainState as `ts`, locates a tensor by name itself and leaves the rest to the functions
// below; `mod` is the module's word in its messages ("headtrain"), `fn` the entry point's ("forward").
#pragma once
#include "host.h"

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

struct HtAdamArgs {
    float *p, *m, *v;
    const float *g;
    int64_t n;
    float omb1, beta2, omb2, eps, step, bc2s;
};

hipError_t headtrain_adam(const HtAdamArgs &a, hipStream_t st);    // headtrain.hip

// Step t of torch.optim.Adam (amsgrad off, weight decay 0) over one flat buffer: the constants as the host forms them, both bias
// corrections in double.
inline hipError_t headtrain_adam_step(float *p, const float *g, float *m, float *v, int64_t n, int64_t t, double lr, double beta1,
                                      double beta2, double eps, hipStream_t st) {
    HtAdamArgs a;
    a.p = p;
    a.g = g;
    a.m = m;
    a.v = v;
    a.n = n;
    a.omb1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.step = (float)(lr / (1.0 - pow(beta1, (double)t)));
    a.bc2s = (float)sqrt(1.0 - pow(beta2, (double)t));
    return headtrain_adam(a, st);
}

// `what` of get_tensor / set_state: SDFA_{HEAD,ATTN,LSTM}TRAIN_PARAM .. _EXP_AVG_SQ are these numbers (each module asserts it)
enum { TS_PARAM = 0, TS_GRAD = 1, TS_EXP_AVG = 2, TS_EXP_AVG_SQ = 3 };
#define TS_SAME_BUFFERS(P) static_assert(P##_PARAM == TS_PARAM && P##_GRAD == TS_GRAD && P##_EXP_AVG == TS_EXP_AVG && P##_EXP_AVG_SQ == TS_EXP_AVG_SQ, #P)

struct TrainState {
    int64_t numel = 0;                   // floats of a parameter-shaped buffer
    std::vector<float> host;             // the parameters until finalize
    std::vector<char> have;              // per tensor: set_tensor has given it
    bool finalized = false;
    float *d_param = nullptr, *d_grad = nullptr, *d_m = nullptr, *d_v = nullptr;
    int64_t step = 0;
    int64_t fwd_N = 0;                   // rows or frames of the last forward, 0 when there is none
    const void *fwd_ws = nullptr;
};

template <class H>
auto ts_of(H *h) -> decltype(&h->ts) { return h ? &h->ts : nullptr; }

inline void ts_init(TrainState &s, int64_t numel, size_t tensors) {
    s.numel = numel;
    s.host.assign((size_t)numel, 0.f);
    s.have.assign(tensors, 0);
}

inline void ts_free(TrainState &s) {
    for (float *p : {s.d_param, s.d_grad, s.d_m, s.d_v})
        if (p) (void)hipFree(p);
}

// Bump allocator of a workspace layout: offsets in floats, every buffer on a 256-byte boundary.
struct WsTake {
    int64_t off = 0;
    int64_t operator()(int64_t floats) {
        const int64_t at = off;
        off += round_up(floats, 64);
        return at;
    }
    int64_t bytes() const { return off * 4; }
};

inline float *ts_buffer_of(TrainState &s, int what) {
    return what == TS_PARAM ? s.d_param : what == TS_GRAD ? s.d_grad : what == TS_EXP_AVG ? s.d_m : what == TS_EXP_AVG_SQ ? s.d_v : nullptr;
}

// The handle exists and is finalised: what every call of the step asks before it looks at anything else.
inline int ts_ready(const TrainState *s, const char *mod, const char *fn) {
    if (!s) return sdfa_fail(SDFA_EINVAL, "%s_%s: null handle", mod, fn);
    if (!s->finalized) return sdfa_fail(SDFA_ESTATE, "%s_%s: the handle is not finalised", mod, fn);
    return SDFA_OK;
}

inline int ts_check_ws(const char *mod, const char *fn, const void *d_ws, int64_t ws_bytes, int64_t need) {
    if (!d_ws) return sdfa_fail(SDFA_EINVAL, "%s_%s: null pointer", mod, fn);
    if (ws_bytes < need) return sdfa_fail(SDFA_EINVAL, "%s_%s: workspace of %lld bytes, %lld needed", mod, fn, (long long)ws_bytes, (long long)need);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "%s_%s: workspace not 256-byte aligned", mod, fn);
    return SDFA_OK;
}

// A backward needs the forward of the same N on the same workspace, with no parameter write in between; `unit`: "rows", "frames".
inline int ts_check_forward(const TrainState &s, const char *mod, int64_t N, const void *d_ws, const char *unit) {
    if (s.fwd_N != N || s.fwd_ws != d_ws)
        return sdfa_fail(SDFA_EINVAL, "%s_backward: no forward of %lld %s on this workspace precedes it", mod, (long long)N, unit);
    return SDFA_OK;
}

// The tensor in slot `slot`, which the module has located at `off`, from the host; before finalize only.
inline int ts_set_tensor(TrainState &s, const char *mod, int slot, int64_t off, const float *h_src, int64_t numel) {
    if (s.finalized) return sdfa_fail(SDFA_ESTATE, "%s_set_tensor: the handle is finalised (sdfa_%s_set_state writes a parameter then)", mod, mod);
    memcpy(s.host.data() + off, h_src, (size_t)numel * sizeof(float));
    s.have[slot] = 1;
    return SDFA_OK;
}

// What finalize refuses; name_of(slot) is the module's full name (std::string) of the first tensor set_tensor has not given.
template <class NameOf>
int ts_check_finalize(const TrainState *s, const char *mod, NameOf name_of) {
    if (!s) return sdfa_fail(SDFA_EINVAL, "%s_finalize: null handle", mod);
    if (s->finalized) return sdfa_fail(SDFA_ESTATE, "%s_finalize: already finalised", mod);
    for (size_t i = 0; i < s->have.size(); ++i)
        if (!s->have[i]) return sdfa_fail(SDFA_ESTATE, "%s_finalize: tensor \"%s\" is missing", mod, name_of((int)i).c_str());
    return SDFA_OK;
}

// The four buffers: the parameters from the host copy, which is released; gradients and moments zero.
inline int ts_finalize(TrainState &s, hipStream_t st) {
    const size_t nb = (size_t)s.numel * sizeof(float);
    HIP_TRY(hipMalloc((void **)&s.d_param, nb));
    HIP_TRY(hipMalloc((void **)&s.d_grad, nb));
    HIP_TRY(hipMalloc((void **)&s.d_m, nb));
    HIP_TRY(hipMalloc((void **)&s.d_v, nb));
    HIP_TRY(hipMemcpyAsync(s.d_param, s.host.data(), nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s.d_grad, 0, nb, st));
    HIP_TRY(hipMemsetAsync(s.d_m, 0, nb, st));
    HIP_TRY(hipMemsetAsync(s.d_v, 0, nb, st));
    HIP_TRY(hipStreamSynchronize(st));             // the host copy is released below
    std::vector<float>().swap(s.host);
    s.finalized = true;
    return SDFA_OK;
}

inline int ts_adam(TrainState *s, const char *mod, double lr, double beta1, double beta2, double eps, void *stream) {
    const int rc = ts_ready(s, mod, "adam");
    if (rc < 0) return rc;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return sdfa_fail(SDFA_EINVAL, "%s_adam: lr %g, betas (%g, %g), eps %g: torch.optim.Adam refuses these", mod, lr, beta1, beta2, eps);
    const int64_t t = s->step + 1;
    HIP_TRY(headtrain_adam_step(s->d_param, s->d_grad, s->d_m, s->d_v, s->numel, t, lr, beta1, beta2, eps, (hipStream_t)stream));
    s->step = t;
    s->fwd_N = 0;                                           // the kept activations belong to the old parameters
    return SDFA_OK;
}

inline int ts_zero_grad(TrainState *s, const char *mod, void *stream) {
    const int rc = ts_ready(s, mod, "zero_grad");
    if (rc < 0) return rc;
    HIP_TRY(hipMemsetAsync(s->d_grad, 0, (size_t)s->numel * sizeof(float), (hipStream_t)stream));
    return SDFA_OK;
}

// numel floats at `off`, which the module has located, of buffer `what` to the host.  The copy waits for the whole device: the
// step may be in flight on any stream.
inline int ts_get_tensor(TrainState &s, const char *mod, int what, int64_t off, float *h_dst, int64_t numel) {
    if (!s.finalized) return sdfa_fail(SDFA_ESTATE, "%s_get_tensor: the handle is not finalised", mod);
    const float *src = ts_buffer_of(s, what);
    if (!src) return sdfa_fail(SDFA_EINVAL, "%s_get_tensor: unknown buffer %d", mod, what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, src + off, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return SDFA_OK;
}

// The other way; a parameter write invalidates the kept forward.
inline int ts_set_state(TrainState &s, const char *mod, int what, int64_t off, const float *h_src, int64_t numel) {
    if (!s.finalized) return sdfa_fail(SDFA_ESTATE, "%s_set_state: the handle is not finalised", mod);
    float *dst = ts_buffer_of(s, what);
    if (!dst) return sdfa_fail(SDFA_EINVAL, "%s_set_state: unknown buffer %d", mod, what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst + off, h_src, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
    if (what == TS_PARAM) s.fwd_N = 0;
    return SDFA_OK;
}

inline int64_t ts_numel(const TrainState *s, const char *mod) { return s ? s->numel : sdfa_fail(SDFA_EINVAL, "%s_numel: null handle", mod); }
inline int64_t ts_step_count(const TrainState *s, const char *mod) { return s ? s->step : sdfa_fail(SDFA_EINVAL, "%s_step_count: null handle", mod); }

inline int ts_set_step_count(TrainState *s, const char *mod, int64_t t) {
    if (!s) return sdfa_fail(SDFA_EINVAL, "%s_set_step_count: null handle", mod);
    if (t < 0) return sdfa_fail(SDFA_EINVAL, "%s_set_step_count: %lld is negative", mod, (long long)t);
    s->step = t;
    return SDFA_OK;
}
