// Host side of a bidirectional LSTM layer's training step (include/sdfa_lstmtrain.h): the handle and its
// flat device buffers, the refusals, the workspace layout and the launches of lstmtrain.hip.  Adam is headtrain.hip's kernel.
#include "host.h"
#include "lstmtrain.h"
#include "headtrain.h"

#include <stdio.h>
#include <string.h>

#include <vector>

namespace {

constexpr int NT = 4;
const char *const PREFIX = "_audio_encoder._layers.9.";
const char *const STEM[NT] = {"weight_ih_l%d", "weight_ih_l%d_reverse", "weight_hh_l%d", "weight_hh_l%d_reverse"};
enum { WIH = 0, WHH = 2 };

// Workspace of a batch of N frames, offsets in floats, every buffer on a 256-byte boundary.
struct Ws {
    int64_t gates, c, img, imgT, part, total;
    int nblk;
};

Ws ws_layout(int64_t N, int64_t numel) {
    Ws w;
    int64_t off = 0;
    auto take = [&](int64_t floats) {
        const int64_t at = off;
        off += round_up(floats, 64);
        return at;
    };
    w.nblk = (int)((N + LT_BLOCK_FRAMES - 1) / LT_BLOCK_FRAMES);
    w.gates = take(2 * N * LT_T * LT_G);
    w.c = take(2 * N * LT_T * LT_H);
    w.img = take(LT_IMG);
    w.imgT = take(LT_IMG);
    w.part = take((int64_t)w.nblk * numel);
    w.total = off * 4;
    return w;
}

}  // namespace

struct sdfa_lstmtrain {
    int in_dim, layer;
    char name[NT][64];                   // without PREFIX
    int64_t off[NT + 1];
    std::vector<float> host;             // the parameters until finalize
    char have[NT];
    bool finalized;
    float *d_param, *d_grad, *d_m, *d_v;
    int64_t step;
    int64_t fwd_N;                       // frames of the last forward, 0 when there is none
    const void *fwd_ws;
};

namespace {

int locate(const sdfa_lstmtrain *h, const char *who, const char *name, int64_t numel) {
    if (!h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    const size_t np = strlen(PREFIX);
    int ti = -1;
    if (strncmp(name, PREFIX, np) == 0)
        for (int i = 0; i < NT; ++i)
            if (strcmp(name + np, h->name[i]) == 0) ti = i;
    if (ti < 0) return sdfa_fail(SDFA_EINVAL, "%s: layer %d of the BiLSTM has no tensor \"%s\"", who, h->layer, name);
    const int64_t want = h->off[ti + 1] - h->off[ti];
    if (numel != want) return sdfa_fail(SDFA_EINVAL, "%s: \"%s\" has %lld elements, %lld given", who, name, (long long)want, (long long)numel);
    return ti;
}

float *buffer_of(sdfa_lstmtrain *h, int what) {
    return what == SDFA_LSTMTRAIN_PARAM ? h->d_param : what == SDFA_LSTMTRAIN_GRAD ? h->d_grad : what == SDFA_LSTMTRAIN_EXP_AVG ? h->d_m
         : what == SDFA_LSTMTRAIN_EXP_AVG_SQ ? h->d_v : nullptr;
}

int check_call(const sdfa_lstmtrain *h, const char *who, int64_t N, const void *d_ws, int64_t ws_bytes) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "%s: null handle", who);
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "%s: the handle is not finalised", who);
    if (N < 1 || N > SDFA_LSTMTRAIN_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "%s: %lld frames outside 1 .. %d", who, (long long)N, SDFA_LSTMTRAIN_MAX_FRAMES);
    if (!d_ws) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    const int64_t need = ws_layout(N, h->off[NT]).total;
    if (ws_bytes < need) return sdfa_fail(SDFA_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)need);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "%s: workspace not 256-byte aligned", who);
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_lstmtrain_abi_version(void) { return SDFA_LSTMTRAIN_ABI_VERSION; }

sdfa_lstmtrain *sdfa_lstmtrain_create(int in_dim) {
    if (in_dim != 256 && in_dim != 512) {
        sdfa_fail(SDFA_EINVAL, "lstmtrain_create: input width %d; the encoder's BiLSTM has 256 (layer 0) and 512 (layer 1)", in_dim);
        return nullptr;
    }
    sdfa_lstmtrain *h = new sdfa_lstmtrain();
    h->in_dim = in_dim;
    h->layer = in_dim == 256 ? 0 : 1;
    h->off[0] = 0;
    for (int i = 0; i < NT; ++i) {
        snprintf(h->name[i], sizeof h->name[i], STEM[i], h->layer);
        h->off[i + 1] = h->off[i] + (int64_t)LT_G * (i < WHH ? in_dim : LT_H);
        h->have[i] = 0;
    }
    h->host.assign((size_t)h->off[NT], 0.f);
    h->finalized = false;
    h->d_param = h->d_grad = h->d_m = h->d_v = nullptr;
    h->step = 0;
    h->fwd_N = 0;
    h->fwd_ws = nullptr;
    return h;
}

void sdfa_lstmtrain_destroy(sdfa_lstmtrain *h) {
    if (!h) return;
    for (float *p : {h->d_param, h->d_grad, h->d_m, h->d_v})
        if (p) (void)hipFree(p);
    delete h;
}

int sdfa_lstmtrain_set_tensor(sdfa_lstmtrain *h, const char *name, const float *h_src, int64_t numel) {
    if (!h_src) return sdfa_fail(SDFA_EINVAL, "lstmtrain_set_tensor: null pointer");
    const int ti = locate(h, "lstmtrain_set_tensor", name, numel);
    if (ti < 0) return ti;
    if (h->finalized) return sdfa_fail(SDFA_ESTATE, "lstmtrain_set_tensor: the handle is finalised (sdfa_lstmtrain_set_state writes a parameter then)");
    memcpy(h->host.data() + h->off[ti], h_src, (size_t)numel * sizeof(float));
    h->have[ti] = 1;
    return SDFA_OK;
}

int sdfa_lstmtrain_finalize(sdfa_lstmtrain *h, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "lstmtrain_finalize: null handle");
    if (h->finalized) return sdfa_fail(SDFA_ESTATE, "lstmtrain_finalize: already finalised");
    for (int i = 0; i < NT; ++i)
        if (!h->have[i]) return sdfa_fail(SDFA_ESTATE, "lstmtrain_finalize: tensor \"%s%s\" is missing", PREFIX, h->name[i]);
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)h->off[NT] * sizeof(float);
    HIP_TRY(hipMalloc((void **)&h->d_param, nb));
    HIP_TRY(hipMalloc((void **)&h->d_grad, nb));
    HIP_TRY(hipMalloc((void **)&h->d_m, nb));
    HIP_TRY(hipMalloc((void **)&h->d_v, nb));
    HIP_TRY(hipMemcpyAsync(h->d_param, h->host.data(), nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->d_grad, 0, nb, st));
    HIP_TRY(hipMemsetAsync(h->d_m, 0, nb, st));
    HIP_TRY(hipMemsetAsync(h->d_v, 0, nb, st));
    HIP_TRY(hipStreamSynchronize(st));             // the host copy is released below
    std::vector<float>().swap(h->host);
    h->finalized = true;
    return SDFA_OK;
}

int64_t sdfa_lstmtrain_numel(const sdfa_lstmtrain *h) { return h ? h->off[NT] : sdfa_fail(SDFA_EINVAL, "lstmtrain_numel: null handle"); }

int64_t sdfa_lstmtrain_workspace_bytes(const sdfa_lstmtrain *h, int64_t max_frames) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "lstmtrain_workspace_bytes: null handle");
    if (max_frames < 1 || max_frames > SDFA_LSTMTRAIN_MAX_FRAMES)
        return sdfa_fail(SDFA_EINVAL, "lstmtrain_workspace_bytes: %lld frames outside 1 .. %d", (long long)max_frames, SDFA_LSTMTRAIN_MAX_FRAMES);
    return ws_layout(max_frames, h->off[NT]).total;
}

int sdfa_lstmtrain_forward(sdfa_lstmtrain *h, const float *d_X, int64_t N, float *d_Y, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "lstmtrain_forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_X || !d_Y) return sdfa_fail(SDFA_EINVAL, "lstmtrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N, h->off[NT]);
    float *f = (float *)d_ws;
    const float *P = h->d_param;
    h->fwd_N = 0;                                           // a forward that fails half way is no forward
    LtImagesArgs im;
    im.Whh = P + h->off[WHH];
    im.img = f + w.img;
    im.imgT = f + w.imgT;
    HIP_TRY(lstmtrain_images(im, st));
    LtPreArgs p;
    p.X = d_X;
    p.Wih = P + h->off[WIH];
    p.gates = f + w.gates;
    p.N = N;
    p.I = h->in_dim;
    HIP_TRY(lstmtrain_pre(p, st));
    LtFwdArgs a;
    a.img = f + w.img;
    a.gates = f + w.gates;
    a.c = f + w.c;
    a.Y = d_Y;
    a.N = N;
    HIP_TRY(lstmtrain_forward(a, st));
    h->fwd_N = N;
    h->fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_lstmtrain_backward(sdfa_lstmtrain *h, const float *d_X, const float *d_Y, const float *d_dY, int64_t N, float *d_dX,
                            void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "lstmtrain_backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_X || !d_Y || !d_dY) return sdfa_fail(SDFA_EINVAL, "lstmtrain_backward: null pointer");
    if (h->fwd_N != N || h->fwd_ws != d_ws)
        return sdfa_fail(SDFA_EINVAL, "lstmtrain_backward: no forward of %lld frames on this workspace precedes it", (long long)N);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N, h->off[NT]);
    float *f = (float *)d_ws;
    h->fwd_N = 0;                                           // the kept gates become dG: one backward per forward
    LtBwdArgs b;
    b.imgT = f + w.imgT;
    b.c = f + w.c;
    b.dY = d_dY;
    b.gates = f + w.gates;
    b.N = N;
    HIP_TRY(lstmtrain_backward(b, st));
    LtProdArgs p;
    p.X = d_X;
    p.Y = d_Y;
    p.gates = f + w.gates;
    p.Wih = h->d_param + h->off[WIH];
    p.part = f + w.part;
    p.dX = d_dX;
    p.N = N;
    p.I = h->in_dim;
    p.nblk = w.nblk;
    HIP_TRY(lstmtrain_products(p, st));
    LtReduceArgs r;
    r.part = f + w.part;
    r.grad = h->d_grad;
    r.numel = h->off[NT];
    r.nblk = w.nblk;
    HIP_TRY(lstmtrain_reduce(r, st));
    return SDFA_OK;
}

int sdfa_lstmtrain_adam(sdfa_lstmtrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "lstmtrain_adam: null handle");
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "lstmtrain_adam: the handle is not finalised");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return sdfa_fail(SDFA_EINVAL, "lstmtrain_adam: lr %g, betas (%g, %g), eps %g: torch.optim.Adam refuses these", lr, beta1, beta2, eps);
    const int64_t t = h->step + 1;
    HIP_TRY(headtrain_adam_step(h->d_param, h->d_grad, h->d_m, h->d_v, h->off[NT], t, lr, beta1, beta2, eps, (hipStream_t)stream));
    h->step = t;
    h->fwd_N = 0;                                           // the kept activations belong to the old parameters
    return SDFA_OK;
}

int sdfa_lstmtrain_zero_grad(sdfa_lstmtrain *h, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "lstmtrain_zero_grad: null handle");
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "lstmtrain_zero_grad: the handle is not finalised");
    HIP_TRY(hipMemsetAsync(h->d_grad, 0, (size_t)h->off[NT] * sizeof(float), (hipStream_t)stream));
    return SDFA_OK;
}

int sdfa_lstmtrain_get_tensor(sdfa_lstmtrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    if (!h_dst) return sdfa_fail(SDFA_EINVAL, "lstmtrain_get_tensor: null pointer");
    const int ti = locate(h, "lstmtrain_get_tensor", name, numel);
    if (ti < 0) return ti;
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "lstmtrain_get_tensor: the handle is not finalised");
    const float *src = buffer_of(h, what);
    if (!src) return sdfa_fail(SDFA_EINVAL, "lstmtrain_get_tensor: unknown buffer %d", what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, src + h->off[ti], (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return SDFA_OK;
}

int sdfa_lstmtrain_set_state(sdfa_lstmtrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    if (!h_src) return sdfa_fail(SDFA_EINVAL, "lstmtrain_set_state: null pointer");
    const int ti = locate(h, "lstmtrain_set_state", name, numel);
    if (ti < 0) return ti;
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "lstmtrain_set_state: the handle is not finalised");
    float *dst = buffer_of(h, what);
    if (!dst) return sdfa_fail(SDFA_EINVAL, "lstmtrain_set_state: unknown buffer %d", what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst + h->off[ti], h_src, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
    if (what == SDFA_LSTMTRAIN_PARAM) h->fwd_N = 0;
    return SDFA_OK;
}

int sdfa_lstmtrain_set_grad(sdfa_lstmtrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_lstmtrain_set_state(h, name, SDFA_LSTMTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_lstmtrain_step_count(const sdfa_lstmtrain *h) { return h ? h->step : sdfa_fail(SDFA_EINVAL, "lstmtrain_step_count: null handle"); }

int sdfa_lstmtrain_set_step_count(sdfa_lstmtrain *h, int64_t t) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "lstmtrain_set_step_count: null handle");
    if (t < 0) return sdfa_fail(SDFA_EINVAL, "lstmtrain_set_step_count: %lld is negative", (long long)t);
    h->step = t;
    return SDFA_OK;
}

}  // extern "C"
