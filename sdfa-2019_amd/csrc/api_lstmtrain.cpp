// Host side of a bidirectional LSTM layer's training step (include/sdfa_lstmtrain.h): the layer's tensor
// names, the workspace layout and the launches of lstmtrain.hip over the flat training state of trainstate.h.
#include "lstmtrain.h"
#include "trainstate.h"

#include <stdio.h>
#include <string.h>

#include <string>

namespace {

const char *const MOD = "lstmtrain";
TS_SAME_BUFFERS(SDFA_LSTMTRAIN);
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
    WsTake take;
    w.nblk = (int)((N + LT_BLOCK_FRAMES - 1) / LT_BLOCK_FRAMES);
    w.gates = take(2 * N * LT_T * LT_G);
    w.c = take(2 * N * LT_T * LT_H);
    w.img = take(LT_IMG);
    w.imgT = take(LT_IMG);
    w.part = take((int64_t)w.nblk * numel);
    w.total = take.bytes();
    return w;
}

}  // namespace

struct sdfa_lstmtrain {
    int in_dim, layer;
    char name[NT][64];                   // without PREFIX
    int64_t off[NT + 1];
    TrainState ts;                       // a slot per tensor
};

namespace {

// The slot of tensor `name`; `data` is the caller's host pointer, refused first.
int locate(const sdfa_lstmtrain *h, const char *who, const char *name, const void *data, int64_t numel) {
    if (!data || !h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
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

int check_call(const sdfa_lstmtrain *h, const char *fn, int64_t N, const void *d_ws, int64_t ws_bytes) {
    const int rc = ts_ready(ts_of(h), MOD, fn);
    if (rc < 0) return rc;
    if (N < 1 || N > SDFA_LSTMTRAIN_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "lstmtrain_%s: %lld frames outside 1 .. %d", fn, (long long)N, SDFA_LSTMTRAIN_MAX_FRAMES);
    return ts_check_ws(MOD, fn, d_ws, ws_bytes, ws_layout(N, h->off[NT]).total);
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
    }
    ts_init(h->ts, h->off[NT], NT);
    return h;
}

void sdfa_lstmtrain_destroy(sdfa_lstmtrain *h) {
    if (!h) return;
    ts_free(h->ts);
    delete h;
}

int sdfa_lstmtrain_set_tensor(sdfa_lstmtrain *h, const char *name, const float *h_src, int64_t numel) {
    const int ti = locate(h, "lstmtrain_set_tensor", name, h_src, numel);
    return ti < 0 ? ti : ts_set_tensor(h->ts, MOD, ti, h->off[ti], h_src, numel);
}

int sdfa_lstmtrain_finalize(sdfa_lstmtrain *h, void *stream) {
    const int rc = ts_check_finalize(ts_of(h), MOD, [&](int ti) { return std::string(PREFIX) + h->name[ti]; });
    return rc < 0 ? rc : ts_finalize(h->ts, (hipStream_t)stream);
}

int64_t sdfa_lstmtrain_numel(const sdfa_lstmtrain *h) { return ts_numel(ts_of(h), MOD); }

int64_t sdfa_lstmtrain_workspace_bytes(const sdfa_lstmtrain *h, int64_t max_frames) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "lstmtrain_workspace_bytes: null handle");
    if (max_frames < 1 || max_frames > SDFA_LSTMTRAIN_MAX_FRAMES)
        return sdfa_fail(SDFA_EINVAL, "lstmtrain_workspace_bytes: %lld frames outside 1 .. %d", (long long)max_frames, SDFA_LSTMTRAIN_MAX_FRAMES);
    return ws_layout(max_frames, h->off[NT]).total;
}

int sdfa_lstmtrain_forward(sdfa_lstmtrain *h, const float *d_X, int64_t N, float *d_Y, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_X || !d_Y) return sdfa_fail(SDFA_EINVAL, "lstmtrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N, h->off[NT]);
    float *f = (float *)d_ws;
    const float *P = h->ts.d_param;
    h->ts.fwd_N = 0;                                        // a forward that fails half way is no forward
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
    h->ts.fwd_N = N;
    h->ts.fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_lstmtrain_backward(sdfa_lstmtrain *h, const float *d_X, const float *d_Y, const float *d_dY, int64_t N, float *d_dX,
                            void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_X || !d_Y || !d_dY) return sdfa_fail(SDFA_EINVAL, "lstmtrain_backward: null pointer");
    const int rf = ts_check_forward(h->ts, MOD, N, d_ws, "frames");
    if (rf < 0) return rf;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N, h->off[NT]);
    float *f = (float *)d_ws;
    h->ts.fwd_N = 0;                                        // the kept gates become dG: one backward per forward
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
    p.Wih = h->ts.d_param + h->off[WIH];
    p.part = f + w.part;
    p.dX = d_dX;
    p.N = N;
    p.I = h->in_dim;
    p.nblk = w.nblk;
    HIP_TRY(lstmtrain_products(p, st));
    LtReduceArgs r;
    r.part = f + w.part;
    r.grad = h->ts.d_grad;
    r.numel = h->off[NT];
    r.nblk = w.nblk;
    HIP_TRY(lstmtrain_reduce(r, st));
    return SDFA_OK;
}

int sdfa_lstmtrain_adam(sdfa_lstmtrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    return ts_adam(ts_of(h), MOD, lr, beta1, beta2, eps, stream);
}

int sdfa_lstmtrain_zero_grad(sdfa_lstmtrain *h, void *stream) { return ts_zero_grad(ts_of(h), MOD, stream); }

int sdfa_lstmtrain_get_tensor(sdfa_lstmtrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    const int ti = locate(h, "lstmtrain_get_tensor", name, h_dst, numel);
    return ti < 0 ? ti : ts_get_tensor(h->ts, MOD, what, h->off[ti], h_dst, numel);
}

int sdfa_lstmtrain_set_state(sdfa_lstmtrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    const int ti = locate(h, "lstmtrain_set_state", name, h_src, numel);
    return ti < 0 ? ti : ts_set_state(h->ts, MOD, what, h->off[ti], h_src, numel);
}

int sdfa_lstmtrain_set_grad(sdfa_lstmtrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_lstmtrain_set_state(h, name, SDFA_LSTMTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_lstmtrain_step_count(const sdfa_lstmtrain *h) { return ts_step_count(ts_of(h), MOD); }
int sdfa_lstmtrain_set_step_count(sdfa_lstmtrain *h, int64_t t) { return ts_set_step_count(ts_of(h), MOD, t); }

}  // extern "C"
