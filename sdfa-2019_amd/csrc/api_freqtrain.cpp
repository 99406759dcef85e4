// Host side of the frequency LSTM's training step (include/sdfa_freqtrain.h): the module's tensor names, the
// workspace layout and the launches of freqtrain.hip over the flat training state of trainstate.h.
#include "freqtrain.h"
#include "trainstate.h"

#include <string.h>

#include <string>

namespace {

const char *const MOD = "freqtrain";
TS_SAME_BUFFERS(SDFA_FREQTRAIN);
constexpr int NT = 10;
const char *const PREFIX = "_audio_encoder._layers.6.";
// without PREFIX, in the order of the flat layout (freqtrain.h)
const char *const NAME[NT] = {"_lstm.weight_ih_l0", "_lstm.weight_ih_l0_reverse", "_lstm.weight_hh_l0", "_lstm.weight_hh_l0_reverse",
                              "_lstm.bias_ih_l0",   "_lstm.bias_ih_l0_reverse",   "_lstm.bias_hh_l0",   "_lstm.bias_hh_l0_reverse",
                              "_proj.weight",       "_proj.bias"};
constexpr int64_t OFF[NT + 1] = {FT_OFF_WIH, FT_OFF_WIH + (int64_t)FT_G * FT_I, FT_OFF_WHH, FT_OFF_WHH + (int64_t)FT_G * FT_H,
                                 FT_OFF_BIH, FT_OFF_BIH + FT_G, FT_OFF_BHH, FT_OFF_BHH + FT_G, FT_OFF_WP, FT_OFF_BP, FT_NUMEL};

// Workspace of a batch of N frames, offsets in floats, every buffer on a 256-byte boundary.
struct Ws {
    int64_t gates, c, HF, dHF, img, imgT, part, total;
    int nblk;
};

Ws ws_layout(int64_t N) {
    Ws w;
    WsTake take;
    const int64_t R = N * FT_COLS;
    w.nblk = (int)((N + FT_BLOCK_FRAMES - 1) / FT_BLOCK_FRAMES);
    w.gates = take(2 * R * FT_S * FT_G);
    w.c = take(2 * R * FT_S * FT_H);
    w.HF = take(R * FT_K);
    w.dHF = take(R * FT_K);
    w.img = take(FT_IMG);
    w.imgT = take(FT_IMG);
    w.part = take((int64_t)w.nblk * FT_NUMEL);
    w.total = take.bytes();
    return w;
}

}  // namespace

struct sdfa_freqtrain {
    TrainState ts;                       // a slot per tensor
};

namespace {

// The slot of tensor `name`; `data` is the caller's host pointer, refused first.
int locate(const sdfa_freqtrain *h, const char *who, const char *name, const void *data, int64_t numel) {
    if (!data || !h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    const size_t np = strlen(PREFIX);
    int ti = -1;
    if (strncmp(name, PREFIX, np) == 0)
        for (int i = 0; i < NT; ++i)
            if (strcmp(name + np, NAME[i]) == 0) ti = i;
    if (ti < 0) return sdfa_fail(SDFA_EINVAL, "%s: the frequency LSTM has no tensor \"%s\"", who, name);
    const int64_t want = OFF[ti + 1] - OFF[ti];
    if (numel != want) return sdfa_fail(SDFA_EINVAL, "%s: \"%s\" has %lld elements, %lld given", who, name, (long long)want, (long long)numel);
    return ti;
}

int check_call(const sdfa_freqtrain *h, const char *fn, int64_t N, const void *d_ws, int64_t ws_bytes) {
    const int rc = ts_ready(ts_of(h), MOD, fn);
    if (rc < 0) return rc;
    if (N < 1 || N > SDFA_FREQTRAIN_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "freqtrain_%s: %lld frames outside 1 .. %d", fn, (long long)N, SDFA_FREQTRAIN_MAX_FRAMES);
    return ts_check_ws(MOD, fn, d_ws, ws_bytes, ws_layout(N).total);
}

}  // namespace

extern "C" {

int sdfa_freqtrain_abi_version(void) { return SDFA_FREQTRAIN_ABI_VERSION; }

sdfa_freqtrain *sdfa_freqtrain_create(void) {
    sdfa_freqtrain *h = new sdfa_freqtrain();
    ts_init(h->ts, FT_NUMEL, NT);
    return h;
}

void sdfa_freqtrain_destroy(sdfa_freqtrain *h) {
    if (!h) return;
    ts_free(h->ts);
    delete h;
}

int sdfa_freqtrain_set_tensor(sdfa_freqtrain *h, const char *name, const float *h_src, int64_t numel) {
    const int ti = locate(h, "freqtrain_set_tensor", name, h_src, numel);
    return ti < 0 ? ti : ts_set_tensor(h->ts, MOD, ti, OFF[ti], h_src, numel);
}

int sdfa_freqtrain_finalize(sdfa_freqtrain *h, void *stream) {
    const int rc = ts_check_finalize(ts_of(h), MOD, [&](int ti) { return std::string(PREFIX) + NAME[ti]; });
    return rc < 0 ? rc : ts_finalize(h->ts, (hipStream_t)stream);
}

int64_t sdfa_freqtrain_numel(const sdfa_freqtrain *h) { return ts_numel(ts_of(h), MOD); }

int64_t sdfa_freqtrain_workspace_bytes(const sdfa_freqtrain *h, int64_t max_frames) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "freqtrain_workspace_bytes: null handle");
    if (max_frames < 1 || max_frames > SDFA_FREQTRAIN_MAX_FRAMES)
        return sdfa_fail(SDFA_EINVAL, "freqtrain_workspace_bytes: %lld frames outside 1 .. %d", (long long)max_frames, SDFA_FREQTRAIN_MAX_FRAMES);
    return ws_layout(max_frames).total;
}

int sdfa_freqtrain_forward(sdfa_freqtrain *h, const float *d_C, int64_t N, float *d_X0, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_C || !d_X0) return sdfa_fail(SDFA_EINVAL, "freqtrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    const float *P = h->ts.d_param;
    h->ts.fwd_N = 0;                                        // a forward that fails half way is no forward
    FtImagesArgs im;
    im.Whh = P + FT_OFF_WHH;
    im.img = f + w.img;
    im.imgT = f + w.imgT;
    HIP_TRY(freqtrain_images(im, st));
    FtPreArgs p;
    p.C = d_C;
    p.P = P;
    p.gates = f + w.gates;
    p.N = N;
    HIP_TRY(freqtrain_pre(p, st));
    FtFwdArgs a;
    a.img = f + w.img;
    a.gates = f + w.gates;
    a.c = f + w.c;
    a.HF = f + w.HF;
    a.N = N;
    HIP_TRY(freqtrain_forward(a, st));
    FtProjArgs j;
    j.HF = f + w.HF;
    j.P = P;
    j.X0 = d_X0;
    j.N = N;
    HIP_TRY(freqtrain_proj(j, st));
    h->ts.fwd_N = N;
    h->ts.fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_freqtrain_backward(sdfa_freqtrain *h, const float *d_C, const float *d_dX0, int64_t N, float *d_dC, void *d_ws,
                            int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_C || !d_dX0) return sdfa_fail(SDFA_EINVAL, "freqtrain_backward: null pointer");
    const int rf = ts_check_forward(h->ts, MOD, N, d_ws, "frames");
    if (rf < 0) return rf;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    const float *P = h->ts.d_param;
    h->ts.fwd_N = 0;                                        // the kept gates become dG: one backward per forward
    FtDhfArgs d;
    d.dX0 = d_dX0;
    d.P = P;
    d.dHF = f + w.dHF;
    d.N = N;
    HIP_TRY(freqtrain_dhf(d, st));
    FtBwdArgs b;
    b.imgT = f + w.imgT;
    b.c = f + w.c;
    b.dHF = f + w.dHF;
    b.gates = f + w.gates;
    b.N = N;
    HIP_TRY(freqtrain_backward(b, st));
    FtProdArgs p;
    p.C = d_C;
    p.HF = f + w.HF;
    p.dX0 = d_dX0;
    p.gates = f + w.gates;
    p.P = P;
    p.part = f + w.part;
    p.dC = d_dC;
    p.N = N;
    p.nblk = w.nblk;
    HIP_TRY(freqtrain_products(p, st));
    FtReduceArgs r;
    r.part = f + w.part;
    r.grad = h->ts.d_grad;
    r.nblk = w.nblk;
    HIP_TRY(freqtrain_reduce(r, st));
    return SDFA_OK;
}

int sdfa_freqtrain_adam(sdfa_freqtrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    return ts_adam(ts_of(h), MOD, lr, beta1, beta2, eps, stream);
}

int sdfa_freqtrain_zero_grad(sdfa_freqtrain *h, void *stream) { return ts_zero_grad(ts_of(h), MOD, stream); }

int sdfa_freqtrain_get_tensor(sdfa_freqtrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    const int ti = locate(h, "freqtrain_get_tensor", name, h_dst, numel);
    return ti < 0 ? ti : ts_get_tensor(h->ts, MOD, what, OFF[ti], h_dst, numel);
}

int sdfa_freqtrain_set_state(sdfa_freqtrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    const int ti = locate(h, "freqtrain_set_state", name, h_src, numel);
    return ti < 0 ? ti : ts_set_state(h->ts, MOD, what, OFF[ti], h_src, numel);
}

int sdfa_freqtrain_set_grad(sdfa_freqtrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_freqtrain_set_state(h, name, SDFA_FREQTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_freqtrain_step_count(const sdfa_freqtrain *h) { return ts_step_count(ts_of(h), MOD); }
int sdfa_freqtrain_set_step_count(sdfa_freqtrain *h, int64_t t) { return ts_set_step_count(ts_of(h), MOD, t); }

}  // extern "C"
