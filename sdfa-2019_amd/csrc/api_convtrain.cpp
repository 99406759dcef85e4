// Host side of the conv stack's training step (include/sdfa_convtrain.h): the module's tensor names, its
// constants, the workspace layout and the launches of convtrain.hip over the flat training state of trainstate.h.  The weight
// norm's fold and its backward are headtrain.hip's launches over this module's layer table.
#include "convtrain.h"
#include "headtrain.h"
#include "trainstate.h"

#include <string.h>

#include <string>

namespace {

const char *const MOD = "convtrain";
TS_SAME_BUFFERS(SDFA_CONVTRAIN);
constexpr int NL = 3, NPER = 5, NCPER = 2, NT = NL * NPER, NC = NL * NCPER;
const char *const PREFIX = "_audio_encoder._layers.";
const int LAYER[NL] = {1, 3, 5};
// after PREFIX and "L.", in the order of the flat layout (convtrain.h); then the constants
const char *const NAME[NPER + NCPER] = {"weight_g", "weight_v", "bias", "_ext_post_bn.weight", "_ext_post_bn.bias",
                                        "_ext_post_bn.running_mean", "_ext_post_bn.running_var"};
constexpr int CO[NL] = {CT_C1, CT_C3, CT_C5}, KK[NL] = {CT_K1, CT_K3, CT_K5};
constexpr int64_t LOFF[NL] = {CT_OFF1, CT_OFF3, CT_OFF5};
constexpr int COFF[NL] = {CT_CONST1, CT_CONST3, CT_CONST5};

// tensor ti < NT is trainable (layer ti / NPER, kind ti % NPER); NT + i is a constant (layer i / NCPER, mean or var)
bool is_const(int ti) { return ti >= NT; }
int64_t numel_of(int ti) {
    if (is_const(ti)) return CO[(ti - NT) / NCPER];
    return ti % NPER == 1 ? (int64_t)CO[ti / NPER] * KK[ti / NPER] : CO[ti / NPER];
}
int64_t offset_of(int ti) {      // in the flat layout, or among the constants
    if (is_const(ti)) return COFF[(ti - NT) / NCPER] + (ti - NT) % NCPER * CO[(ti - NT) / NCPER];
    const int li = ti / NPER, k = ti % NPER, co = CO[li];
    return LOFF[li] + (k == 0 ? 0 : k == 1 ? co : co + (int64_t)co * KK[li] + (k - 2) * co);
}
std::string name_of(int ti) {
    const int li = is_const(ti) ? (ti - NT) / NCPER : ti / NPER, k = is_const(ti) ? NPER + (ti - NT) % NCPER : ti % NPER;
    return std::string(PREFIX) + std::to_string(LAYER[li]) + "." + NAME[k];
}

// Workspace of a batch of N frames, offsets in floats, every buffer on a 256-byte boundary.
struct Ws {
    int64_t a1, a3, a5, p1, p3, dp1, dp3, q1, q3, q5, W, dW, inv, sc, part, total;
    int nblk;
};

Ws ws_layout(int64_t N) {
    Ws w;
    WsTake take;
    const int64_t R = N * CT_COLS;
    w.nblk = (int)((N + CT_BLOCK_FRAMES - 1) / CT_BLOCK_FRAMES);
    w.a1 = take(R * CT_F1 * CT_C1);
    w.a3 = take(R * CT_F3 * CT_C3);
    w.a5 = take(R * CT_F5 * CT_C5);
    w.p1 = take(R * CT_F3 * CT_C1);
    w.p3 = take(R * CT_F5 * CT_C3);
    w.dp1 = take(R * CT_F3 * CT_C1);
    w.dp3 = take(R * CT_F5 * CT_C3);
    w.q1 = take(R * CT_F3 * CT_C1);
    w.q3 = take(R * CT_F5 * CT_C3);
    w.q5 = take(R * CT_F5 * CT_C5);
    w.W = take(CT_NUMEL);
    w.dW = take(CT_NUMEL);
    w.inv = take(CT_ROWS);
    w.sc = take(CT_ROWS);
    w.part = take((int64_t)w.nblk * CT_NUMEL);
    w.total = take.bytes();
    return w;
}

}  // namespace

struct sdfa_convtrain {
    TrainState ts;                       // a slot per trainable tensor
    HtTable t;                           // the three layers as rows of weight-normed matrices: [co][ci kf]
    float consts[CT_CONSTS];             // running_mean and running_var until finalize
    char have_const[NC];
    float *d_const = nullptr;
};

namespace {

// The tensor `name`; `data` is the caller's host pointer, refused first.
int locate(const sdfa_convtrain *h, const char *who, const char *name, const void *data, int64_t numel) {
    if (!data || !h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    int ti = -1;
    for (int i = 0; i < NT + NC; ++i)
        if (name_of(i) == name) ti = i;
    if (ti < 0) return sdfa_fail(SDFA_EINVAL, "%s: the conv stack has no tensor \"%s\"", who, name);
    const int64_t want = numel_of(ti);
    if (numel != want) return sdfa_fail(SDFA_EINVAL, "%s: \"%s\" has %lld elements, %lld given", who, name, (long long)want, (long long)numel);
    return ti;
}

int check_call(const sdfa_convtrain *h, const char *fn, int64_t N, const void *d_ws, int64_t ws_bytes) {
    const int rc = ts_ready(ts_of(h), MOD, fn);
    if (rc < 0) return rc;
    if (N < 1 || N > SDFA_CONVTRAIN_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "convtrain_%s: %lld frames outside 1 .. %d", fn, (long long)N, SDFA_CONVTRAIN_MAX_FRAMES);
    return ts_check_ws(MOD, fn, d_ws, ws_bytes, ws_layout(N).total);
}

CtArgs args_of(const sdfa_convtrain *h, const float *d_feat, int64_t N, void *d_ws) {
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    CtArgs a = {};
    a.feat = d_feat;
    a.P = h->ts.d_param;
    a.K = h->d_const;
    a.W = f + w.W;
    a.a1 = f + w.a1;
    a.a3 = f + w.a3;
    a.a5 = f + w.a5;
    a.p1 = f + w.p1;
    a.p3 = f + w.p3;
    a.dp1 = f + w.dp1;
    a.dp3 = f + w.dp3;
    a.q1 = f + w.q1;
    a.q3 = f + w.q3;
    a.q5 = f + w.q5;
    a.part = f + w.part;
    a.dW = f + w.dW;
    a.grad = h->ts.d_grad;
    a.N = N;
    a.nblk = w.nblk;
    return a;
}

}  // namespace

extern "C" {

int sdfa_convtrain_abi_version(void) { return SDFA_CONVTRAIN_ABI_VERSION; }

sdfa_convtrain *sdfa_convtrain_create(void) {
    sdfa_convtrain *h = new sdfa_convtrain();
    ts_init(h->ts, CT_NUMEL, NT);
    memset(h->consts, 0, sizeof(h->consts));
    memset(h->have_const, 0, sizeof(h->have_const));
    memset(&h->t, 0, sizeof(h->t));
    h->t.nl = NL;
    h->t.rows = CT_ROWS;
    int row = 0;
    for (int li = 0; li < NL; ++li) {
        HtLayer &L = h->t.l[li];
        L.P = CO[li];
        L.K = L.Kin = KK[li];
        L.row0 = row;
        L.og = offset_of(li * NPER);
        L.ov = L.ow = offset_of(li * NPER + 1);          // W and dW lie in the parameter layout, at v's place
        L.ob = offset_of(li * NPER + 2);
        row += CO[li];
    }
    return h;
}

void sdfa_convtrain_destroy(sdfa_convtrain *h) {
    if (!h) return;
    ts_free(h->ts);
    if (h->d_const) (void)hipFree(h->d_const);
    delete h;
}

int sdfa_convtrain_set_tensor(sdfa_convtrain *h, const char *name, const float *h_src, int64_t numel) {
    const int ti = locate(h, "convtrain_set_tensor", name, h_src, numel);
    if (ti < 0) return ti;
    if (!is_const(ti)) return ts_set_tensor(h->ts, MOD, ti, offset_of(ti), h_src, numel);
    if (h->ts.finalized) return sdfa_fail(SDFA_ESTATE, "convtrain_set_tensor: the handle is finalised (\"%s\" is a constant)", name);
    memcpy(h->consts + offset_of(ti), h_src, (size_t)numel * sizeof(float));
    h->have_const[ti - NT] = 1;
    return SDFA_OK;
}

int sdfa_convtrain_finalize(sdfa_convtrain *h, void *stream) {
    const int rc = ts_check_finalize(ts_of(h), MOD, name_of);
    if (rc < 0) return rc;
    for (int i = 0; i < NC; ++i)
        if (!h->have_const[i]) return sdfa_fail(SDFA_ESTATE, "convtrain_finalize: tensor \"%s\" is missing", name_of(NT + i).c_str());
    // the constants first, into a buffer the handle takes only once both uploads stand: a finalize that fails leaves nothing behind
    float *d_const = nullptr;
    HIP_TRY(hipMalloc((void **)&d_const, sizeof(h->consts)));
    const hipError_t e = hipMemcpy(d_const, h->consts, sizeof(h->consts), hipMemcpyHostToDevice);
    const int rf = e != hipSuccess ? sdfa_fail(SDFA_EHIP, "convtrain_finalize: the constants' upload failed: %s", hipGetErrorString(e))
                                   : ts_finalize(h->ts, (hipStream_t)stream);
    if (rf < 0) {
        (void)hipFree(d_const);
        return rf;
    }
    h->d_const = d_const;
    return SDFA_OK;
}

int64_t sdfa_convtrain_numel(const sdfa_convtrain *h) { return ts_numel(ts_of(h), MOD); }

int64_t sdfa_convtrain_workspace_bytes(const sdfa_convtrain *h, int64_t max_frames) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "convtrain_workspace_bytes: null handle");
    if (max_frames < 1 || max_frames > SDFA_CONVTRAIN_MAX_FRAMES)
        return sdfa_fail(SDFA_EINVAL, "convtrain_workspace_bytes: %lld frames outside 1 .. %d", (long long)max_frames, SDFA_CONVTRAIN_MAX_FRAMES);
    return ws_layout(max_frames).total;
}

int sdfa_convtrain_forward(sdfa_convtrain *h, const float *d_feat, int64_t N, float *d_C, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_feat || !d_C) return sdfa_fail(SDFA_EINVAL, "convtrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    CtArgs a = args_of(h, d_feat, N, d_ws);
    a.C = d_C;
    h->ts.fwd_N = 0;                                        // a forward that fails half way is no forward
    HIP_TRY(headtrain_fold(h->t, h->ts.d_param, f + w.W, f + w.inv, f + w.sc, st));
    HIP_TRY(convtrain_forward(a, st));
    h->ts.fwd_N = N;
    h->ts.fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_convtrain_backward(sdfa_convtrain *h, const float *d_feat, const float *d_dC, int64_t N, void *d_ws, int64_t ws_bytes,
                            void *stream) {
    const int rc = check_call(h, "backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_feat || !d_dC) return sdfa_fail(SDFA_EINVAL, "convtrain_backward: null pointer");
    const int rf = ts_check_forward(h->ts, MOD, N, d_ws, "frames");
    if (rf < 0) return rf;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    CtArgs a = args_of(h, d_feat, N, d_ws);
    a.dC = d_dC;
    h->ts.fwd_N = 0;                                        // the kept a become da: one backward per forward
    HIP_TRY(convtrain_backward(a, st));
    HIP_TRY(convtrain_products(a, st));
    HIP_TRY(convtrain_reduce(a, st));
    HIP_TRY(headtrain_wnorm_backward(h->t, h->ts.d_param, f + w.dW, f + w.inv, f + w.sc, h->ts.d_grad, st));
    return SDFA_OK;
}

int sdfa_convtrain_adam(sdfa_convtrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    return ts_adam(ts_of(h), MOD, lr, beta1, beta2, eps, stream);
}

int sdfa_convtrain_zero_grad(sdfa_convtrain *h, void *stream) { return ts_zero_grad(ts_of(h), MOD, stream); }

int sdfa_convtrain_get_tensor(sdfa_convtrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    const int ti = locate(h, "convtrain_get_tensor", name, h_dst, numel);
    if (ti < 0) return ti;
    if (!is_const(ti)) return ts_get_tensor(h->ts, MOD, what, offset_of(ti), h_dst, numel);
    if (!h->ts.finalized) return sdfa_fail(SDFA_ESTATE, "convtrain_get_tensor: the handle is not finalised");
    if (what != TS_PARAM) return sdfa_fail(SDFA_EINVAL, "convtrain_get_tensor: \"%s\" is a constant: it has no buffer %d", name, what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, h->d_const + offset_of(ti), (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return SDFA_OK;
}

int sdfa_convtrain_set_state(sdfa_convtrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    const int ti = locate(h, "convtrain_set_state", name, h_src, numel);
    if (ti < 0) return ti;
    if (is_const(ti)) return sdfa_fail(SDFA_EINVAL, "convtrain_set_state: \"%s\" is a constant: sdfa_convtrain_set_tensor gives it, before finalize", name);
    return ts_set_state(h->ts, MOD, what, offset_of(ti), h_src, numel);
}

int sdfa_convtrain_set_grad(sdfa_convtrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_convtrain_set_state(h, name, SDFA_CONVTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_convtrain_step_count(const sdfa_convtrain *h) { return ts_step_count(ts_of(h), MOD); }
int sdfa_convtrain_set_step_count(sdfa_convtrain *h, int64_t t) { return ts_set_step_count(ts_of(h), MOD, t); }

}  // extern "C"
