// Host side of the attention layer's training step (include/sdfa_attntrain.h): the layer's tensor table,
// the workspace layout and the launches of attntrain.hip over the flat training state of trainstate.h.
#include "attntrain.h"
#include "trainstate.h"

#include <string.h>

#include <string>

namespace {

const char *const MOD = "attntrain";
TS_SAME_BUFFERS(SDFA_ATTNTRAIN);
constexpr int NT = 5;
constexpr int64_t QW = (int64_t)AT_KW * AT_D;
const char *const PREFIX = "_audio_encoder._layers.10.";
const struct {
    const char *name;
    int64_t numel;
} TENSOR[NT] = {
    {"_conv_query.weight", AT_D * QW}, {"proj_qry.weight", (int64_t)AT_A * AT_D}, {"proj_key.weight", (int64_t)AT_A * AT_D},
    {"v.weight", AT_A}, {"b", AT_A},
};
enum { WC = 0, WQ = 1, WK = 2, V = 3, B = 4 };

// Workspace of a batch of N frames, offsets in floats, every buffer on a 256-byte boundary.
struct Ws {
    int64_t qc, qp, u, al, dpre, dvp, dqp, dqc, dHq, part, partv, total;
    int nblk;
};

Ws ws_layout(int64_t N) {
    Ws w;
    WsTake take;
    w.nblk = (int)((N + AT_BLOCK_FRAMES - 1) / AT_BLOCK_FRAMES);
    w.qc = take(N * AT_D);
    w.qp = take(N * AT_A);
    w.u = take(N * AT_T * AT_A);
    w.al = take(N * AT_T);
    w.dpre = take(N * AT_T * AT_A);
    w.dvp = take(N * AT_A);
    w.dqp = take(N * AT_A);
    w.dqc = take(N * AT_D);
    w.dHq = take(N * QW);
    w.part = take((int64_t)w.nblk * AT_A * AT_D);
    w.partv = take((int64_t)w.nblk * 2 * AT_A);
    w.total = take.bytes();
    return w;
}

}  // namespace

struct sdfa_attntrain {
    int64_t off[NT + 1];
    TrainState ts;                       // a slot per tensor
};

namespace {

// The slot of tensor `name`; `data` is the caller's host pointer, refused first.
int locate(const sdfa_attntrain *h, const char *who, const char *name, const void *data, int64_t numel) {
    if (!data || !h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    const size_t np = strlen(PREFIX);
    int ti = -1;
    if (strncmp(name, PREFIX, np) == 0)
        for (int i = 0; i < NT; ++i)
            if (strcmp(name + np, TENSOR[i].name) == 0) ti = i;
    if (ti < 0) return sdfa_fail(SDFA_EINVAL, "%s: the attention layer has no tensor \"%s\"", who, name);
    if (numel != TENSOR[ti].numel)
        return sdfa_fail(SDFA_EINVAL, "%s: \"%s\" has %lld elements, %lld given", who, name, (long long)TENSOR[ti].numel, (long long)numel);
    return ti;
}

int check_call(const sdfa_attntrain *h, const char *fn, int64_t N, const void *d_ws, int64_t ws_bytes) {
    const int rc = ts_ready(ts_of(h), MOD, fn);
    if (rc < 0) return rc;
    if (N < 1 || N > SDFA_ATTNTRAIN_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "attntrain_%s: %lld frames outside 1 .. %d", fn, (long long)N, SDFA_ATTNTRAIN_MAX_FRAMES);
    return ts_check_ws(MOD, fn, d_ws, ws_bytes, ws_layout(N).total);
}

AtOp op(const float *p, int64_t si, int64_t sc, int64_t ni, int nc) { return AtOp{p, si, sc, ni, nc}; }

}  // namespace

extern "C" {

int sdfa_attntrain_abi_version(void) { return SDFA_ATTNTRAIN_ABI_VERSION; }

sdfa_attntrain *sdfa_attntrain_create(void) {
    sdfa_attntrain *h = new sdfa_attntrain();
    h->off[0] = 0;
    for (int i = 0; i < NT; ++i) h->off[i + 1] = h->off[i] + TENSOR[i].numel;
    ts_init(h->ts, h->off[NT], NT);
    return h;
}

void sdfa_attntrain_destroy(sdfa_attntrain *h) {
    if (!h) return;
    ts_free(h->ts);
    delete h;
}

int sdfa_attntrain_set_tensor(sdfa_attntrain *h, const char *name, const float *h_src, int64_t numel) {
    const int ti = locate(h, "attntrain_set_tensor", name, h_src, numel);
    return ti < 0 ? ti : ts_set_tensor(h->ts, MOD, ti, h->off[ti], h_src, numel);
}

int sdfa_attntrain_finalize(sdfa_attntrain *h, void *stream) {
    const int rc = ts_check_finalize(ts_of(h), MOD, [](int ti) { return std::string(PREFIX) + TENSOR[ti].name; });
    return rc < 0 ? rc : ts_finalize(h->ts, (hipStream_t)stream);
}

int64_t sdfa_attntrain_numel(const sdfa_attntrain *h) { return ts_numel(ts_of(h), MOD); }

int64_t sdfa_attntrain_workspace_bytes(const sdfa_attntrain *h, int64_t max_frames) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "attntrain_workspace_bytes: null handle");
    if (max_frames < 1 || max_frames > SDFA_ATTNTRAIN_MAX_FRAMES)
        return sdfa_fail(SDFA_EINVAL, "attntrain_workspace_bytes: %lld frames outside 1 .. %d", (long long)max_frames, SDFA_ATTNTRAIN_MAX_FRAMES);
    return ws_layout(max_frames).total;
}

int sdfa_attntrain_forward(sdfa_attntrain *h, const float *d_H, int64_t N, float *d_z, float *d_align, void *d_ws, int64_t ws_bytes,
                           void *stream) {
    const int rc = check_call(h, "forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_H || !d_z || !d_align) return sdfa_fail(SDFA_EINVAL, "attntrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    const float *P = h->ts.d_param;
    h->ts.fwd_N = 0;                                        // a forward that fails half way is no forward
    AtProdArgs p;
    p.A = op(d_H + AT_W0 * AT_D, (int64_t)AT_T * AT_D, 1, N, (int)QW);      // the window H[n][31 .. 33][:], contiguous
    p.B = op(P + h->off[WC], QW, 1, AT_D, (int)QW);
    p.out = f + w.qc;
    p.ldo = AT_D;
    HIP_TRY(attntrain_product(AT_PROD_QC, p, st));
    p.A = op(f + w.qc, AT_D, 1, N, AT_D);
    p.B = op(P + h->off[WQ], AT_D, 1, AT_A, AT_D);
    p.out = f + w.qp;
    p.ldo = AT_A;
    HIP_TRY(attntrain_product(AT_PROD_QP, p, st));
    AtFwdArgs a;
    a.H = d_H;
    a.Wk = P + h->off[WK];
    a.v = P + h->off[V];
    a.b = P + h->off[B];
    a.qp = f + w.qp;
    a.u = f + w.u;
    a.al = f + w.al;
    a.z = d_z;
    a.align = d_align;
    a.N = N;
    HIP_TRY(attntrain_frame_forward(a, st));
    h->ts.fwd_N = N;
    h->ts.fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_attntrain_backward(sdfa_attntrain *h, const float *d_H, const float *d_dz, int64_t N, float *d_dH, void *d_ws,
                            int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_H || !d_dz) return sdfa_fail(SDFA_EINVAL, "attntrain_backward: null pointer");
    const int rf = ts_check_forward(h->ts, MOD, N, d_ws, "frames");
    if (rf < 0) return rf;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    const float *P = h->ts.d_param;
    AtFrameBwdArgs fb;
    fb.H = d_H;
    fb.dz = d_dz;
    fb.al = f + w.al;
    fb.u = f + w.u;
    fb.v = P + h->off[V];
    fb.dpre = f + w.dpre;
    fb.dvp = f + w.dvp;
    fb.dqp = f + w.dqp;
    fb.N = N;
    HIP_TRY(attntrain_frame_backward(fb, st));
    AtProdArgs p;
    p.A = op(f + w.dqp, AT_A, 1, N, AT_A);
    p.B = op(P + h->off[WQ], 1, AT_D, AT_D, AT_A);          // Wq^T
    p.out = f + w.dqc;
    p.ldo = AT_D;
    HIP_TRY(attntrain_product(AT_PROD_DQC, p, st));
    if (d_dH) {
        p.A = op(f + w.dqc, AT_D, 1, N, AT_D);
        p.B = op(P + h->off[WC], 1, QW, QW, AT_D);          // Wc^T, its rows in window order
        p.out = f + w.dHq;
        p.ldo = QW;
        HIP_TRY(attntrain_product(AT_PROD_DHQ, p, st));
    }
    AtBwdArgs b;
    b.H = d_H;
    b.dz = d_dz;
    b.al = f + w.al;
    b.dpre = f + w.dpre;
    b.dvp = f + w.dvp;
    b.dqp = f + w.dqp;
    b.dqc = f + w.dqc;
    b.qc = f + w.qc;
    b.dHq = f + w.dHq;
    b.Wk = P + h->off[WK];
    b.gWc = h->ts.d_grad + h->off[WC];
    b.gWq = h->ts.d_grad + h->off[WQ];
    b.part = f + w.part;
    b.partv = f + w.partv;
    b.dH = d_dH;
    b.N = N;
    b.nblk = w.nblk;
    HIP_TRY(attntrain_backward(b, st));
    AtReduceArgs r;
    r.part = f + w.part;
    r.partv = f + w.partv;
    r.gWk = h->ts.d_grad + h->off[WK];
    r.gv = h->ts.d_grad + h->off[V];
    r.gb = h->ts.d_grad + h->off[B];
    r.nblk = w.nblk;
    HIP_TRY(attntrain_reduce(r, st));
    return SDFA_OK;
}

int sdfa_attntrain_adam(sdfa_attntrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    return ts_adam(ts_of(h), MOD, lr, beta1, beta2, eps, stream);
}

int sdfa_attntrain_zero_grad(sdfa_attntrain *h, void *stream) { return ts_zero_grad(ts_of(h), MOD, stream); }

int sdfa_attntrain_get_tensor(sdfa_attntrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    const int ti = locate(h, "attntrain_get_tensor", name, h_dst, numel);
    return ti < 0 ? ti : ts_get_tensor(h->ts, MOD, what, h->off[ti], h_dst, numel);
}

int sdfa_attntrain_set_state(sdfa_attntrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    const int ti = locate(h, "attntrain_set_state", name, h_src, numel);
    return ti < 0 ? ti : ts_set_state(h->ts, MOD, what, h->off[ti], h_src, numel);
}

int sdfa_attntrain_set_grad(sdfa_attntrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_attntrain_set_state(h, name, SDFA_ATTNTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_attntrain_step_count(const sdfa_attntrain *h) { return ts_step_count(ts_of(h), MOD); }
int sdfa_attntrain_set_step_count(sdfa_attntrain *h, int64_t t) { return ts_set_step_count(ts_of(h), MOD, t); }

}  // extern "C"
