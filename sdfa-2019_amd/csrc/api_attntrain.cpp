// Host side of the attention layer's training step (include/sdfa_attntrain.h): the handle and its flat
// device buffers, the refusals, the workspace layout and the launches of attntrain.hip.  Adam is headtrain.hip's kernel.
#include "host.h"
#include "attntrain.h"
#include "headtrain.h"

#include <string.h>

#include <vector>

namespace {

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
    int64_t off = 0;
    auto take = [&](int64_t floats) {
        const int64_t at = off;
        off += round_up(floats, 64);
        return at;
    };
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
    w.total = off * 4;
    return w;
}

}  // namespace

struct sdfa_attntrain {
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

int locate(const sdfa_attntrain *h, const char *who, const char *name, int64_t numel) {
    if (!h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
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

float *buffer_of(sdfa_attntrain *h, int what) {
    return what == SDFA_ATTNTRAIN_PARAM ? h->d_param : what == SDFA_ATTNTRAIN_GRAD ? h->d_grad : what == SDFA_ATTNTRAIN_EXP_AVG ? h->d_m
         : what == SDFA_ATTNTRAIN_EXP_AVG_SQ ? h->d_v : nullptr;
}

int check_call(const sdfa_attntrain *h, const char *who, int64_t N, const void *d_ws, int64_t ws_bytes) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "%s: null handle", who);
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "%s: the handle is not finalised", who);
    if (N < 1 || N > SDFA_ATTNTRAIN_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "%s: %lld frames outside 1 .. %d", who, (long long)N, SDFA_ATTNTRAIN_MAX_FRAMES);
    if (!d_ws) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    const int64_t need = ws_layout(N).total;
    if (ws_bytes < need) return sdfa_fail(SDFA_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)need);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "%s: workspace not 256-byte aligned", who);
    return SDFA_OK;
}

AtOp op(const float *p, int64_t si, int64_t sc, int64_t ni, int nc) { return AtOp{p, si, sc, ni, nc}; }

}  // namespace

extern "C" {

int sdfa_attntrain_abi_version(void) { return SDFA_ATTNTRAIN_ABI_VERSION; }

sdfa_attntrain *sdfa_attntrain_create(void) {
    sdfa_attntrain *h = new sdfa_attntrain();
    h->off[0] = 0;
    for (int i = 0; i < NT; ++i) {
        h->off[i + 1] = h->off[i] + TENSOR[i].numel;
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

void sdfa_attntrain_destroy(sdfa_attntrain *h) {
    if (!h) return;
    for (float *p : {h->d_param, h->d_grad, h->d_m, h->d_v})
        if (p) (void)hipFree(p);
    delete h;
}

int sdfa_attntrain_set_tensor(sdfa_attntrain *h, const char *name, const float *h_src, int64_t numel) {
    if (!h_src) return sdfa_fail(SDFA_EINVAL, "attntrain_set_tensor: null pointer");
    const int ti = locate(h, "attntrain_set_tensor", name, numel);
    if (ti < 0) return ti;
    if (h->finalized) return sdfa_fail(SDFA_ESTATE, "attntrain_set_tensor: the handle is finalised (sdfa_attntrain_set_state writes a parameter then)");
    memcpy(h->host.data() + h->off[ti], h_src, (size_t)numel * sizeof(float));
    h->have[ti] = 1;
    return SDFA_OK;
}

int sdfa_attntrain_finalize(sdfa_attntrain *h, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "attntrain_finalize: null handle");
    if (h->finalized) return sdfa_fail(SDFA_ESTATE, "attntrain_finalize: already finalised");
    for (int i = 0; i < NT; ++i)
        if (!h->have[i]) return sdfa_fail(SDFA_ESTATE, "attntrain_finalize: tensor \"%s%s\" is missing", PREFIX, TENSOR[i].name);
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

int64_t sdfa_attntrain_numel(const sdfa_attntrain *h) { return h ? h->off[NT] : sdfa_fail(SDFA_EINVAL, "attntrain_numel: null handle"); }

int64_t sdfa_attntrain_workspace_bytes(const sdfa_attntrain *h, int64_t max_frames) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "attntrain_workspace_bytes: null handle");
    if (max_frames < 1 || max_frames > SDFA_ATTNTRAIN_MAX_FRAMES)
        return sdfa_fail(SDFA_EINVAL, "attntrain_workspace_bytes: %lld frames outside 1 .. %d", (long long)max_frames, SDFA_ATTNTRAIN_MAX_FRAMES);
    return ws_layout(max_frames).total;
}

int sdfa_attntrain_forward(sdfa_attntrain *h, const float *d_H, int64_t N, float *d_z, float *d_align, void *d_ws, int64_t ws_bytes,
                           void *stream) {
    const int rc = check_call(h, "attntrain_forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_H || !d_z || !d_align) return sdfa_fail(SDFA_EINVAL, "attntrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    const float *P = h->d_param;
    h->fwd_N = 0;                                           // a forward that fails half way is no forward
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
    h->fwd_N = N;
    h->fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_attntrain_backward(sdfa_attntrain *h, const float *d_H, const float *d_dz, int64_t N, float *d_dH, void *d_ws,
                            int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "attntrain_backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_H || !d_dz) return sdfa_fail(SDFA_EINVAL, "attntrain_backward: null pointer");
    if (h->fwd_N != N || h->fwd_ws != d_ws)
        return sdfa_fail(SDFA_EINVAL, "attntrain_backward: no forward of %lld frames on this workspace precedes it", (long long)N);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(N);
    float *f = (float *)d_ws;
    const float *P = h->d_param;
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
    b.gWc = h->d_grad + h->off[WC];
    b.gWq = h->d_grad + h->off[WQ];
    b.part = f + w.part;
    b.partv = f + w.partv;
    b.dH = d_dH;
    b.N = N;
    b.nblk = w.nblk;
    HIP_TRY(attntrain_backward(b, st));
    AtReduceArgs r;
    r.part = f + w.part;
    r.partv = f + w.partv;
    r.gWk = h->d_grad + h->off[WK];
    r.gv = h->d_grad + h->off[V];
    r.gb = h->d_grad + h->off[B];
    r.nblk = w.nblk;
    HIP_TRY(attntrain_reduce(r, st));
    return SDFA_OK;
}

int sdfa_attntrain_adam(sdfa_attntrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "attntrain_adam: null handle");
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "attntrain_adam: the handle is not finalised");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return sdfa_fail(SDFA_EINVAL, "attntrain_adam: lr %g, betas (%g, %g), eps %g: torch.optim.Adam refuses these", lr, beta1, beta2, eps);
    const int64_t t = h->step + 1;
    HIP_TRY(headtrain_adam_step(h->d_param, h->d_grad, h->d_m, h->d_v, h->off[NT], t, lr, beta1, beta2, eps, (hipStream_t)stream));
    h->step = t;
    h->fwd_N = 0;                                           // the kept activations belong to the old parameters
    return SDFA_OK;
}

int sdfa_attntrain_zero_grad(sdfa_attntrain *h, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "attntrain_zero_grad: null handle");
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "attntrain_zero_grad: the handle is not finalised");
    HIP_TRY(hipMemsetAsync(h->d_grad, 0, (size_t)h->off[NT] * sizeof(float), (hipStream_t)stream));
    return SDFA_OK;
}

int sdfa_attntrain_get_tensor(sdfa_attntrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    if (!h_dst) return sdfa_fail(SDFA_EINVAL, "attntrain_get_tensor: null pointer");
    const int ti = locate(h, "attntrain_get_tensor", name, numel);
    if (ti < 0) return ti;
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "attntrain_get_tensor: the handle is not finalised");
    const float *src = buffer_of(h, what);
    if (!src) return sdfa_fail(SDFA_EINVAL, "attntrain_get_tensor: unknown buffer %d", what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, src + h->off[ti], (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return SDFA_OK;
}

int sdfa_attntrain_set_state(sdfa_attntrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    if (!h_src) return sdfa_fail(SDFA_EINVAL, "attntrain_set_state: null pointer");
    const int ti = locate(h, "attntrain_set_state", name, numel);
    if (ti < 0) return ti;
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "attntrain_set_state: the handle is not finalised");
    float *dst = buffer_of(h, what);
    if (!dst) return sdfa_fail(SDFA_EINVAL, "attntrain_set_state: unknown buffer %d", what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst + h->off[ti], h_src, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
    if (what == SDFA_ATTNTRAIN_PARAM) h->fwd_N = 0;
    return SDFA_OK;
}

int sdfa_attntrain_set_grad(sdfa_attntrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_attntrain_set_state(h, name, SDFA_ATTNTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_attntrain_step_count(const sdfa_attntrain *h) { return h ? h->step : sdfa_fail(SDFA_EINVAL, "attntrain_step_count: null handle"); }

int sdfa_attntrain_set_step_count(sdfa_attntrain *h, int64_t t) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "attntrain_set_step_count: null handle");
    if (t < 0) return sdfa_fail(SDFA_EINVAL, "attntrain_set_step_count: %lld is negative", (long long)t);
    h->step = t;
    return SDFA_OK;
}

}  // extern "C"
