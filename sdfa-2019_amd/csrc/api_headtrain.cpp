// Host side of the regressor head's training step (include/sdfa_headtrain.h): the handle and its flat
// device buffers, the refusals, the workspace layout and the launches of headtrain.hip.
#include "host.h"
#include "headtrain.h"

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

namespace {

struct Spec {
    const char *name;
    int P, K, Kin, cond, act;
};

// speech_anime/config/model/dgrad.py: the trunk, then the scale branch, then the rotat branch
const Spec DGRAD[7] = {
    {"_output_module._layers.0", 512, 520, 512, 1, HT_ACT_LRELU},
    {"_output_module._scale_layers.0", 512, 520, 512, 1, HT_ACT_LRELU},
    {"_output_module._scale_layers.1", 256, 512, 512, 0, HT_ACT_TANH},
    {"_output_module._scale_layers.2", 85, 256, 256, 0, HT_ACT_LINEAR},
    {"_output_module._rotat_layers.0", 512, 520, 512, 1, HT_ACT_LRELU},
    {"_output_module._rotat_layers.1", 256, 512, 512, 0, HT_ACT_TANH},
    {"_output_module._rotat_layers.2", 180, 256, 256, 0, HT_ACT_LINEAR},
};
// speech_anime/config/model/offsets.py
const Spec OFFSETS[3] = {
    {"_output_module._layers.0", 512, 520, 512, 1, HT_ACT_LRELU},
    {"_output_module._layers.1", 256, 512, 512, 0, HT_ACT_TANH},
    {"_output_module._layers.2", 59, 256, 256, 0, HT_ACT_LINEAR},
};

// Workspace of a batch of N rows, offsets in floats, every buffer on a 256-byte boundary.
struct Ws {
    int64_t z, sid, h0, h1[2], h2[2], d2[2], d1[2], d0, total;
};

}  // namespace

struct sdfa_headtrain {
    int head, nb, kc;
    const Spec *spec;
    HtTable t;
    int64_t numel, wnumel;               // floats of a parameter-shaped buffer; of W
    std::vector<float> host;             // the parameters until finalize
    std::vector<char> have;              // [layer][g, v, bias]
    bool finalized;
    float *d_param, *d_grad, *d_m, *d_v, *d_W, *d_dW, *d_inv, *d_sc;
    int64_t step;
    int64_t fwd_N;                       // rows of the last forward, 0 when there is none
    const void *fwd_ws;
};

namespace {

Ws ws_layout(const sdfa_headtrain *h, int64_t N) {
    Ws w;
    int64_t off = 0;
    auto take = [&](int64_t floats) {
        const int64_t at = off;
        off += round_up(floats, 64);
        return at;
    };
    w.z = take(N * SDFA_HEADTRAIN_Z);
    w.sid = take(N);
    w.h0 = w.d0 = 0;
    if (h->head == SDFA_HEADTRAIN_HEAD_DGRAD) {
        w.h0 = take(N * 512);
        w.d0 = take(N * 512);
    }
    for (int b = 0; b < 2; ++b) {
        const bool on = b < h->nb;
        w.h1[b] = on ? take(N * 512) : 0;
        w.h2[b] = on ? take(N * 256) : 0;
        w.d2[b] = on ? take(N * 256) : 0;
        w.d1[b] = on ? take(N * 512) : 0;
    }
    w.total = off * 4;
    return w;
}

// name -> (layer, part 0 g | 1 v | 2 bias); -1 when the head has no such tensor
int find_tensor(const sdfa_headtrain *h, const char *name, int *part) {
    static const char *const SUF[3] = {".weight_g", ".weight_v", ".bias"};
    for (int li = 0; li < h->t.nl; ++li) {
        const size_t n = strlen(h->spec[li].name);
        if (strncmp(name, h->spec[li].name, n) != 0) continue;
        for (int s = 0; s < 3; ++s)
            if (strcmp(name + n, SUF[s]) == 0) {
                *part = s;
                return li;
            }
    }
    return -1;
}

int64_t part_offset(const HtLayer &L, int part) { return part == 0 ? L.og : part == 1 ? L.ov : L.ob; }
int64_t part_numel(const HtLayer &L, int part) { return part == 1 ? (int64_t)L.P * L.K : L.P; }

int locate(const sdfa_headtrain *h, const char *who, const char *name, int64_t numel, int64_t *off) {
    if (!h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    int part = 0;
    const int li = find_tensor(h, name, &part);
    if (li < 0) return sdfa_fail(SDFA_EINVAL, "%s: the head has no tensor \"%s\"", who, name);
    const HtLayer &L = h->t.l[li];
    if (numel != part_numel(L, part)) return sdfa_fail(SDFA_EINVAL, "%s: \"%s\" has %lld elements, %lld given", who, name, (long long)part_numel(L, part), (long long)numel);
    *off = part_offset(L, part);
    return li * 3 + part;
}

float *buffer_of(sdfa_headtrain *h, int what) {
    return what == SDFA_HEADTRAIN_PARAM ? h->d_param : what == SDFA_HEADTRAIN_GRAD ? h->d_grad : what == SDFA_HEADTRAIN_EXP_AVG ? h->d_m
         : what == SDFA_HEADTRAIN_EXP_AVG_SQ ? h->d_v : nullptr;
}

int check_call(const sdfa_headtrain *h, const char *who, int64_t N, const void *d_ws, int64_t ws_bytes) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "%s: null handle", who);
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "%s: the handle is not finalised", who);
    if (N < 2 || N % 2 != 0) return sdfa_fail(SDFA_EINVAL, "%s: a batch of %lld rows is not [a; b] with at least one pair", who, (long long)N);
    if (N > SDFA_HEADTRAIN_MAX_ROWS) return sdfa_fail(SDFA_EINVAL, "%s: %lld rows, at most %d", who, (long long)N, SDFA_HEADTRAIN_MAX_ROWS);
    if (!d_ws) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    const int64_t need = ws_layout(h, N).total;
    if (ws_bytes < need) return sdfa_fail(SDFA_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)need);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "%s: workspace not 256-byte aligned", who);
    return SDFA_OK;
}

HtFwdJob fwd_job(const sdfa_headtrain *h, int li, const float *X, int ldx, float *Y, int ldy) {
    const HtLayer &L = h->t.l[li];
    HtFwdJob j;
    j.X = X;
    j.W = h->d_W + L.ow;
    j.bias = h->d_param + L.ob;
    j.Y = Y;
    j.ldx = ldx;
    j.ldw = L.K;
    j.ldy = ldy;
    j.P = L.P;
    j.Kin = L.Kin;
    j.cond = L.cond;
    j.act = L.act;
    return j;
}

HtBwdJob bwd_job(const sdfa_headtrain *h, int li, const float *D, int ldd, const float *X, const float *Yprev, float *Dprev) {
    const HtLayer &L = h->t.l[li];
    HtBwdJob j;
    j.D = D;
    j.X = X;
    j.W = h->d_W + L.ow;
    j.dW = h->d_dW + L.ow;
    j.db = h->d_grad + L.ob;
    j.Yprev = Yprev;
    j.Dprev = Dprev;
    j.ldd = ldd;
    j.ldx = L.Kin;
    j.ldp = L.Kin;
    j.P = L.P;
    j.K = L.K;
    j.Kin = L.Kin;
    j.cond = L.cond;
    j.tp = (L.P + SDFA_HEADTRAIN_TILE - 1) / SDFA_HEADTRAIN_TILE;
    j.tk = (L.K + 1 + SDFA_HEADTRAIN_TILE - 1) / SDFA_HEADTRAIN_TILE;
    j.ndw = j.tp * j.tk;
    return j;
}

}  // namespace

extern "C" {

int sdfa_headtrain_abi_version(void) { return SDFA_HEADTRAIN_ABI_VERSION; }

sdfa_headtrain *sdfa_headtrain_create(int head) {
    if (head != SDFA_HEADTRAIN_HEAD_DGRAD && head != SDFA_HEADTRAIN_HEAD_OFFSETS) {
        sdfa_fail(SDFA_EINVAL, "headtrain_create: unknown head %d", head);
        return nullptr;
    }
    sdfa_headtrain *h = new sdfa_headtrain();
    const bool dg = head == SDFA_HEADTRAIN_HEAD_DGRAD;
    h->head = head;
    h->nb = dg ? 2 : 1;
    h->spec = dg ? DGRAD : OFFSETS;
    h->t.nl = dg ? 7 : 3;
    h->kc = dg ? 265 : 59;
    int64_t off = 0, woff = 0;
    int row = 0;
    for (int li = 0; li < h->t.nl; ++li) {
        const Spec &s = h->spec[li];
        HtLayer &L = h->t.l[li];
        L.P = s.P;
        L.K = s.K;
        L.Kin = s.Kin;
        L.cond = s.cond;
        L.act = s.act;
        L.row0 = row;
        L.og = off;
        L.ov = off + s.P;
        L.ob = L.ov + (int64_t)s.P * s.K;
        off = L.ob + s.P;
        L.ow = woff;
        woff += (int64_t)s.P * s.K;
        row += s.P;
    }
    h->t.rows = row;
    h->numel = off;
    h->wnumel = woff;
    h->host.assign((size_t)off, 0.f);
    h->have.assign((size_t)h->t.nl * 3, 0);
    h->finalized = false;
    h->d_param = h->d_grad = h->d_m = h->d_v = h->d_W = h->d_dW = h->d_inv = h->d_sc = nullptr;
    h->step = 0;
    h->fwd_N = 0;
    h->fwd_ws = nullptr;
    return h;
}

void sdfa_headtrain_destroy(sdfa_headtrain *h) {
    if (!h) return;
    for (float *p : {h->d_param, h->d_grad, h->d_m, h->d_v, h->d_W, h->d_dW, h->d_inv, h->d_sc})
        if (p) (void)hipFree(p);
    delete h;
}

int sdfa_headtrain_set_tensor(sdfa_headtrain *h, const char *name, const float *h_src, int64_t numel) {
    if (!h_src) return sdfa_fail(SDFA_EINVAL, "headtrain_set_tensor: null pointer");
    int64_t off = 0;
    const int slot = locate(h, "headtrain_set_tensor", name, numel, &off);
    if (slot < 0) return slot;
    if (h->finalized) return sdfa_fail(SDFA_ESTATE, "headtrain_set_tensor: the handle is finalised (sdfa_headtrain_set_state writes a parameter then)");
    memcpy(h->host.data() + off, h_src, (size_t)numel * sizeof(float));
    h->have[slot] = 1;
    return SDFA_OK;
}

int sdfa_headtrain_finalize(sdfa_headtrain *h, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "headtrain_finalize: null handle");
    if (h->finalized) return sdfa_fail(SDFA_ESTATE, "headtrain_finalize: already finalised");
    static const char *const SUF[3] = {".weight_g", ".weight_v", ".bias"};
    for (size_t s = 0; s < h->have.size(); ++s)
        if (!h->have[s]) return sdfa_fail(SDFA_ESTATE, "headtrain_finalize: tensor \"%s%s\" is missing", h->spec[s / 3].name, SUF[s % 3]);
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)h->numel * sizeof(float), wb = (size_t)h->wnumel * sizeof(float), rb = (size_t)h->t.rows * sizeof(float);
    HIP_TRY(hipMalloc((void **)&h->d_param, nb));
    HIP_TRY(hipMalloc((void **)&h->d_grad, nb));
    HIP_TRY(hipMalloc((void **)&h->d_m, nb));
    HIP_TRY(hipMalloc((void **)&h->d_v, nb));
    HIP_TRY(hipMalloc((void **)&h->d_W, wb));
    HIP_TRY(hipMalloc((void **)&h->d_dW, wb));
    HIP_TRY(hipMalloc((void **)&h->d_inv, rb));
    HIP_TRY(hipMalloc((void **)&h->d_sc, rb));
    HIP_TRY(hipMemcpyAsync(h->d_param, h->host.data(), nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->d_grad, 0, nb, st));
    HIP_TRY(hipMemsetAsync(h->d_m, 0, nb, st));
    HIP_TRY(hipMemsetAsync(h->d_v, 0, nb, st));
    HIP_TRY(hipMemsetAsync(h->d_dW, 0, wb, st));
    HIP_TRY(hipStreamSynchronize(st));             // the host copy is released below
    std::vector<float>().swap(h->host);
    h->finalized = true;
    return SDFA_OK;
}

int sdfa_headtrain_coef_dim(const sdfa_headtrain *h) { return h ? h->kc : sdfa_fail(SDFA_EINVAL, "headtrain_coef_dim: null handle"); }
int64_t sdfa_headtrain_numel(const sdfa_headtrain *h) { return h ? h->numel : sdfa_fail(SDFA_EINVAL, "headtrain_numel: null handle"); }

int64_t sdfa_headtrain_workspace_bytes(const sdfa_headtrain *h, int64_t max_rows) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "headtrain_workspace_bytes: null handle");
    if (max_rows < 2 || max_rows > SDFA_HEADTRAIN_MAX_ROWS) return sdfa_fail(SDFA_EINVAL, "headtrain_workspace_bytes: %lld rows outside 2 .. %d", (long long)max_rows, SDFA_HEADTRAIN_MAX_ROWS);
    return ws_layout(h, max_rows).total;
}

int sdfa_headtrain_forward(sdfa_headtrain *h, const float *d_z, const int64_t *d_speaker_id, int64_t N, float *d_coef,
                           void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "headtrain_forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_z || !d_speaker_id || !d_coef) return sdfa_fail(SDFA_EINVAL, "headtrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(h, N);
    float *f = (float *)d_ws;
    h->fwd_N = 0;                                           // a forward that fails half way is no forward
    HIP_TRY(headtrain_fold(h->t, h->d_param, h->d_W, h->d_inv, h->d_sc, st));
    HtFwdArgs a;
    a.N = N;
    a.sid = d_speaker_id;
    a.zcopy = f + w.z;
    a.sidcopy = (int *)(f + w.sid);
    a.nb = 1;
    int l1 = 0;                                             // first layer of branch 0
    const float *x1 = d_z;
    if (h->head == SDFA_HEADTRAIN_HEAD_DGRAD) {
        a.b[0] = a.b[1] = fwd_job(h, 0, d_z, SDFA_HEADTRAIN_Z, f + w.h0, 512);
        HIP_TRY(headtrain_forward_layer(a, st));
        a.zcopy = nullptr;
        a.sidcopy = nullptr;
        l1 = 1;
        x1 = f + w.h0;
    }
    a.nb = h->nb;
    int coff = 0;
    for (int depth = 0; depth < 3; ++depth) {
        coff = 0;
        for (int b = 0; b < h->nb; ++b) {
            const int li = l1 + 3 * b + depth;
            if (depth == 0) a.b[b] = fwd_job(h, li, x1, 512, f + w.h1[b], 512);
            else if (depth == 1) a.b[b] = fwd_job(h, li, f + w.h1[b], 512, f + w.h2[b], 256);
            else a.b[b] = fwd_job(h, li, f + w.h2[b], 256, d_coef + coff, h->kc);
            coff += h->t.l[li].P;
        }
        if (h->nb == 1) a.b[1] = a.b[0];
        HIP_TRY(headtrain_forward_layer(a, st));
        a.zcopy = nullptr;
        a.sidcopy = nullptr;
    }
    h->fwd_N = N;
    h->fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_headtrain_backward(sdfa_headtrain *h, const float *d_dcoef, int64_t N, float *d_dz, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "headtrain_backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_dcoef) return sdfa_fail(SDFA_EINVAL, "headtrain_backward: null pointer");
    if (h->fwd_N != N || h->fwd_ws != d_ws)
        return sdfa_fail(SDFA_EINVAL, "headtrain_backward: no forward of %lld rows on this workspace precedes it", (long long)N);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(h, N);
    float *f = (float *)d_ws;
    const bool dg = h->head == SDFA_HEADTRAIN_HEAD_DGRAD;
    const int l1 = dg ? 1 : 0;
    const float *x1 = dg ? f + w.h0 : f + w.z;
    HtBwdArgs a;
    a.N = N;
    a.sid = (const int *)(f + w.sid);
    a.nb = h->nb;
    a.rowtiles = (int)((N + SDFA_HEADTRAIN_TILE - 1) / SDFA_HEADTRAIN_TILE);
    for (int depth = 2; depth >= 0; --depth) {
        int coff = 0;
        for (int b = 0; b < h->nb; ++b) {
            const int li = l1 + 3 * b + depth;
            if (depth == 2) a.b[b] = bwd_job(h, li, d_dcoef + coff, h->kc, f + w.h2[b], f + w.h2[b], f + w.d2[b]);
            else if (depth == 1) a.b[b] = bwd_job(h, li, f + w.d2[b], 256, f + w.h1[b], f + w.h1[b], f + w.d1[b]);
            else a.b[b] = bwd_job(h, li, f + w.d1[b], 512, x1, dg ? f + w.h0 : nullptr, dg ? f + w.d0 : d_dz);
            coff += h->t.l[li].P;
        }
        if (h->nb == 1) a.b[1] = a.b[0];
        a.tkx = a.b[0].Kin / SDFA_HEADTRAIN_TILE;
        if (depth == 2) {
            a.dx_mode = HT_DX_BRANCH;
            a.act_prev = HT_ACT_TANH;
        } else if (depth == 1) {
            a.dx_mode = HT_DX_BRANCH;
            a.act_prev = HT_ACT_LRELU;
        } else if (dg) {
            a.dx_mode = HT_DX_MERGE;
            a.act_prev = HT_ACT_LRELU;
        } else {
            a.dx_mode = d_dz ? HT_DX_PLAIN : HT_DX_NONE;
            a.act_prev = HT_ACT_LINEAR;
        }
        HIP_TRY(headtrain_backward_layer(a, st));
    }
    if (dg) {
        a.nb = 1;
        a.b[0] = a.b[1] = bwd_job(h, 0, f + w.d0, 512, f + w.z, nullptr, d_dz);
        a.tkx = a.b[0].Kin / SDFA_HEADTRAIN_TILE;
        a.dx_mode = d_dz ? HT_DX_PLAIN : HT_DX_NONE;
        a.act_prev = HT_ACT_LINEAR;
        HIP_TRY(headtrain_backward_layer(a, st));
    }
    HIP_TRY(headtrain_wnorm_backward(h->t, h->d_param, h->d_dW, h->d_inv, h->d_sc, h->d_grad, st));
    return SDFA_OK;
}

int sdfa_headtrain_adam(sdfa_headtrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "headtrain_adam: null handle");
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "headtrain_adam: the handle is not finalised");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return sdfa_fail(SDFA_EINVAL, "headtrain_adam: lr %g, betas (%g, %g), eps %g: torch.optim.Adam refuses these", lr, beta1, beta2, eps);
    const int64_t t = h->step + 1;
    HIP_TRY(headtrain_adam_step(h->d_param, h->d_grad, h->d_m, h->d_v, h->numel, t, lr, beta1, beta2, eps, (hipStream_t)stream));
    h->step = t;
    h->fwd_N = 0;                                           // the kept activations belong to the old parameters
    return SDFA_OK;
}

int sdfa_headtrain_zero_grad(sdfa_headtrain *h, void *stream) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "headtrain_zero_grad: null handle");
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "headtrain_zero_grad: the handle is not finalised");
    HIP_TRY(hipMemsetAsync(h->d_grad, 0, (size_t)h->numel * sizeof(float), (hipStream_t)stream));
    return SDFA_OK;
}

int sdfa_headtrain_get_tensor(sdfa_headtrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    if (!h_dst) return sdfa_fail(SDFA_EINVAL, "headtrain_get_tensor: null pointer");
    int64_t off = 0;
    const int slot = locate(h, "headtrain_get_tensor", name, numel, &off);
    if (slot < 0) return slot;
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "headtrain_get_tensor: the handle is not finalised");
    const float *src = buffer_of(h, what);
    if (!src) return sdfa_fail(SDFA_EINVAL, "headtrain_get_tensor: unknown buffer %d", what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, src + off, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return SDFA_OK;
}

int sdfa_headtrain_set_state(sdfa_headtrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    if (!h_src) return sdfa_fail(SDFA_EINVAL, "headtrain_set_state: null pointer");
    int64_t off = 0;
    const int slot = locate(h, "headtrain_set_state", name, numel, &off);
    if (slot < 0) return slot;
    if (!h->finalized) return sdfa_fail(SDFA_ESTATE, "headtrain_set_state: the handle is not finalised");
    float *dst = buffer_of(h, what);
    if (!dst) return sdfa_fail(SDFA_EINVAL, "headtrain_set_state: unknown buffer %d", what);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst + off, h_src, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
    if (what == SDFA_HEADTRAIN_PARAM) h->fwd_N = 0;
    return SDFA_OK;
}

int sdfa_headtrain_set_grad(sdfa_headtrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_headtrain_set_state(h, name, SDFA_HEADTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_headtrain_step_count(const sdfa_headtrain *h) { return h ? h->step : sdfa_fail(SDFA_EINVAL, "headtrain_step_count: null handle"); }

int sdfa_headtrain_set_step_count(sdfa_headtrain *h, int64_t t) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "headtrain_set_step_count: null handle");
    if (t < 0) return sdfa_fail(SDFA_EINVAL, "headtrain_set_step_count: %lld is negative", (long long)t);
    h->step = t;
    return SDFA_OK;
}

}  // extern "C"
