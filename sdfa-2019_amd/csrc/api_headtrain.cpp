// Host side of the regressor head's training step (include/sdfa_headtrain.h): the head's tensor table, its
// effective-weight buffers, the workspace layout and the launches of headtrain.hip over the flat training state of trainstate.h.
#include "headtrain.h"

#include <string.h>

#include <string>

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
    int64_t z, sid, h0, h1[2], h2[2], d2[2], d1[2], d0, partW, partb, total;
    int nblk;                            // row blocks of the dW | db contraction; their partials exist for more than one
};

const char *const MOD = "headtrain";
const char *const SUF[3] = {".weight_g", ".weight_v", ".bias"};
TS_SAME_BUFFERS(SDFA_HEADTRAIN);

}  // namespace

struct sdfa_headtrain {
    int head, nb, kc;
    const Spec *spec;
    HtTable t;
    int64_t wnumel;                      // floats of W
    TrainState ts;                       // slots [layer][g, v, bias]
    float *d_W, *d_dW, *d_inv, *d_sc;
};

namespace {

Ws ws_layout(const sdfa_headtrain *h, int64_t N) {
    Ws w;
    WsTake take;
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
    w.nblk = (int)((N + HT_BLOCK_ROWS - 1) / HT_BLOCK_ROWS);
    w.partW = w.nblk > 1 ? take(w.nblk * h->wnumel) : 0;
    w.partb = w.nblk > 1 ? take((int64_t)w.nblk * h->t.rows) : 0;
    w.total = take.bytes();
    return w;
}

// name -> (layer, part 0 g | 1 v | 2 bias); -1 when the head has no such tensor
int find_tensor(const sdfa_headtrain *h, const char *name, int *part) {
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

// The slot of tensor `name` and its offset in a parameter-shaped buffer; `data` is the caller's host pointer, refused first.
int locate(const sdfa_headtrain *h, const char *who, const char *name, const void *data, int64_t numel, int64_t *off) {
    if (!data || !h || !name) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    int part = 0;
    const int li = find_tensor(h, name, &part);
    if (li < 0) return sdfa_fail(SDFA_EINVAL, "%s: the head has no tensor \"%s\"", who, name);
    const HtLayer &L = h->t.l[li];
    if (numel != part_numel(L, part)) return sdfa_fail(SDFA_EINVAL, "%s: \"%s\" has %lld elements, %lld given", who, name, (long long)part_numel(L, part), (long long)numel);
    *off = part_offset(L, part);
    return li * 3 + part;
}

int check_call(const sdfa_headtrain *h, const char *fn, int64_t N, const void *d_ws, int64_t ws_bytes) {
    const int rc = ts_ready(ts_of(h), MOD, fn);
    if (rc < 0) return rc;
    if (N < 2 || N % 2 != 0) return sdfa_fail(SDFA_EINVAL, "headtrain_%s: a batch of %lld rows is not [a; b] with at least one pair", fn, (long long)N);
    if (N > SDFA_HEADTRAIN_MAX_ROWS) return sdfa_fail(SDFA_EINVAL, "headtrain_%s: %lld rows, at most %d", fn, (long long)N, SDFA_HEADTRAIN_MAX_ROWS);
    return ts_check_ws(MOD, fn, d_ws, ws_bytes, ws_layout(h, N).total);
}

HtFwdJob fwd_job(const sdfa_headtrain *h, int li, const float *X, int ldx, float *Y, int ldy) {
    const HtLayer &L = h->t.l[li];
    HtFwdJob j;
    j.X = X;
    j.W = h->d_W + L.ow;
    j.bias = h->ts.d_param + L.ob;
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

HtBwdJob bwd_job(const sdfa_headtrain *h, const Ws &w, float *f, int li, const float *D, int ldd, const float *X, const float *Yprev, float *Dprev) {
    const HtLayer &L = h->t.l[li];
    HtBwdJob j;
    j.D = D;
    j.X = X;
    j.W = h->d_W + L.ow;
    j.dW = h->d_dW + L.ow;
    j.db = h->ts.d_grad + L.ob;
    j.pW = f + w.partW + L.ow;
    j.pb = f + w.partb + L.row0;
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
    h->wnumel = woff;
    ts_init(h->ts, off, (size_t)h->t.nl * 3);
    h->d_W = h->d_dW = h->d_inv = h->d_sc = nullptr;
    return h;
}

void sdfa_headtrain_destroy(sdfa_headtrain *h) {
    if (!h) return;
    ts_free(h->ts);
    for (float *p : {h->d_W, h->d_dW, h->d_inv, h->d_sc})
        if (p) (void)hipFree(p);
    delete h;
}

int sdfa_headtrain_set_tensor(sdfa_headtrain *h, const char *name, const float *h_src, int64_t numel) {
    int64_t off = 0;
    const int slot = locate(h, "headtrain_set_tensor", name, h_src, numel, &off);
    return slot < 0 ? slot : ts_set_tensor(h->ts, MOD, slot, off, h_src, numel);
}

int sdfa_headtrain_finalize(sdfa_headtrain *h, void *stream) {
    const int rc = ts_check_finalize(ts_of(h), MOD, [&](int slot) { return std::string(h->spec[slot / 3].name) + SUF[slot % 3]; });
    if (rc < 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t wb = (size_t)h->wnumel * sizeof(float), rb = (size_t)h->t.rows * sizeof(float);
    HIP_TRY(hipMalloc((void **)&h->d_W, wb));
    HIP_TRY(hipMalloc((void **)&h->d_dW, wb));
    HIP_TRY(hipMalloc((void **)&h->d_inv, rb));
    HIP_TRY(hipMalloc((void **)&h->d_sc, rb));
    HIP_TRY(hipMemsetAsync(h->d_dW, 0, wb, st));
    return ts_finalize(h->ts, st);
}

int sdfa_headtrain_coef_dim(const sdfa_headtrain *h) { return h ? h->kc : sdfa_fail(SDFA_EINVAL, "headtrain_coef_dim: null handle"); }
int64_t sdfa_headtrain_numel(const sdfa_headtrain *h) { return ts_numel(ts_of(h), MOD); }

int64_t sdfa_headtrain_workspace_bytes(const sdfa_headtrain *h, int64_t max_rows) {
    if (!h) return sdfa_fail(SDFA_EINVAL, "headtrain_workspace_bytes: null handle");
    if (max_rows < 2 || max_rows > SDFA_HEADTRAIN_MAX_ROWS) return sdfa_fail(SDFA_EINVAL, "headtrain_workspace_bytes: %lld rows outside 2 .. %d", (long long)max_rows, SDFA_HEADTRAIN_MAX_ROWS);
    return ws_layout(h, max_rows).total;
}

int sdfa_headtrain_forward(sdfa_headtrain *h, const float *d_z, const int64_t *d_speaker_id, int64_t N, float *d_coef,
                           void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "forward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_z || !d_speaker_id || !d_coef) return sdfa_fail(SDFA_EINVAL, "headtrain_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = ws_layout(h, N);
    float *f = (float *)d_ws;
    h->ts.fwd_N = 0;                                        // a forward that fails half way is no forward
    HIP_TRY(headtrain_fold(h->t, h->ts.d_param, h->d_W, h->d_inv, h->d_sc, st));
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
    h->ts.fwd_N = N;
    h->ts.fwd_ws = d_ws;
    return SDFA_OK;
}

int sdfa_headtrain_backward(sdfa_headtrain *h, const float *d_dcoef, int64_t N, float *d_dz, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_call(h, "backward", N, d_ws, ws_bytes);
    if (rc < 0) return rc;
    if (!d_dcoef) return sdfa_fail(SDFA_EINVAL, "headtrain_backward: null pointer");
    const int rf = ts_check_forward(h->ts, MOD, N, d_ws, "rows");
    if (rf < 0) return rf;
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
    a.nblk = w.nblk;
    a.psw = h->wnumel;
    a.psb = h->t.rows;
    for (int depth = 2; depth >= 0; --depth) {
        int coff = 0;
        for (int b = 0; b < h->nb; ++b) {
            const int li = l1 + 3 * b + depth;
            if (depth == 2) a.b[b] = bwd_job(h, w, f, li, d_dcoef + coff, h->kc, f + w.h2[b], f + w.h2[b], f + w.d2[b]);
            else if (depth == 1) a.b[b] = bwd_job(h, w, f, li, f + w.d2[b], 256, f + w.h1[b], f + w.h1[b], f + w.d1[b]);
            else a.b[b] = bwd_job(h, w, f, li, f + w.d1[b], 512, x1, dg ? f + w.h0 : nullptr, dg ? f + w.d0 : d_dz);
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
        a.b[0] = a.b[1] = bwd_job(h, w, f, 0, f + w.d0, 512, f + w.z, nullptr, d_dz);
        a.tkx = a.b[0].Kin / SDFA_HEADTRAIN_TILE;
        a.dx_mode = d_dz ? HT_DX_PLAIN : HT_DX_NONE;
        a.act_prev = HT_ACT_LINEAR;
        HIP_TRY(headtrain_backward_layer(a, st));
    }
    if (w.nblk > 1) {
        HtReduceArgs r;
        r.t = h->t;
        r.pW = f + w.partW;
        r.pb = f + w.partb;
        r.dW = h->d_dW;
        r.grads = h->ts.d_grad;
        r.wnumel = h->wnumel;
        r.nblk = w.nblk;
        HIP_TRY(headtrain_reduce(r, st));
    }
    HIP_TRY(headtrain_wnorm_backward(h->t, h->ts.d_param, h->d_dW, h->d_inv, h->d_sc, h->ts.d_grad, st));
    return SDFA_OK;
}

int sdfa_headtrain_adam(sdfa_headtrain *h, double lr, double beta1, double beta2, double eps, void *stream) {
    return ts_adam(ts_of(h), MOD, lr, beta1, beta2, eps, stream);
}

int sdfa_headtrain_zero_grad(sdfa_headtrain *h, void *stream) { return ts_zero_grad(ts_of(h), MOD, stream); }

int sdfa_headtrain_get_tensor(sdfa_headtrain *h, const char *name, int what, float *h_dst, int64_t numel) {
    int64_t off = 0;
    const int slot = locate(h, "headtrain_get_tensor", name, h_dst, numel, &off);
    return slot < 0 ? slot : ts_get_tensor(h->ts, MOD, what, off, h_dst, numel);
}

int sdfa_headtrain_set_state(sdfa_headtrain *h, const char *name, int what, const float *h_src, int64_t numel) {
    int64_t off = 0;
    const int slot = locate(h, "headtrain_set_state", name, h_src, numel, &off);
    return slot < 0 ? slot : ts_set_state(h->ts, MOD, what, off, h_src, numel);
}

int sdfa_headtrain_set_grad(sdfa_headtrain *h, const char *name, const float *h_src, int64_t numel) {
    return sdfa_headtrain_set_state(h, name, SDFA_HEADTRAIN_GRAD, h_src, numel);
}

int64_t sdfa_headtrain_step_count(const sdfa_headtrain *h) { return ts_step_count(ts_of(h), MOD); }
int sdfa_headtrain_set_step_count(sdfa_headtrain *h, int64_t t) { return ts_set_step_count(ts_of(h), MOD, t); }

}  // extern "C"
