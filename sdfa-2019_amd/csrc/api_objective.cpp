// Host side of the training objective (include/sdfa_objective.h): the refusals, the partition plan, the
// workspace layout and the launches of objective.hip.  Nothing here copies or synchronises.
#include "host.h"
#include "objective.h"

namespace {

// Workgroups the plan aims at: two per CU of a 256-CU device.  A constant, not the device's count: the partition -- and
// with it the order of the additions -- depends on the shape alone.
constexpr int64_t TARGET_WGS = 512;

struct Plan {
    ObjArgs a;                               // shape fields only; pointers are filled by the call
    int64_t lpart_off, gpart_off, total;     // bytes
};

void plan_part(ObjPart &p, int64_t C, int64_t K, int koff, int G, int S, int OFF, int exp) {
    p.compT = p.means = nullptr;
    p.C = C;
    p.K = (int)K;
    p.KS = (int)round_up(K, 32);
    p.KP = p.KS + 4;
    p.koff = koff;
    p.G = G;
    p.S = S;
    p.OFF = OFF;
    p.exp = exp;
    p.ncb = (int)((C + SDFA_OBJECTIVE_COLS - 1) / SDFA_OBJECTIVE_COLS);
}

int make_plan(const char *who, int64_t N, int64_t W, int64_t Ks, int64_t Kr, int layout, Plan *pl) {
    if (layout != SDFA_OBJECTIVE_LAYOUT_DGRAD && layout != SDFA_OBJECTIVE_LAYOUT_PLAIN) return sdfa_fail(SDFA_EINVAL, "%s: unknown layout %d", who, layout);
    const bool dg = layout == SDFA_OBJECTIVE_LAYOUT_DGRAD;
    if (N < 2 || N % 2 != 0) return sdfa_fail(SDFA_EINVAL, "%s: a batch of %lld rows is not [a; b] with at least one pair", who, (long long)N);
    if (N / 2 > 65535ll * SDFA_OBJECTIVE_PAIRS) return sdfa_fail(SDFA_EINVAL, "%s: %lld rows, at most %lld", who, (long long)N, 2 * 65535ll * SDFA_OBJECTIVE_PAIRS);
    if (W < 1 || W > (1ll << 30)) return sdfa_fail(SDFA_EINVAL, "%s: row width %lld outside 1 .. 2^30", who, (long long)W);
    if (dg && W % 9 != 0) return sdfa_fail(SDFA_EINVAL, "%s: a dgrad row of %lld values is no multiple of 9", who, (long long)W);
    if (Ks < 1 || Ks > SDFA_OBJECTIVE_MAX_K) return sdfa_fail(SDFA_EINVAL, "%s: %lld coefficients outside 1 .. %d", who, (long long)Ks, SDFA_OBJECTIVE_MAX_K);
    if (dg && (Kr < 1 || Kr > SDFA_OBJECTIVE_MAX_K)) return sdfa_fail(SDFA_EINVAL, "%s: %lld rotat coefficients outside 1 .. %d", who, (long long)Kr, SDFA_OBJECTIVE_MAX_K);

    ObjArgs &a = pl->a;
    a.nparts = dg ? 2 : 1;
    a.N = N;
    a.B = N / 2;
    a.W = W;
    a.Kc = (int)(dg ? Ks + Kr : Ks);
    a.rowtiles = (int)((a.B + SDFA_OBJECTIVE_PAIRS - 1) / SDFA_OBJECTIVE_PAIRS);
    a.n = (double)(dg ? W / 9 : W);
    if (dg) {
        plan_part(a.part[0], W / 9 * 6, Ks, 0, 6, 9, 0, 0);
        plan_part(a.part[1], W / 9 * 3, Kr, (int)Ks, 3, 9, 6, 1);
    } else {
        plan_part(a.part[0], W, Ks, 0, 1, 1, 0, 0);
        a.part[1] = a.part[0];
    }
    // column partitions: TARGET_WGS workgroups over the row tiles, shared between the parts by their slab traffic (column
    // blocks x padded K), at least one and at most one per column block
    const int64_t want = TARGET_WGS / a.rowtiles > a.nparts ? TARGET_WGS / a.rowtiles : a.nparts;
    int64_t cost = 0;
    for (int p = 0; p < a.nparts; ++p) cost += (int64_t)a.part[p].ncb * a.part[p].KS;
    int px = 0;
    int64_t goff = 0;
    for (int p = 0; p < a.nparts; ++p) {
        ObjPart &q = a.part[p];
        int64_t P = (want * q.ncb * q.KS + cost / 2) / cost;
        P = P < 1 ? 1 : (P > q.ncb ? q.ncb : P);
        q.P = (int)P;
        q.px0 = px;
        px += q.P;
        q.gpart_off = goff;
        goff += P * 2 * a.rowtiles * 2 * SDFA_OBJECTIVE_PAIRS * q.KS;
    }
    pl->lpart_off = 0;
    pl->gpart_off = round_up((int64_t)px * N * 2 * 8, 256);
    pl->total = pl->gpart_off + round_up(goff * 4, 256);
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_objective_abi_version(void) { return SDFA_OBJECTIVE_ABI_VERSION; }

int64_t sdfa_objective_workspace_bytes(int64_t N, int64_t W, int64_t Ks, int64_t Kr, int layout) {
    Plan pl;
    const int rc = make_plan("objective_workspace_bytes", N, W, Ks, Kr, layout, &pl);
    return rc < 0 ? rc : pl.total;
}

int sdfa_objective(const float *d_coef, int64_t N, int64_t W, int64_t Ks, int64_t Kr, int layout, const float *d_compT_s,
                   const float *d_means_s, const float *d_compT_r, const float *d_means_r, const float *d_truth,
                   const float *d_weight, float *d_loss, double *d_rec, float *d_grad, void *d_ws, int64_t ws_bytes, void *stream) {
    Plan pl;
    const int rc = make_plan("objective", N, W, Ks, Kr, layout, &pl);
    if (rc < 0) return rc;
    const bool dg = layout == SDFA_OBJECTIVE_LAYOUT_DGRAD;
    if (!d_coef || !d_compT_s || !d_means_s || !d_truth || !d_weight || !d_loss || !d_rec || !d_grad || !d_ws || (dg && (!d_compT_r || !d_means_r)))
        return sdfa_fail(SDFA_EINVAL, "objective: null pointer");
    if (ws_bytes < pl.total) return sdfa_fail(SDFA_EINVAL, "objective: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)pl.total);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "objective: workspace not 256-byte aligned");

    ObjArgs &a = pl.a;
    a.part[0].compT = d_compT_s;
    a.part[0].means = d_means_s;
    a.part[1].compT = dg ? d_compT_r : d_compT_s;
    a.part[1].means = dg ? d_means_r : d_means_s;
    a.coef = d_coef;
    a.truth = d_truth;
    a.weight = d_weight;
    a.lpart = (double *)((char *)d_ws + pl.lpart_off);
    a.gpart = (float *)((char *)d_ws + pl.gpart_off);
    a.loss = d_loss;
    a.rec = d_rec;
    a.grad = d_grad;
    HIP_TRY(objective_launch(a, (hipStream_t)stream));
    return SDFA_OK;
}

}  // extern "C"
