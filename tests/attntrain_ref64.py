"""Float64 restatement of the attention layer's training step (include/sdfa_attntrain.h): the query convolution and its
projection, the scores, the softmax, the context z, the analytic backward down to dH, and torch.optim.Adam -- each value with a
propagated first-order error scale kappa for the float32 operations the device forms it with.  kappa is built by the rules of
tests/headtrain_ref64.py, which derives them (the high-probability scale of Higham and Mary's probabilistic model of rounding,
sub-gaussian parameters sigma, kappa = LAMBDA sigma, LAMBDA = 8 from the number of compared elements; nothing is fitted):

    sums        n products summed in ANY order: sigma = sqrt(n + 1) U sum |a b|.  The row-block partials of dWk, dv, db are such
                an order.
    features    incoming errors of a contraction over features (c, k, o, m) are taken as independent: combined in quadrature.
    batch       incoming errors of a contraction over the rows (n, t) -- dWk, dWq, dWc, dv, db, dqp, and z and the softmax's
                sums over t -- share the errors of qp, v and Wk: they are NOT independent and are added linearly.  Elementwise
                operations add linearly as well.
    tanh        sech^2 at the nearest point of the argument's interval times the argument's error, plus K_TANH U |y| (2 ulp).
    tanh'       f = fma(-u, u, 1): 2 |u| du + 2 U;  each product: U.
    softmax     e_t = expf(s_t - max): the relative error of e_t is the error of s_t, U |s_t - max| for the subtraction and
                K_EXP U (expf at its published 1 ulp); the error of max itself cancels (every step subtracts the same number).
                a_t = e_t / sum: the relative errors of e_t and of the sum (the a-weighted mean of the e_j's, sqrt(65) U for
                the additions), U for the division.
    Jacobian    ds_t = a_t (da_t - sum_j a_j da_j) cancels: the errors of da_t and of the sum enter at their ABSOLUTE scale
                (whole, not relative to the small difference), plus U |difference|.
    Adam        headtrain_ref64.adam, unchanged.

Errors of the inputs (the parameters after an earlier step) enter through `dparams` and are propagated like the rounding
errors, so the scale carries over several steps.  H and dz are exact float32 inputs.

`flaw` builds deliberately wrong models, the controls: "no_softmax_sum" (the sum_j a_j da_j term dropped), "no_tanh_prime",
"no_value_term" (a_t dz dropped from dH), "no_window_term" (the query-window term dropped from dH[31 .. 33]), "taps_reversed"
(the conv taps k reversed in dWc), "window_30" (the window taken at 30 .. 32), "no_bias_correction" (Adam)."""
import numpy as np

from headtrain_ref64 import K_TANH, LAMBDA, U, adam
from score_ref64 import K_EXP

FLAWS = ("no_softmax_sum", "no_tanh_prime", "no_value_term", "no_window_term", "taps_reversed", "window_30", "no_bias_correction")
FAMILIES = ("flat", "peaked")
TS, D, NA, W0, KW = 64, 512, 128, 31, 3
P = "_audio_encoder._layers.10."
WC, WQ, WK, V, B = P + "_conv_query.weight", P + "proj_qry.weight", P + "proj_key.weight", P + "v.weight", P + "b"
SHAPES = {WC: (D, D, KW), WQ: (NA, D), WK: (NA, D), V: (1, NA), B: (1, 1, NA)}


def case(N, seed, family="flat"):
    """Seeded float32 inputs of a batch of N frames.  H = tanh(gaussian), bounded like a BiLSTM output.  "flat": Glorot-sized
    parameters (normal, std sqrt(2 / (fan_in + fan_out))), b ~ N(0, 0.05): the largest align is about 0.05.  "peaked": v times
    6 and Wk times 2, so that the largest align exceeds 0.5 in at least half the frames (tests/test_attntrain_ref64_cpu.py
    asserts it).  dz ~ N(0, 1) / N."""
    assert family in FAMILIES, family
    rs = np.random.RandomState(seed)
    f32 = np.float32
    params = {
        WC: rs.normal(0, np.sqrt(2.0 / (KW * D + KW * D)), SHAPES[WC]).astype(f32),
        WQ: rs.normal(0, np.sqrt(2.0 / (D + NA)), SHAPES[WQ]).astype(f32),
        WK: rs.normal(0, np.sqrt(2.0 / (D + NA)), SHAPES[WK]).astype(f32),
        V: rs.normal(0, np.sqrt(2.0 / (NA + 1)), SHAPES[V]).astype(f32),
        B: rs.normal(0, 0.05, SHAPES[B]).astype(f32),
    }
    if family == "peaked":
        params[V] = (params[V] * f32(6.0)).astype(f32)
        params[WK] = (params[WK] * f32(2.0)).astype(f32)
    H = np.tanh(rs.normal(0, 1, (N, TS, D))).astype(f32)
    dz = (rs.normal(0, 1, (N, D)) / N).astype(f32)
    return dict(family=family, params=params, H=H, dz=dz)


def _f64(a):
    return np.asarray(a, np.float64)


def _q(*terms):
    """quadrature"""
    return np.sqrt(sum(t * t for t in terms))


def run(params, H, dz=None, dparams=None, flaw=None, ddz=None, pieces=False):
    """float32 inputs -> dict: z, align, dH, grads {name: array} in float64 and their kappas k_z, k_align, k_dH, k_grads.
    dz None: forward only.  ddz: kappa of dz where it is not an exact input (the head's backward produced it); its elements
    are features of a contraction: quadrature.  pieces: also `pieces`, the operands of the gradients' contractions over rows and
    frames with their sigmas, frame by frame (tests/bigbatch_ref64.py sums them with other frame weights)."""
    assert flaw is None or flaw in FLAWS, flaw
    H = _f64(H)
    N = len(H)
    Wc, Wq, Wk, v, b = (_f64(params[n]) for n in (WC, WQ, WK, V, B))
    v, b = v.reshape(NA), b.reshape(NA)
    if dparams:
        eWc, eWq, eWk, ev, eb = (_f64(dparams[n]) / LAMBDA for n in (WC, WQ, WK, V, B))       # kappa in, sigma inside
        ev, eb = ev.reshape(NA), eb.reshape(NA)
    else:
        eWc, eWq, eWk, ev, eb = (np.zeros_like(a) for a in (Wc, Wq, Wk, v, b))
    # the conv as a matrix over the window in the order (k, c)
    Wc2, eWc2 = Wc.transpose(0, 2, 1).reshape(D, KW * D), eWc.transpose(0, 2, 1).reshape(D, KW * D)
    w0 = 30 if flaw == "window_30" else W0
    hq = H[:, w0:w0 + KW, :].reshape(N, KW * D)
    qc = hq @ Wc2.T
    e_qc = _q(np.sqrt((hq * hq) @ (eWc2 * eWc2).T), np.sqrt(KW * D + 1) * U * (np.abs(hq) @ np.abs(Wc2).T))
    qp = qc @ Wq.T
    e_qp = np.sqrt((e_qc * e_qc) @ (Wq * Wq).T + (qc * qc) @ (eWq * eWq).T + (np.sqrt(D + 1) * U * (np.abs(qc) @ np.abs(Wq).T)) ** 2)
    Hf = H.reshape(N * TS, D)
    KP = (Hf @ Wk.T).reshape(N, TS, NA)
    e_KP = np.sqrt((Hf * Hf) @ (eWk * eWk).T + (np.sqrt(D + 1) * U * (np.abs(Hf) @ np.abs(Wk).T)) ** 2).reshape(N, TS, NA)
    kq = KP + qp[:, None, :]
    pre = kq + b
    e_pre = np.sqrt(e_KP ** 2 + (e_qp ** 2)[:, None, :] + eb ** 2) + U * np.abs(kq) + U * np.abs(pre)
    u = np.tanh(pre)
    e_u = e_pre / np.cosh(np.maximum(np.abs(pre) - LAMBDA * e_pre, 0.0)) ** 2 + K_TANH * U * np.abs(u)
    s = u @ v
    e_s = np.sqrt((e_u * e_u) @ (v * v) + (u * u) @ (ev * ev) + (np.sqrt(NA + 1) * U * (np.abs(u) @ np.abs(v))) ** 2)
    mx = s.max(1, keepdims=True)
    ex = np.exp(s - mx)
    a = ex / ex.sum(1, keepdims=True)
    r_e = e_s + U * np.abs(s - mx) + K_EXP * U
    r_sum = (a * r_e).sum(1, keepdims=True) + np.sqrt(TS + 1) * U
    e_a = a * (r_e + r_sum + U)
    z = np.einsum("nt,ntc->nc", a, H)
    e_z = np.einsum("nt,ntc->nc", e_a, np.abs(H)) + np.sqrt(TS + 1) * U * np.einsum("nt,ntc->nc", a, np.abs(H))
    out = dict(z=z, align=a, k_z=LAMBDA * e_z, k_align=LAMBDA * e_a, qc=qc, u=u)
    if dz is None:
        return out

    dz = _f64(dz)
    da = np.einsum("nc,ntc->nt", dz, H)
    e_dz = np.zeros_like(dz) if ddz is None else _f64(ddz) / LAMBDA
    e_da = _q(np.sqrt(D + 1) * U * np.einsum("nc,ntc->nt", np.abs(dz), np.abs(H)), np.sqrt(np.einsum("nc,ntc->nt", e_dz * e_dz, H * H)))
    dot = (a * da).sum(1, keepdims=True)
    e_dot = (e_a * np.abs(da) + a * e_da).sum(1, keepdims=True) + np.sqrt(TS + 1) * U * (a * np.abs(da)).sum(1, keepdims=True)
    if flaw == "no_softmax_sum":
        dot = np.zeros_like(dot)
    diff = da - dot
    e_diff = e_da + e_dot + U * np.abs(diff)
    ds = a * diff
    e_ds = e_a * np.abs(diff) + a * e_diff + U * np.abs(ds)
    rows = N * TS
    dsu = ds[:, :, None] * u
    grads, kg = {}, {}
    grads[V] = dsu.sum((0, 1)).reshape(SHAPES[V])
    kg[V] = LAMBDA * ((e_ds[:, :, None] * np.abs(u) + np.abs(ds)[:, :, None] * e_u).sum((0, 1)) + np.sqrt(rows + 1) * U * np.abs(dsu).sum((0, 1))).reshape(SHAPES[V])
    g = ds[:, :, None] * v
    e_g = e_ds[:, :, None] * np.abs(v) + np.abs(ds)[:, :, None] * ev + U * np.abs(g)
    f = np.ones_like(u) if flaw == "no_tanh_prime" else 1.0 - u * u
    e_f = 2 * np.abs(u) * e_u + 2 * U
    dpre = g * f
    e_dpre = e_g * np.abs(f) + np.abs(g) * e_f + U * np.abs(dpre)
    grads[B] = dpre.sum((0, 1)).reshape(SHAPES[B])
    kg[B] = LAMBDA * (e_dpre.sum((0, 1)) + np.sqrt(rows + 1) * U * np.abs(dpre).sum((0, 1))).reshape(SHAPES[B])
    dqp = dpre.sum(1)
    e_dqp = e_dpre.sum(1) + np.sqrt(TS + 1) * U * np.abs(dpre).sum(1)
    dpf, e_dpf = dpre.reshape(rows, NA), e_dpre.reshape(rows, NA)
    grads[WK] = dpf.T @ Hf
    kg[WK] = LAMBDA * (e_dpf.T @ np.abs(Hf) + np.sqrt(rows + 1) * U * (np.abs(dpf).T @ np.abs(Hf)))
    grads[WQ] = dqp.T @ qc
    kg[WQ] = LAMBDA * (e_dqp.T @ np.abs(qc) + np.abs(dqp).T @ e_qc + np.sqrt(N + 1) * U * (np.abs(dqp).T @ np.abs(qc)))
    dqc = dqp @ Wq
    e_dqc = np.sqrt((e_dqp * e_dqp) @ (Wq * Wq) + (dqp * dqp) @ (eWq * eWq) + (np.sqrt(NA + 1) * U * (np.abs(dqp) @ np.abs(Wq))) ** 2)
    dWc2 = dqc.T @ hq
    k_dWc2 = LAMBDA * (e_dqc.T @ np.abs(hq) + np.sqrt(N + 1) * U * (np.abs(dqc).T @ np.abs(hq)))
    dWc, k_dWc = (x.reshape(D, KW, D).transpose(0, 2, 1) for x in (dWc2, k_dWc2))
    if flaw == "taps_reversed":
        dWc = dWc[:, :, ::-1]
    grads[WC], kg[WC] = np.ascontiguousarray(dWc), np.ascontiguousarray(k_dWc)
    dHq = (dqc @ Wc2).reshape(N, KW, D)
    e_dHq = np.sqrt((e_dqc * e_dqc) @ (Wc2 * Wc2) + (dqc * dqc) @ (eWc2 * eWc2) + (np.sqrt(D + 1) * U * (np.abs(dqc) @ np.abs(Wc2))) ** 2).reshape(N, KW, D)
    dHk = (dpf @ Wk).reshape(N, TS, D)
    e_dHk = np.sqrt((e_dpf * e_dpf) @ (Wk * Wk) + (dpf * dpf) @ (eWk * eWk) + (np.sqrt(NA + 1) * U * (np.abs(dpf) @ np.abs(Wk))) ** 2).reshape(N, TS, D)
    val = a[:, :, None] * dz[:, None, :]
    dH = dHk if flaw == "no_value_term" else dHk + val
    e_dH = e_dHk + e_a[:, :, None] * np.abs(dz)[:, None, :] + a[:, :, None] * e_dz[:, None, :] + U * np.abs(dH)
    if flaw != "no_window_term":
        dH = dH.copy()
        dH[:, w0:w0 + KW] += dHq
        e_dH[:, w0:w0 + KW] += e_dHq + U * np.abs(dH[:, w0:w0 + KW])
    out.update(dH=dH, k_dH=LAMBDA * e_dH, grads=grads, k_grads=kg)
    if pieces:
        out["pieces"] = dict(H=H, hq=hq, qc=qc, e_qc=e_qc, u=u, e_u=e_u, ds=ds, e_ds=e_ds, dpre=dpre, e_dpre=e_dpre, dqp=dqp, e_dqp=e_dqp,
                             dqc=dqc, e_dqc=e_dqc)
    return out


def train_steps(c, steps, flaw=None, lr=1e-4):
    """`steps` full steps on the case `c` (the same batch every step) in float64, the errors carried from step to step:
    -> (params, exp_avg, exp_avg_sq, k_params, k_exp_avg, k_exp_avg_sq, first step's run)."""
    names = list(c["params"])
    p = {n: _f64(c["params"][n]) for n in names}
    m = {n: np.zeros_like(p[n]) for n in names}
    v = {n: np.zeros_like(p[n]) for n in names}
    ep = {n: np.zeros_like(p[n]) for n in names}
    em = {n: np.zeros_like(p[n]) for n in names}
    ev = {n: np.zeros_like(p[n]) for n in names}
    first = None
    for t in range(1, steps + 1):
        r = run(p, c["H"], c["dz"], dparams=ep, flaw=flaw)
        first = first or r
        for n in names:
            p[n], m[n], v[n], ep[n], em[n], ev[n] = adam(p[n], r["grads"][n], m[n], v[n], t, lr=lr, ep=ep[n], eg=r["k_grads"][n],
                                                         em=em[n], ev=ev[n], flaw=flaw)
    return p, m, v, ep, em, ev, first


def loss(params, H, dz):
    """the scalar whose gradients `run` states: (z * dz).sum()"""
    return float((run(params, H)["z"] * _f64(dz)).sum())
