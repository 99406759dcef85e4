"""Float64 restatement of the frequency LSTM's training step (include/sdfa_freqtrain.h) on R columns, for any R: the input
projection with the biases, the recurrence along the 32 frequency bins, X0 = HF Wp^T + bp, the analytic backward (dbp, dWp, dHF,
back-propagation through the 32 steps, dW_ih, dW_hh, db, dC), and torch.optim.Adam -- each value with a propagated first-order
error scale kappa for the float32 operations the device forms it with.  kappa is built by the rules of tests/headtrain_ref64.py,
which derives them (LAMBDA, U and adam are imported from it), with the activation and product rules of tests/lstmtrain_ref64.py
(imported as well: the device uses the same sigmoidf_acc / tanhf_acc and the same gate formulas).  What is particular here:

    pre         C W_ih^T is one chain of 64 products: sqrt(64 + 1) U sum |C W|.  b = b_ih + b_hh is one float32 addition
                (U |b|) and pre + b another (U |pre + b|); both add linearly, as elementwise operations do.
    step        a step's pre-activation is one chain of pre_f and 128 recurrent products: sqrt(128 + 2) U (|pre| + sum |W_hh h|)
                on top of the error pre brings, incoming errors of h in quadrature through W_hh^2.
    X0          one chain of 8,192 products, the errors of HF in quadrature through Wp^2; the bias one addition.
    dHF         one chain of 256 products.
    rows        dWp, dbp contract over the R columns, dW_ih, dW_hh, db over the 32 R pairs (column, step): incoming errors are
                added linearly, the summation sqrt(n + 1) U sum |a b| for any order, which covers the row-block partials.
    dC          one chain over both directions' 1,024 gate rows.

`flaw` builds deliberately wrong models, the controls: "bias_ih_only" (the bias gradient given to bias_ih only), "dwhh_h_t" (dW_hh
with h_f instead of h_{f-1}), "reverse_forward" (the reverse direction run forward), "wp_dfu" (Wp's columns read as [d][f][u]),
"no_dbp" (dbp left out), "dc_forward_only" (dC from the forward direction's gates only), "c_init" (a direction's first step reading
c_f where c_{-1} = 0 belongs, in df)."""
import numpy as np

from headtrain_ref64 import LAMBDA, U, adam
from lstmtrain_ref64 import _mul, _one_minus_sq, _s_prime, _sig, _tanh

FLAWS = ("bias_ih_only", "dwhh_h_t", "reverse_forward", "wp_dfu", "no_dbp", "dc_forward_only", "c_init")
FAMILIES = ("default", "carry")
COLS, NS, NI, NH, NG, NO = 64, 32, 64, 128, 512, 256
NK = NS * 2 * NH
P = "_audio_encoder._layers.6."
CARRY_SHIFT = 3.0                       # added to the forget rows of bias_ih: sigmoid(3) = 0.95


def names():
    """the ten tensors in the order of the device's flat buffers"""
    out = [f"{P}_lstm.{kind}_l0{suffix}" for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for suffix in ("", "_reverse")]
    return tuple(out + [P + "_proj.weight", P + "_proj.bias"])


def shapes():
    n = names()
    return {n[0]: (NG, NI), n[1]: (NG, NI), n[2]: (NG, NH), n[3]: (NG, NH), n[4]: (NG,), n[5]: (NG,), n[6]: (NG,), n[7]: (NG,),
            n[8]: (NO, NK), n[9]: (NO,)}


def case(R, seed, family="default"):
    """Seeded float32 inputs of R columns.  "default": weights and biases as torch initialises them, uniform(+-1/sqrt(128)) for
    the LSTM and uniform(+-1/sqrt(8192)) for the projection; C = tanh(gaussian).  "carry": the forget rows of both directions'
    bias_ih carry an extra CARRY_SHIFT, so the forget gate is open and the gradient reaches far back through the cell state.
    dX0 = (gaussian + 1) / R: a common component, as a loss gradient has (the sums over the rows then grow with R, as their
    kappa does)."""
    assert family in FAMILIES, family
    rs = np.random.RandomState(seed)
    f32 = np.float32
    params = {}
    for n, s in shapes().items():
        b = 1.0 / np.sqrt(NK if "_proj" in n else NH)
        params[n] = rs.uniform(-b, b, s).astype(f32)
    if family == "carry":
        for n in names()[4:6]:
            params[n][NH:2 * NH] += f32(CARRY_SHIFT)
    C = np.tanh(rs.normal(0, 1, (R, NS, NI))).astype(f32)
    dX0 = ((rs.normal(0, 1, (R, NO)) + 1.0) / R).astype(f32)
    return dict(family=family, params=params, C=C, dX0=dX0)


def _f64(a):
    return np.asarray(a, np.float64)


def _mm(a, b):
    """a @ b, or 0 where an operand is all zeros: the error terms of exact inputs (no dparams, no kC) cost nothing"""
    return a @ b if a.any() and b.any() else 0.0


def _forward_direction(C, eC, Wih, eWih, Whh, eWhh, b, eb):
    """One direction over ASCENDING steps (the caller flips the reverse direction's step axis): sigmas in, sigmas out."""
    R = C.shape[0]
    pairs = R * NS
    Cf, eCf = C.reshape(pairs, NI), eC.reshape(pairs, NI)
    acc = Cf @ Wih.T
    e_acc = np.sqrt(_mm(eCf * eCf, (Wih * Wih).T) + _mm(Cf * Cf, (eWih * eWih).T) + (np.sqrt(NI + 1) * U * (np.abs(Cf) @ np.abs(Wih).T)) ** 2)
    pre = (acc + b).reshape(R, NS, NG)
    e_pre = (e_acc + eb).reshape(R, NS, NG) + U * np.abs(pre)
    W2, aW, eW2 = Whh * Whh, np.abs(Whh), eWhh * eWhh
    z3 = lambda w: np.zeros((R, NS, w))
    k = dict(gi=z3(NH), gf=z3(NH), gg=z3(NH), go=z3(NH), c=z3(NH), h=z3(NH), e_gi=z3(NH), e_gf=z3(NH), e_gg=z3(NH), e_go=z3(NH),
             e_c=z3(NH), e_h=z3(NH))
    hp, e_hp, cp, e_cp = (np.zeros((R, NH)) for _ in range(4))
    for t in range(NS):
        a = pre[:, t] + hp @ Whh.T
        e_a = np.sqrt(e_pre[:, t] ** 2 + _mm(e_hp * e_hp, W2.T) + _mm(hp * hp, eW2.T) + (np.sqrt(NH + 2) * U * (np.abs(pre[:, t]) + np.abs(hp) @ aW.T)) ** 2)
        k["gi"][:, t], k["e_gi"][:, t] = _sig(a[:, :NH], e_a[:, :NH])
        k["gf"][:, t], k["e_gf"][:, t] = _sig(a[:, NH:2 * NH], e_a[:, NH:2 * NH])
        k["gg"][:, t], k["e_gg"][:, t] = _tanh(a[:, 2 * NH:3 * NH], e_a[:, 2 * NH:3 * NH])
        k["go"][:, t], k["e_go"][:, t] = _sig(a[:, 3 * NH:], e_a[:, 3 * NH:])
        ig, e_ig = _mul(k["gi"][:, t], k["e_gi"][:, t], k["gg"][:, t], k["e_gg"][:, t])
        k["c"][:, t] = k["gf"][:, t] * cp + ig
        k["e_c"][:, t] = k["e_gf"][:, t] * np.abs(cp) + k["gf"][:, t] * e_cp + e_ig + U * np.abs(k["c"][:, t])
        tc, e_tc = _tanh(k["c"][:, t], k["e_c"][:, t])
        k["h"][:, t], k["e_h"][:, t] = _mul(k["go"][:, t], k["e_go"][:, t], tc, e_tc)
        hp, e_hp, cp, e_cp = k["h"][:, t], k["e_h"][:, t], k["c"][:, t], k["e_c"][:, t]
    k.update(Cf=Cf, eCf=eCf)
    return k


def _backward_direction(k, Whh, eWhh, dY, edY, flaw):
    """BPTT of one direction over its ascending steps, dY = this direction's share of dHF: dG, the weight and bias gradients."""
    R = dY.shape[0]
    pairs = R * NS
    W2, aW, eW2 = Whh * Whh, np.abs(Whh), eWhh * eWhh
    dG, e_dG = np.zeros((R, NS, NG)), np.zeros((R, NS, NG))
    rec, e_rec, dc, e_dc = (np.zeros((R, NH)) for _ in range(4))
    c, e_c, h, e_h = k["c"], k["e_c"], k["h"], k["e_h"]
    for t in range(NS - 1, -1, -1):
        dh = dY[:, t] + rec
        e_dh = edY[:, t] + e_rec + U * np.abs(dh)
        tc, e_tc = _tanh(c[:, t], e_c[:, t])
        if t > 0:
            cprev, e_cprev = c[:, t - 1], e_c[:, t - 1]
        elif flaw == "c_init":
            cprev, e_cprev = c[:, t], e_c[:, t]
        else:
            cprev, e_cprev = np.zeros((R, NH)), np.zeros((R, NH))
        i_, f_, g_, o_ = k["gi"][:, t], k["gf"][:, t], k["gg"][:, t], k["go"][:, t]
        ei, ef, eg, eo = k["e_gi"][:, t], k["e_gf"][:, t], k["e_gg"][:, t], k["e_go"][:, t]
        p1, e_p1 = _mul(dh, e_dh, tc, e_tc)
        so, e_so = _s_prime(o_, eo)
        d_o, e_do = _mul(p1, e_p1, so, e_so)
        p2, e_p2 = _mul(dh, e_dh, o_, eo)
        f2, e_f2 = _one_minus_sq(tc, e_tc)
        d = p2 * f2 + dc
        e_d = e_p2 * np.abs(f2) + np.abs(p2) * e_f2 + e_dc + U * np.abs(d)
        q, e_q = _mul(d, e_d, g_, eg)
        si, e_si = _s_prime(i_, ei)
        d_i, e_di = _mul(q, e_q, si, e_si)
        q, e_q = _mul(d, e_d, cprev, e_cprev)
        sf, e_sf = _s_prime(f_, ef)
        d_f, e_df = _mul(q, e_q, sf, e_sf)
        q, e_q = _mul(d, e_d, i_, ei)
        gp, e_gp = _one_minus_sq(g_, eg)
        d_g, e_dg = _mul(q, e_q, gp, e_gp)
        dG[:, t] = np.concatenate([d_i, d_f, d_g, d_o], 1)
        e_dG[:, t] = np.concatenate([e_di, e_df, e_dg, e_do], 1)
        dc, e_dc = _mul(d, e_d, f_, ef)
        g_t, eg_t = dG[:, t], e_dG[:, t]
        rec = g_t @ Whh
        e_rec = np.sqrt((eg_t * eg_t) @ W2 + _mm(g_t * g_t, eW2) + (np.sqrt(NG + 1) * U * (np.abs(g_t) @ aW)) ** 2)
    hprev, e_hprev = np.zeros_like(h), np.zeros_like(h)
    if flaw == "dwhh_h_t":
        hprev, e_hprev = h, e_h
    else:
        hprev[:, 1:], e_hprev[:, 1:] = h[:, :-1], e_h[:, :-1]
    Gf, eGf, aGf = dG.reshape(pairs, NG), e_dG.reshape(pairs, NG), np.abs(dG).reshape(pairs, NG)
    Hf, eHf = hprev.reshape(pairs, NH), e_hprev.reshape(pairs, NH)
    Cf, eCf = k["Cf"], k["eCf"]
    s = np.sqrt(pairs + 1) * U
    return dict(dG=dG, e_dG=e_dG, hprev=hprev, e_hprev=e_hprev,
                dWih=Gf.T @ Cf, e_dWih=eGf.T @ np.abs(Cf) + _mm(aGf.T, eCf) + s * (aGf.T @ np.abs(Cf)),
                dWhh=Gf.T @ Hf, e_dWhh=eGf.T @ np.abs(Hf) + aGf.T @ eHf + s * (aGf.T @ np.abs(Hf)),
                db=Gf.sum(0), e_db=eGf.sum(0) + s * aGf.sum(0))


def run(params, C, dX0=None, dparams=None, flaw=None, kC=None, kdX0=None, want_dC=True, pieces=False):
    """float32 inputs -> dict: X0, HF, dC, grads {name: array} in float64 and their kappas k_X0, k_HF, k_dC, k_grads; mean_f, the
    mean forget gate.  dX0 None: forward only.  kC, kdX0: kappas of C and dX0 where they are another stage's outputs.
    pieces=True adds "pieces": the per-column operands of every contraction over the rows and their sigmas, the very arrays
    contracted here (tests/bigbatch_ref64.py builds a periodic batch's gradients from them): D = dX0 [R][256] and HF [R][8192] with
    e_D, e_HF for dWp and dbp; "dirs", per direction dG [R][32][512] (in the direction's own ascending step order, as contracted),
    Cf [32 R][64] and hprev [R][32][128] with e_dG, eCf, e_hprev for dW_ih, dW_hh and db."""
    assert flaw is None or flaw in FLAWS, flaw
    C = _f64(C)
    R = C.shape[0]
    assert C.shape == (R, NS, NI), C.shape
    nm = names()
    W = [_f64(params[n]) for n in nm]
    eW = [_f64(dparams[n]) / LAMBDA if dparams else np.zeros_like(w) for n, w in zip(nm, W)]            # kappa in, sigma inside
    eC = np.zeros_like(C) if kC is None else _f64(kC) / LAMBDA
    Wp, eWp, bp, ebp = W[8], eW[8], W[9], eW[9]
    if flaw == "wp_dfu":        # the device's HF index f 256 + d 128 + u taken for d 4096 + f 128 + u
        perm = np.arange(NK).reshape(2, NS, NH).transpose(1, 0, 2).reshape(NK)
        Wp, eWp = Wp[:, perm], eWp[:, perm]
    res = []
    for d in (0, 1):
        flip = d == 1 and flaw != "reverse_forward"
        tr = (lambda a: a[:, ::-1]) if flip else (lambda a: a)
        b = W[4 + d] + W[6 + d]
        eb = eW[4 + d] + eW[6 + d] + U * np.abs(b)
        res.append((_forward_direction(tr(C), tr(eC), W[d], eW[d], W[2 + d], eW[2 + d], b, eb), tr))
    HF = np.stack([tr(k["h"]) for k, tr in res], 2).reshape(R, NK)                  # [R][f][d][u]
    eHF = np.stack([tr(k["e_h"]) for k, tr in res], 2).reshape(R, NK)
    acc = HF @ Wp.T
    e_acc = np.sqrt((eHF * eHF) @ (Wp * Wp).T + _mm(HF * HF, (eWp * eWp).T) + (np.sqrt(NK + 1) * U * (np.abs(HF) @ np.abs(Wp).T)) ** 2)
    X0 = acc + bp
    eX0 = e_acc + ebp + U * np.abs(X0)
    out = dict(X0=X0, k_X0=LAMBDA * eX0, HF=HF, k_HF=LAMBDA * eHF, mean_f=float(np.mean([k["gf"].mean() for k, _ in res])))
    if dX0 is None:
        return out
    D = _f64(dX0)
    assert D.shape == (R, NO), D.shape
    eD = np.zeros_like(D) if kdX0 is None else _f64(kdX0) / LAMBDA
    aD = np.abs(D)
    s = np.sqrt(R + 1) * U
    grads, kg = {}, {}
    dWp, e_dWp = D.T @ HF, _mm(eD.T, np.abs(HF)) + aD.T @ eHF + s * (aD.T @ np.abs(HF))
    if flaw == "wp_dfu":
        inv = np.argsort(perm)
        dWp, e_dWp = dWp[:, inv], e_dWp[:, inv]
    grads[nm[8]], kg[nm[8]] = dWp, LAMBDA * e_dWp
    grads[nm[9]], kg[nm[9]] = (np.zeros(NO) if flaw == "no_dbp" else D.sum(0)), LAMBDA * (eD.sum(0) + s * aD.sum(0))
    dHF = (D @ Wp).reshape(R, NS, 2, NH)
    e_dHF = np.sqrt(_mm(eD * eD, Wp * Wp) + _mm(D * D, eWp * eWp) + (np.sqrt(NO + 1) * U * (aD @ np.abs(Wp))) ** 2).reshape(R, NS, 2, NH)
    back = []
    for d in (0, 1):
        k, tr = res[d]
        r = _backward_direction(k, W[2 + d], eW[2 + d], tr(dHF[:, :, d]), tr(e_dHF[:, :, d]), flaw)
        own = dict(dG=r["dG"], e_dG=r["e_dG"], Cf=k["Cf"], eCf=k["eCf"], hprev=r["hprev"], e_hprev=r["e_hprev"])
        r["dG"], r["e_dG"] = tr(r["dG"]), tr(r["e_dG"])
        back.append((r, own))
        grads[nm[d]], kg[nm[d]] = r["dWih"], LAMBDA * r["e_dWih"]
        grads[nm[2 + d]], kg[nm[2 + d]] = r["dWhh"], LAMBDA * r["e_dWhh"]
        grads[nm[4 + d]], kg[nm[4 + d]] = r["db"], LAMBDA * r["e_db"]
        grads[nm[6 + d]], kg[nm[6 + d]] = (np.zeros(NG) if flaw == "bias_ih_only" else r["db"]), LAMBDA * r["e_db"]
    out.update(grads=grads, k_grads=kg, dHF=dHF.reshape(R, NK), k_dHF=LAMBDA * e_dHF.reshape(R, NK))
    if want_dC:
        pairs = R * NS
        G = [r["dG"].reshape(pairs, NG) for r, _ in back]
        eG = [r["e_dG"].reshape(pairs, NG) for r, _ in back]
        use = (0,) if flaw == "dc_forward_only" else (0, 1)
        dC = sum(G[d] @ W[d] for d in use)
        q = sum((eG[d] * eG[d]) @ (W[d] * W[d]) + _mm(G[d] * G[d], eW[d] * eW[d]) for d in (0, 1))
        e_dC = np.sqrt(q + (np.sqrt(2 * NG + 1) * U * (np.abs(G[0]) @ np.abs(W[0]) + np.abs(G[1]) @ np.abs(W[1]))) ** 2)
        out.update(dC=dC.reshape(R, NS, NI), k_dC=LAMBDA * e_dC.reshape(R, NS, NI))
    if pieces:
        out["pieces"] = dict(D=D, e_D=eD, HF=HF, e_HF=eHF, dirs=[own for _, own in back])
    return out


def train_steps(c, steps, flaw=None, lr=1e-4):
    """`steps` full steps on the case `c` (the same batch every step) in float64, the errors carried from step to step:
    -> (params, exp_avg, exp_avg_sq, k_params, k_exp_avg, k_exp_avg_sq, first step's run, which also carries the parameters
    after that step as params1, k_params1)."""
    nm = list(c["params"])
    p = {n: _f64(c["params"][n]) for n in nm}
    m = {n: np.zeros_like(p[n]) for n in nm}
    v = {n: np.zeros_like(p[n]) for n in nm}
    ep = {n: np.zeros_like(p[n]) for n in nm}
    em = {n: np.zeros_like(p[n]) for n in nm}
    ev = {n: np.zeros_like(p[n]) for n in nm}
    first = None
    for t in range(1, steps + 1):
        r = run(p, c["C"], c["dX0"], dparams=ep, flaw=flaw)
        first = first or r
        for n in nm:
            p[n], m[n], v[n], ep[n], em[n], ev[n] = adam(p[n], r["grads"][n], m[n], v[n], t, lr=lr, ep=ep[n], eg=r["k_grads"][n],
                                                         em=em[n], ev=ev[n])
        if t == 1:
            first["params1"], first["k_params1"] = dict(p), dict(ep)      # the state after the first step
    return p, m, v, ep, em, ev, first


def loss(params, C, dX0):
    """the scalar whose gradients `run` states: (X0 * dX0).sum()"""
    return float((run(params, C)["X0"] * _f64(dX0)).sum())
