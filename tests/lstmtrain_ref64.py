"""Float64 restatement of one bidirectional LSTM layer's training step (include/sdfa_lstmtrain.h): the input projection, the
recurrence, back-propagation through time down to dX, the weight gradients, and torch.optim.Adam -- each value with a propagated
first-order error scale kappa for the float32 operations the device forms it with.  One layer for either input width (256:
layer 0, 512: layer 1); `stack` composes the two into the encoder's layer 9.  kappa is built by the rules of
tests/headtrain_ref64.py, which derives them (the high-probability scale of Higham and Mary's probabilistic model of rounding,
sub-gaussian parameters sigma, kappa = LAMBDA sigma, LAMBDA = 8 from the number of compared elements; nothing is fitted):

    sums        n products summed in ANY order: sigma = sqrt(n + 1) U sum |a b|.  A step's pre-activation is one chain of the
                step's pre (itself I products) and 256 recurrent products: sqrt(256 + 2) U (|pre| + sum |W_hh h|) on top of the
                error pre brings.  The row-block partials of dW_ih, dW_hh are such an order.
    features    incoming errors of a contraction over features (input columns, hidden units, gate rows) are taken as
                independent: combined in quadrature.  That is how the recurrence's error is carried from step to step: the
                error of h_{t-1} enters step t through W_hh^2, the error of dG_{t+1} enters dh_t through (W_hh^T)^2.
    rows        incoming errors of a contraction over the rows (n, t) -- dW_ih, dW_hh -- share the errors of the weights: they
                are NOT independent and are added linearly.  Elementwise operations add linearly as well; the cell state's
                error is carried by |f| and dc's by |f| in the same way.
    sigmoid     the device forms s = rcp(1 + e), e = exp2(-x log2e) (sigmoidf_acc of csrc/common.h, which states v_exp_f32 and
                v_rcp_f32 at 1-2 ulp; 2 ulp = 4 U relative is taken for each).  e carries U |x| for the rounded product, U |x|
                for the float32 constant and 4 U for the instruction; de enters s as s^2 de = s (1 - s) times the relative
                error; 1 + e, the reciprocal: U + 4 U relative to s.  Absolute: s (1 - s) (2 U |x| + 4 U) + 5 U s, plus
                s (1 - s) times the argument's error.
    tanh        t = (1 - e) rcp(1 + e), e = exp2(-2 |x| log2e) (tanhf_acc): e carries 2 U |2 x| + 4 U relative; d t / d e =
                -2 / (1 + e)^2 and 4 e / (1 + e)^2 = 1 - t^2, so e's error enters as (1 - t^2) / 2 times the relative error;
                1 - e, 1 + e, the reciprocal, the product: U + U + 4 U + U relative to t.  Absolute:
                (1 - t^2) / 2 (4 U |x| + 4 U) + 7 U |t| -- 2 U at x = 0, the cancellation in 1 - e -- plus sech^2 at the nearest
                point of the argument's interval times the argument's error.
    cell        ig = i g: U;  c_t = fma(f, c_{t-1}, ig): one rounding, U |c_t|;  h_t = o tanh(c_t): U.
    backward    every product U;  o (1 - o): |1 - 2 o| do + 2 U o (1 - o) (the subtraction, the product);  fma(-y, y, 1):
                2 |y| dy + 2 U, as headtrain_ref64 takes it;  dh = dY + dh_rec: U.
    Adam        headtrain_ref64.adam, unchanged.

Errors of the inputs enter through `dparams` (the parameters after an earlier step), `kX` (X where it is another layer's output)
and `kdY` (dY where it is another layer's dX) and are propagated like the rounding errors.

`flaw` builds deliberately wrong models, the controls: "no_dc_carry" (dc <- dc f dropped), "no_tanh_prime_g" (tanh' omitted on
g), "gates_ifog" (the gate rows read as i, f, o, g), "reverse_forward" (the reverse direction run forward), "dwhh_h_t" (dW_hh
with h_t instead of h_{t-1}), "no_rec_term" (W_hh^T dG dropped from dh), "c_init" (a direction's first step reading c_t where
c_{-1} = 0 belongs, in df), "no_bias_correction" (Adam)."""
import numpy as np

from headtrain_ref64 import LAMBDA, U, adam

FLAWS = ("no_dc_carry", "no_tanh_prime_g", "gates_ifog", "reverse_forward", "dwhh_h_t", "no_rec_term", "c_init", "no_bias_correction")
FAMILIES = ("default", "carry")
TS, NH, NG, NY = 64, 256, 1024, 512
IN_DIM = {0: 256, 1: 512}
P = "_audio_encoder._layers.9."
CARRY_SHIFT = 3.0                       # the common component of the forget rows' weight on the constant feature: sigmoid(3) = 0.95


def names(layer):
    """(W_ih, W_ih reverse, W_hh, W_hh reverse) of a layer, the order of the device's flat buffers"""
    return tuple(f"{P}weight_{kind}_l{layer}{suffix}" for kind in ("ih", "hh") for suffix in ("", "_reverse"))


def shapes(layer):
    n = names(layer)
    return {n[0]: (NG, IN_DIM[layer]), n[1]: (NG, IN_DIM[layer]), n[2]: (NG, NH), n[3]: (NG, NH)}


def case(layer, N, seed, family="default"):
    """Seeded float32 inputs of a batch of N frames for one layer.  "default": weights uniform(+-1/16) as torch initialises
    nn.LSTM(hidden 256), X = tanh(gaussian).  "carry": feature 0 of X is the constant 1 and the forget rows of W_ih weigh it with
    an extra CARRY_SHIFT, so the mean forget gate is at least 0.9 (tests/test_lstmtrain_ref64_cpu.py asserts it) and the gradient
    reaches far back through the cell state.  dY ~ N(0, 1) / N."""
    assert family in FAMILIES, family
    rs = np.random.RandomState(seed)
    f32 = np.float32
    params = {n: rs.uniform(-1.0 / 16, 1.0 / 16, s).astype(f32) for n, s in shapes(layer).items()}
    X = np.tanh(rs.normal(0, 1, (N, TS, IN_DIM[layer]))).astype(f32)
    if family == "carry":
        X[:, :, 0] = 1.0
        for n in names(layer)[:2]:
            params[n][NH:2 * NH, 0] += f32(CARRY_SHIFT)
    dY = (rs.normal(0, 1, (N, TS, NY)) / N).astype(f32)
    return dict(layer=layer, family=family, params=params, X=X, dY=dY)


def stack_case(N, seed, family="default"):
    """Both layers: layer 0's case (its X is the stack's input) and layer 1's parameters; dY belongs to the stack's output."""
    c0, c1 = case(0, N, seed, family), case(1, N, seed + 7919, family)
    return dict(family=family, params={**c0["params"], **c1["params"]}, X=c0["X"], dY=c1["dY"])


def _f64(a):
    return np.asarray(a, np.float64)


def _sig(x, e_x):
    s = 1.0 / (1.0 + np.exp(-x))
    return s, s * (1.0 - s) * (e_x + 2 * U * np.abs(x) + 4 * U) + 5 * U * s


def _tanh(x, e_x):
    t = np.tanh(x)
    return t, e_x / np.cosh(np.maximum(np.abs(x) - LAMBDA * e_x, 0.0)) ** 2 + 0.5 * (1.0 - t * t) * (4 * U * np.abs(x) + 4 * U) + 7 * U * np.abs(t)


def _mul(a, e_a, b, e_b):
    p = a * b
    return p, e_a * np.abs(b) + np.abs(a) * e_b + U * np.abs(p)


def _one_minus_sq(y, e_y):
    return 1.0 - y * y, 2 * np.abs(y) * e_y + 2 * U


def _s_prime(s, e_s):
    return s * (1.0 - s), np.abs(1.0 - 2.0 * s) * e_s + 2 * U * s * (1.0 - s)


def _direction(X, eX, Wih, eWih, Whh, eWhh, dY, edY, flaw, pieces=False):
    """One direction over ASCENDING steps (the caller flips the reverse direction's time axis): sigmas in, sigmas out."""
    N, I = X.shape[0], X.shape[2]
    rows = N * TS
    Xf, eXf = X.reshape(rows, I), eX.reshape(rows, I)
    pre = (Xf @ Wih.T).reshape(N, TS, NG)
    e_pre = np.sqrt((eXf * eXf) @ (Wih * Wih).T + (Xf * Xf) @ (eWih * eWih).T + (np.sqrt(I + 1) * U * (np.abs(Xf) @ np.abs(Wih).T)) ** 2).reshape(N, TS, NG)
    W2, aW, eW2 = Whh * Whh, np.abs(Whh), eWhh * eWhh
    z3 = lambda w: np.zeros((N, TS, w))
    gi, gf, gg, go, c, h = z3(NH), z3(NH), z3(NH), z3(NH), z3(NH), z3(NH)
    e_gi, e_gf, e_gg, e_go, e_c, e_h = z3(NH), z3(NH), z3(NH), z3(NH), z3(NH), z3(NH)
    hp, e_hp, cp, e_cp = (np.zeros((N, NH)) for _ in range(4))
    for t in range(TS):
        a = pre[:, t] + hp @ Whh.T
        e_a = np.sqrt(e_pre[:, t] ** 2 + (e_hp * e_hp) @ W2.T + (hp * hp) @ eW2.T + (np.sqrt(NH + 2) * U * (np.abs(pre[:, t]) + np.abs(hp) @ aW.T)) ** 2)
        gi[:, t], e_gi[:, t] = _sig(a[:, :NH], e_a[:, :NH])
        gf[:, t], e_gf[:, t] = _sig(a[:, NH:2 * NH], e_a[:, NH:2 * NH])
        gg[:, t], e_gg[:, t] = _tanh(a[:, 2 * NH:3 * NH], e_a[:, 2 * NH:3 * NH])
        go[:, t], e_go[:, t] = _sig(a[:, 3 * NH:], e_a[:, 3 * NH:])
        ig, e_ig = _mul(gi[:, t], e_gi[:, t], gg[:, t], e_gg[:, t])
        c[:, t] = gf[:, t] * cp + ig
        e_c[:, t] = e_gf[:, t] * np.abs(cp) + gf[:, t] * e_cp + e_ig + U * np.abs(c[:, t])
        tc, e_tc = _tanh(c[:, t], e_c[:, t])
        h[:, t], e_h[:, t] = _mul(go[:, t], e_go[:, t], tc, e_tc)
        hp, e_hp, cp, e_cp = h[:, t], e_h[:, t], c[:, t], e_c[:, t]
    out = dict(h=h, e_h=e_h, gf=gf)
    if dY is None:
        return out

    dG, e_dG = z3(NG), z3(NG)
    rec, e_rec, dc, e_dc = (np.zeros((N, NH)) for _ in range(4))
    for t in range(TS - 1, -1, -1):
        dh = dY[:, t] + rec
        e_dh = edY[:, t] + e_rec + U * np.abs(dh)
        tc, e_tc = _tanh(c[:, t], e_c[:, t])
        if t > 0:
            cprev, e_cprev = c[:, t - 1], e_c[:, t - 1]
        elif flaw == "c_init":
            cprev, e_cprev = c[:, t], e_c[:, t]
        else:
            cprev, e_cprev = np.zeros((N, NH)), np.zeros((N, NH))
        i_, f_, g_, o_ = gi[:, t], gf[:, t], gg[:, t], go[:, t]
        ei, ef, eg, eo = e_gi[:, t], e_gf[:, t], e_gg[:, t], e_go[:, t]
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
        if flaw == "no_tanh_prime_g":
            d_g, e_dg = q, e_q
        else:
            gp, e_gp = _one_minus_sq(g_, eg)
            d_g, e_dg = _mul(q, e_q, gp, e_gp)
        dG[:, t] = np.concatenate([d_i, d_f, d_g, d_o], 1)
        e_dG[:, t] = np.concatenate([e_di, e_df, e_dg, e_do], 1)
        if flaw == "no_dc_carry":
            dc, e_dc = np.zeros((N, NH)), np.zeros((N, NH))
        else:
            dc, e_dc = _mul(d, e_d, f_, ef)
        if flaw == "no_rec_term":
            continue
        g_t, eg_t = dG[:, t], e_dG[:, t]
        rec = g_t @ Whh
        e_rec = np.sqrt((eg_t * eg_t) @ W2 + (g_t * g_t) @ eW2 + (np.sqrt(NG + 1) * U * (np.abs(g_t) @ aW)) ** 2)
    hprev, e_hprev = np.zeros_like(h), np.zeros_like(h)
    if flaw == "dwhh_h_t":
        hprev, e_hprev = h, e_h
    else:
        hprev[:, 1:], e_hprev[:, 1:] = h[:, :-1], e_h[:, :-1]
    Gf, eGf, aGf = dG.reshape(rows, NG), e_dG.reshape(rows, NG), np.abs(dG).reshape(rows, NG)
    Hf, eHf = hprev.reshape(rows, NH), e_hprev.reshape(rows, NH)
    out.update(dG=dG, e_dG=e_dG,
               dWih=Gf.T @ Xf, e_dWih=eGf.T @ np.abs(Xf) + aGf.T @ eXf + np.sqrt(rows + 1) * U * (aGf.T @ np.abs(Xf)),
               dWhh=Gf.T @ Hf, e_dWhh=eGf.T @ np.abs(Hf) + aGf.T @ eHf + np.sqrt(rows + 1) * U * (aGf.T @ np.abs(Hf)))
    if pieces:
        out["pieces"] = dict(dG=dG, e_dG=e_dG, X=X, e_X=eX, hprev=hprev, e_hprev=e_hprev)      # in this direction's step order
    return out


_IFOG = np.r_[0:2 * NH, 3 * NH:4 * NH, 2 * NH:3 * NH]          # an involution of the gate rows


def run(layer, params, X, dY=None, dparams=None, flaw=None, kX=None, kdY=None, want_dX=True, pieces=False):
    """float32 inputs -> dict: Y, dX, grads {name: array} in float64 and their kappas k_Y, k_dX, k_grads; mean_f, the mean forget
    gate.  dY None: forward only.  pieces: also `pieces`, per direction the operands of dW_ih and dW_hh (dG, X, h_{t-1} and their
    sigmas, frame by frame; tests/bigbatch_ref64.py sums them with other frame weights)."""
    assert flaw is None or flaw in FLAWS, flaw
    X = _f64(X)
    N, I = X.shape[0], IN_DIM[layer]
    assert X.shape == (N, TS, I), X.shape
    nm = names(layer)
    W = [_f64(params[n]) for n in nm]
    eW = [_f64(dparams[n]) / LAMBDA if dparams else np.zeros_like(w) for n, w in zip(nm, W)]            # kappa in, sigma inside
    if flaw == "gates_ifog":
        W, eW = [w[_IFOG] for w in W], [e[_IFOG] for e in eW]
    eX = np.zeros_like(X) if kX is None else _f64(kX) / LAMBDA
    if dY is not None:
        dY = _f64(dY)
        edY = np.zeros_like(dY) if kdY is None else _f64(kdY) / LAMBDA
    res = []
    for d in (0, 1):
        flip = d == 1 and flaw != "reverse_forward"
        tr = (lambda a: a[:, ::-1]) if flip else (lambda a: a)
        sl = slice(d * NH, (d + 1) * NH)
        r = _direction(tr(X), tr(eX), W[d], eW[d], W[2 + d], eW[2 + d], None if dY is None else tr(dY[:, :, sl]),
                       None if dY is None else tr(edY[:, :, sl]), flaw, pieces)
        for k in ("h", "e_h", "gf", "dG", "e_dG"):
            if k in r:
                r[k] = tr(r[k])
        res.append(r)
    Y = np.concatenate([res[0]["h"], res[1]["h"]], 2)
    out = dict(Y=Y, k_Y=LAMBDA * np.concatenate([res[0]["e_h"], res[1]["e_h"]], 2), mean_f=float(np.mean([r["gf"].mean() for r in res])))
    if dY is None:
        return out
    grads, kg = {}, {}
    for d in (0, 1):
        for n, v, e in ((nm[d], "dWih", "e_dWih"), (nm[2 + d], "dWhh", "e_dWhh")):
            g, k = res[d][v], LAMBDA * res[d][e]
            if flaw == "gates_ifog":
                g, k = g[_IFOG], k[_IFOG]
            grads[n], kg[n] = g, k
    out.update(grads=grads, k_grads=kg)
    if pieces:
        out["pieces"] = [r["pieces"] for r in res]
    if want_dX:
        rows = N * TS
        G = [r["dG"].reshape(rows, NG) for r in res]
        eG = [r["e_dG"].reshape(rows, NG) for r in res]
        dX = G[0] @ W[0] + G[1] @ W[1]
        q = sum((eG[d] * eG[d]) @ (W[d] * W[d]) + (G[d] * G[d]) @ (eW[d] * eW[d]) for d in (0, 1))
        e_dX = np.sqrt(q + (np.sqrt(2 * NG + 1) * U * (np.abs(G[0]) @ np.abs(W[0]) + np.abs(G[1]) @ np.abs(W[1]))) ** 2)
        out.update(dX=dX.reshape(N, TS, I), k_dX=LAMBDA * e_dX.reshape(N, TS, I))
    return out


def stack(params, X, dY=None, dparams=None, flaw=None, p=0.0, mask=None):
    """The two-layer stack, layer 0's Y (times `mask` / (1 - p) where given: nn.LSTM's inter-layer dropout) feeding layer 1:
    -> dict H, k_H, dX0, k_dX0, grads, k_grads (both layers' tensors), and the two layers' runs r0, r1."""
    r0 = run(0, params, X, dparams=dparams, flaw=flaw)
    keep = 1.0 if mask is None else _f64(mask) / (1.0 - p)
    r1 = run(1, params, r0["Y"] * keep, dY, dparams=dparams, flaw=flaw, kX=r0["k_Y"] * keep)
    out = dict(H=r1["Y"], k_H=r1["k_Y"], r0=r0, r1=r1)
    if dY is None:
        return out
    b0 = run(0, params, X, r1["dX"] * keep, dparams=dparams, flaw=flaw, kdY=r1["k_dX"] * keep)
    out.update(dX0=b0["dX"], k_dX0=b0["k_dX"], grads={**b0["grads"], **r1["grads"]}, k_grads={**b0["k_grads"], **r1["k_grads"]}, r0=b0)
    return out


def train_steps(c, steps, flaw=None, lr=1e-4):
    """`steps` full steps on the case `c` (the same batch every step; a one-layer case of `case` or a two-layer one of
    `stack_case`) in float64, the errors carried from step to step:
    -> (params, exp_avg, exp_avg_sq, k_params, k_exp_avg, k_exp_avg_sq, first step's run, which also carries the parameters
    after that step as params1, k_params1)."""
    if "layer" not in c:
        return _steps(c, steps, flaw, lr, lambda p, ep: stack(p, c["X"], c["dY"], dparams=ep, flaw=flaw))
    return _steps(c, steps, flaw, lr, lambda p, ep: run(c["layer"], p, c["X"], c["dY"], dparams=ep, flaw=flaw))


def _steps(c, steps, flaw, lr, once):
    nm = list(c["params"])
    p = {n: _f64(c["params"][n]) for n in nm}
    m = {n: np.zeros_like(p[n]) for n in nm}
    v = {n: np.zeros_like(p[n]) for n in nm}
    ep = {n: np.zeros_like(p[n]) for n in nm}
    em = {n: np.zeros_like(p[n]) for n in nm}
    ev = {n: np.zeros_like(p[n]) for n in nm}
    first = None
    for t in range(1, steps + 1):
        r = once(p, ep)
        first = first or r
        for n in nm:
            p[n], m[n], v[n], ep[n], em[n], ev[n] = adam(p[n], r["grads"][n], m[n], v[n], t, lr=lr, ep=ep[n], eg=r["k_grads"][n],
                                                         em=em[n], ev=ev[n], flaw=flaw)
        if t == 1:
            first["params1"], first["k_params1"] = dict(p), dict(ep)      # the state after the first step
    return p, m, v, ep, em, ev, first


def loss(layer, params, X, dY):
    """the scalar whose gradients `run` states: (Y * dY).sum()"""
    return float((run(layer, params, X)["Y"] * _f64(dY)).sum())


def stack_loss(params, X, dY):
    """the scalar whose gradients `stack` states: (H * dY).sum()"""
    return float((stack(params, X)["H"] * _f64(dY)).sum())
