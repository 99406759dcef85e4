"""Float64 restatement of the regressor head's training step (include/sdfa_headtrain.h): the weight-norm fold, the forward,
the analytic backward (weight norm included), dz, and one torch.optim.Adam step -- each value with a propagated first-order
error scale kappa for the float32 operations the device forms it with.  Every factor is an operation count, a published
bound or the constant LAMBDA derived below; none is fitted.  Errors of the inputs (the parameters after an earlier step) enter
through `dparams` and are propagated like the rounding errors, so the scale carries over several steps.

What kappa is.  A worst-case elementwise bound is useless four layers deep: a contraction over k adds sum_k |W_pk| e_k, about 25
times the typical e_k for these layers, at every layer, and (K + 3) U sum |x w| at the first one; at coef it reaches 8.8 times
the coefficient itself and every wrong model below lies inside it (measured on case dgrad_b3 before this form was chosen).
kappa is therefore the high-probability scale of the standard probabilistic model of rounding (N. J. Higham, T. Mary, "A new
approach to probabilistic rounding error analysis", SIAM J. Sci. Comput. 41, 2019): the roundings are independent, mean zero
and bounded by U |x|.  A bounded mean-zero error is sub-gaussian with its bound as parameter (Hoeffding's lemma); a sum of
independent ones with coefficients a_k has parameter sqrt(sum a_k^2 sigma_k^2), and exceeds LAMBDA times it with probability
at most 2 exp(-LAMBDA^2 / 2).  The model propagates the parameters sigma and returns kappa = LAMBDA sigma.

    LAMBDA      8: 2 exp(-32) = 2.5e-14 per element; a test compares fewer than 1e7 elements, so the chance that a correct
                implementation leaves kappa anywhere is below 3e-7.  Not chosen from any measured error.
    sums        n products summed in ANY order: sigma = sqrt(n + 1) U sum |a b| (Higham and Mary's Theorem 3.1 in sigma form).
                A layer's pre-activation (Kin products, the bias, the one-hot column): sqrt(Kin + 3) U (sum |x w| + |b| + |w_col|).
    features    incoming errors of a contraction over features (k or p) are taken as independent: combined in quadrature.
    batch       incoming errors of a contraction over the rows of the batch (dW, db) share the fold's errors of W: they are
                NOT independent and are added linearly.  Elementwise operations add linearly as well.
    fold        ss = sum v^2;  sqrtf and the division: 2 U each (correctly rounded ones need U);  s = g inv, W = s v: U each.
    lrelu       1-Lipschitz: the argument's error, plus U |y| for the product with the float32 constant 0.2f (SLOPE32).  Where
                |pre| <= LAMBDA sigma the SIGN the device saw is not known: the backward factor may be 1 or 0.2 there, and
                kappa takes the whole difference (AMBIGUOUS elements; they are counted in the result).
    tanh        sech^2 at the nearest point of the argument's interval times the argument's error, plus K_TANH U |y|.
    tanh'       f = fma(-y, y, 1): 2 |y| dy + 2 U;  the product with dX: U.
    weight norm dot = <dW, v>;  dg = dot inv, c = dg inv, t = dW - c v, dv = s t: one U per operation.
    Adam        the constants (1 - beta1, beta2, 1 - beta2, eps, lr / bc1, sqrt(bc2)) are float32 roundings of the doubles the
                host forms: U each;  |sqrt a - sqrt b| <= |a - b| / sqrt a;  the quotient's denominator is taken at the low end
                of its interval.  An element with g = m = v = 0 and no incoming error has kappa 0: it must keep its bits.

Both checks the model must pass are in tests/test_headtrain_ref64_cpu.py: the reference's own float32 run lies within
1 x kappa (not too small), every wrong model lies more than 100 x kappa away somewhere (not too loose).

`flaw` builds deliberately wrong models, the controls: "no_proj" (the projection term of dv dropped), "lrelu1" (slope 1 on the
negative side), "no_rotat" (the rotat branch's share of dh0 omitted), "wrong_speaker" (the one-hot column of speaker + 1),
"no_bias_correction" (Adam)."""
import numpy as np

U = 2.0 ** -24
LAMBDA = 8.0
# Twice the ulp bound of the device's tanhf.  HIP's math API documentation (docs/reference/math_api, "Single precision
# mathematical functions") lists tanhf with a maximum error of 2 ULP; 1 ulp of a value v is at most 2 U |v|.  As for expf
# (score_ref64.K_EXP) the value stands on the published table: the installation ships no copy of it.
K_TANH = 4.0
SLOPE32 = float(np.float32(0.2))         # the device's constant; the reference's double run uses 0.2
FLAWS = ("no_proj", "lrelu1", "no_rotat", "wrong_speaker", "no_bias_correction")

_BRANCH = ((512, 520, 512, 1, "lrelu"), (256, 512, 512, 0, "tanh"), (None, 256, 256, 0, "linear"))


def layers_of(head):
    """[dict(name, P, K, Kin, cond, act)]: the trunk (dgrad only), then each branch's three layers."""
    o = "_output_module."
    out = []
    if head == "dgrad":
        out.append(dict(name=o + "_layers.0", P=512, K=520, Kin=512, cond=1, act="lrelu"))
        for br, nco in (("_scale", 85), ("_rotat", 180)):
            out += [dict(name=f"{o}{br}_layers.{i}", P=p or nco, K=k, Kin=kin, cond=c, act=a) for i, (p, k, kin, c, a) in enumerate(_BRANCH)]
    else:
        out += [dict(name=f"{o}_layers.{i}", P=p or 59, K=k, Kin=kin, cond=c, act=a) for i, (p, k, kin, c, a) in enumerate(_BRANCH)]
    return out


def branches_of(head):
    """(trunk layer or None, [[three layers] per branch])"""
    ls = layers_of(head)
    return (ls[0], [ls[1:4], ls[4:7]]) if head == "dgrad" else (None, [ls])


def case(head, B, seed, speakers=tuple(range(8))):
    """Seeded float32 inputs of a batch of N = 2 B rows: weight-normed layers as the synthetic checkpoints have them
    (v ~ N(0, gain / fan_in), g = ||v|| uniform(0.8, 1.2), bias ~ N(0, 0.05)), z ~ N(0, 0.5), speaker ids drawn from
    `speakers`, dcoef ~ N(0, 1) / N."""
    rs = np.random.RandomState(seed)
    f32 = np.float32
    params = {}
    for L in layers_of(head):
        gain = 2.0 if L["K"] == 520 else 1.0
        v = rs.normal(0, np.sqrt(gain / L["K"]), (L["P"], L["K"])).astype(f32)
        g = (np.sqrt((v.astype(np.float64) ** 2).sum(1)) * rs.uniform(0.8, 1.2, L["P"])).astype(f32)
        params[L["name"] + ".weight_g"] = g.reshape(-1, 1)
        params[L["name"] + ".weight_v"] = v
        params[L["name"] + ".bias"] = rs.normal(0, 0.05, L["P"]).astype(f32)
    N = 2 * B
    Kc = 265 if head == "dgrad" else 59
    z = rs.normal(0, 0.5, (N, 512)).astype(f32)
    sid = np.asarray(speakers, np.int64)[rs.randint(0, len(speakers), N)]
    dcoef = (rs.normal(0, 1, (N, Kc)) / N).astype(f32)
    return dict(head=head, params=params, z=z, sid=sid, dcoef=dcoef)


def _f64(a):
    return np.asarray(a, np.float64)


class _Layer:
    """One layer's fold in float64 with its error parameters (sigma, not kappa)."""

    def __init__(self, L, params, dparams):
        n = L["name"]
        self.L = L
        self.g, self.v, self.b = _f64(params[n + ".weight_g"]).reshape(-1), _f64(params[n + ".weight_v"]), _f64(params[n + ".bias"])
        zero = lambda a: np.zeros_like(a)
        self.eg = _f64(dparams[n + ".weight_g"]).reshape(-1) / LAMBDA if dparams else zero(self.g)      # kappa in, sigma inside
        self.ev = _f64(dparams[n + ".weight_v"]) / LAMBDA if dparams else zero(self.v)
        self.eb = _f64(dparams[n + ".bias"]) / LAMBDA if dparams else zero(self.b)
        K = L["K"]
        ss = (self.v * self.v).sum(1)
        nrm = np.sqrt(ss)
        self.inv = 1.0 / nrm
        self.s = self.g * self.inv
        self.W = self.s[:, None] * self.v
        e_ss = 2 * np.sqrt(((self.v * self.ev) ** 2).sum(1)) + np.sqrt(K + 1) * U * ss
        e_nrm = e_ss / (2 * nrm) + 2 * U * nrm
        self.einv = e_nrm / (nrm * nrm) + 2 * U * self.inv
        self.es = np.abs(self.g) * self.einv + self.eg * self.inv + U * np.abs(self.s)
        self.eW = self.es[:, None] * np.abs(self.v) + np.abs(self.s)[:, None] * self.ev + U * np.abs(self.W)


def _onehot(sid, flaw):
    s = (np.asarray(sid, np.int64) + (1 if flaw == "wrong_speaker" else 0)) % 8
    return np.eye(8)[s]


def weight_norm_backward(f, K, dW, edW, flaw=None):
    """dW of the folded weight and its sigma through the weight norm of the fold `f` (a _Layer):
    -> (dg, kappa of dg, dv, kappa of dv), dg as a column."""
    dot = (dW * f.v).sum(1)
    edot = np.sqrt(((edW * f.v) ** 2 + (dW * f.ev) ** 2).sum(1)) + np.sqrt(K + 1) * U * np.abs(dW * f.v).sum(1)
    dg = dot * f.inv
    edg = edot * f.inv + np.abs(dot) * f.einv + U * np.abs(dg)
    c = dg * f.inv
    ec = edg * f.inv + np.abs(dg) * f.einv + U * np.abs(c)
    if flaw == "no_proj":
        c = np.zeros_like(c)
    t = dW - c[:, None] * f.v
    et = edW + ec[:, None] * np.abs(f.v) + np.abs(c)[:, None] * f.ev + U * np.abs(c[:, None] * f.v) + U * np.abs(t)
    dv = f.s[:, None] * t
    return dg.reshape(-1, 1), LAMBDA * edg.reshape(-1, 1), dv, LAMBDA * (f.es[:, None] * np.abs(t) + np.abs(f.s)[:, None] * et + U * np.abs(dv))


def run(head, params, z, sid, dcoef=None, dparams=None, flaw=None, slope=SLOPE32, pieces=False):
    """float32 inputs -> dict: coef, dz, grads {name: array} in float64, their kappas k_coef, k_dz, k_grads, and `ambiguous`,
    the number of lrelu outputs whose sign the bound cannot tell.  dcoef None: forward only.  pieces: also `pieces`, per layer
    the operands of its contraction over the rows (dPre, its sigma, the layer's input with the one-hot columns, its sigma), and
    `fold`, the layers' folds (tests/bigbatch_ref64.py sums them with other row weights)."""
    assert flaw is None or flaw in FLAWS, flaw
    z, N = _f64(z), len(z)
    oh = _onehot(sid, flaw)
    trunk, branches = branches_of(head)
    lay = {L["name"]: _Layer(L, params, dparams) for L in layers_of(head)}
    neg = 1.0 if flaw == "lrelu1" else slope
    kept = {}
    ambiguous = 0

    def forward(L, X, eX):
        nonlocal ambiguous
        f = lay[L["name"]]
        Kin = L["Kin"]
        Wk, eWk = f.W[:, :Kin], f.eW[:, :Kin]
        pre = X @ Wk.T + f.b
        mag = np.abs(X) @ np.abs(Wk).T + np.abs(f.b)
        e2 = (eX * eX) @ (Wk * Wk).T + (X * X) @ (eWk * eWk).T + f.eb * f.eb
        if L["cond"]:
            pre = pre + oh @ f.W[:, Kin:].T
            mag = mag + oh @ np.abs(f.W[:, Kin:]).T
            e2 = e2 + oh @ (f.eW[:, Kin:] ** 2).T
        e = np.sqrt(e2 + (np.sqrt(Kin + 3) * U * mag) ** 2)
        if L["act"] == "lrelu":
            y = np.where(pre >= 0, pre, neg * pre)
            ey = e + U * np.abs(y)
            amb = np.abs(pre) <= LAMBDA * e
            ambiguous += int(amb.sum())
        elif L["act"] == "tanh":
            y = np.tanh(pre)
            ey = e / np.cosh(np.maximum(np.abs(pre) - LAMBDA * e, 0.0)) ** 2 + K_TANH * U * np.abs(y)
            amb = None
        else:
            y, ey, amb = pre, e, None
        kept[L["name"]] = (X, eX, y, ey, amb)
        return y, ey

    x, ex = z, np.zeros_like(z)
    if trunk:
        x, ex = forward(trunk, x, ex)
    outs = []
    for br in branches:
        y, ey = x, ex
        for L in br:
            y, ey = forward(L, y, ey)
        outs.append((y, ey))
    out = dict(coef=np.concatenate([o[0] for o in outs], 1), k_coef=LAMBDA * np.concatenate([o[1] for o in outs], 1))
    if dcoef is None:
        out["ambiguous"] = ambiguous
        return out

    grads, k_grads = {}, {}

    def backward(L, D, eD):
        """dPre of layer L -> (dX, its error) with respect to the layer's input; fills the layer's gradients."""
        f = lay[L["name"]]
        n, Kin, K = L["name"], L["Kin"], L["K"]
        X, eX = kept[n][0], kept[n][1]
        aD = np.abs(D)
        grads[n + ".bias"] = D.sum(0)
        k_grads[n + ".bias"] = LAMBDA * (eD.sum(0) + np.sqrt(N + 1) * U * aD.sum(0))
        Xf = np.concatenate((X, oh), 1) if L["cond"] else X
        eXf = np.concatenate((eX, np.zeros_like(oh)), 1) if L["cond"] else eX
        dW = D.T @ Xf
        edW = eD.T @ np.abs(Xf) + aD.T @ eXf + np.sqrt(N + 1) * U * (aD.T @ np.abs(Xf))
        dX = D @ f.W[:, :Kin]
        edX = np.sqrt((eD * eD) @ (f.W[:, :Kin] ** 2) + (D * D) @ (f.eW[:, :Kin] ** 2)
                      + (np.sqrt(L["P"] + 1) * U * (aD @ np.abs(f.W[:, :Kin]))) ** 2)
        grads[n + ".weight_g"], k_grads[n + ".weight_g"], grads[n + ".weight_v"], k_grads[n + ".weight_v"] = weight_norm_backward(f, K, dW, edW, flaw)
        out.setdefault("dW", {})[n] = dW
        if pieces:
            out.setdefault("pieces", {})[n] = (D, eD, Xf, eXf)
        return dX, edX

    def through(L, dX, edX):
        """dX with respect to the OUTPUT of layer L -> dPre of layer L"""
        _, _, y, ey, amb = kept[L["name"]]
        if L["act"] == "lrelu":
            f = np.where(y > 0, 1.0, neg)
            D = dX * f
            eD = edX * np.where(amb, 1.0, f) + U * np.abs(D) + np.where(amb, (1.0 - neg) * np.abs(dX) / LAMBDA, 0.0)
        else:
            f = 1.0 - y * y
            D = dX * f
            eD = edX * f + np.abs(dX) * (2 * np.abs(y) * ey + 2 * U) + U * np.abs(D)
        return D, eD

    D0 = _f64(dcoef)
    col = 0
    shares = []
    for br in branches:
        P = br[2]["P"]
        D, eD = D0[:, col:col + P], np.zeros((N, P))
        col += P
        dX, edX = backward(br[2], D, eD)
        D, eD = through(br[1], dX, edX)
        dX, edX = backward(br[1], D, eD)
        D, eD = through(br[0], dX, edX)
        shares.append(backward(br[0], D, eD))
    if trunk:
        if flaw == "no_rotat":
            dh0, edh0 = shares[0]
        else:
            dh0 = shares[0][0] + shares[1][0]
            edh0 = shares[0][1] + shares[1][1] + U * np.abs(dh0)
        D, eD = through(trunk, dh0, edh0)
        dz, edz = backward(trunk, D, eD)
    else:
        dz, edz = shares[0]
    out.update(dz=dz, k_dz=LAMBDA * edz, grads=grads, k_grads=k_grads, ambiguous=ambiguous)
    if pieces:
        out["fold"] = lay
    return out


def adam(p, g, m, v, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, ep=0.0, eg=0.0, em=0.0, ev=0.0, flaw=None):
    """One torch.optim.Adam step (amsgrad off, weight decay 0) from step t - 1 to t, elementwise in float64, with the
    kappas of the inputs: -> (p, m, v, k_p, k_m, k_v)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    ep, eg, em, ev = (np.broadcast_to(_f64(e), p.shape) / LAMBDA for e in (ep, eg, em, ev))      # kappa in, sigma inside
    bc1, bc2 = (1.0, 1.0) if flaw == "no_bias_correction" else (1.0 - beta1 ** t, 1.0 - beta2 ** t)
    step, bc2s = lr / bc1, np.sqrt(bc2)
    inc = (g - m) * (1.0 - beta1)
    m1 = m + inc
    em1 = em + (eg + em) * (1.0 - beta1) + 3 * U * np.abs(inc) + np.where(inc == 0, 0.0, U * np.abs(m1))
    v1 = beta2 * v + (1.0 - beta2) * g * g
    ev1 = beta2 * ev + 2 * U * beta2 * np.abs(v) + (1.0 - beta2) * (2 * np.abs(g) * eg + 4 * U * g * g) + np.where(g == 0, 0.0, U * np.abs(v1))
    sq = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        esq = np.where(v1 > 0, ev1 / np.where(v1 > 0, sq, 1.0), np.sqrt(LAMBDA * ev1) / LAMBDA) + U * sq
    den = sq / bc2s + eps
    eden = esq / bc2s + 3 * U * sq / bc2s + 2 * U * eps + U * den
    den_lo = np.maximum(den - LAMBDA * eden, 0.5 * eps)
    q = m1 / den
    eq = em1 / den_lo + np.abs(m1) * eden / (den * den_lo) + U * np.abs(q)
    upd = step * q
    p1 = p - upd
    ep1 = ep + step * eq + 3 * U * np.abs(upd) + np.where(upd == 0, 0.0, U * np.abs(p1))
    return p1, m1, v1, LAMBDA * ep1, LAMBDA * em1, LAMBDA * ev1


def train_steps(c, steps, flaw=None, lr=1e-4, slope=SLOPE32):
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
        r = run(c["head"], p, c["z"], c["sid"], c["dcoef"], dparams=ep, flaw=flaw, slope=slope)
        first = first or r
        for n in names:
            p[n], m[n], v[n], ep[n], em[n], ev[n] = adam(p[n], r["grads"][n], m[n], v[n], t, lr=lr, ep=ep[n], eg=r["k_grads"][n],
                                                         em=em[n], ev=ev[n], flaw=flaw)
    return p, m, v, ep, em, ev, first
