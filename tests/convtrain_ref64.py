"""Float64 restatement of the conv stack's training step (include/sdfa_convtrain.h) on R columns, for any R: the weight-norm fold,
three convolutions along frequency with LeakyReLU(0.2), the inference-form BatchNorm (running statistics, eps 1e-3) and two
max-pools, the analytic backward from dC (dbeta, dgamma, db, dW, dX, the weight norm), and torch.optim.Adam -- each value with a
propagated first-order error scale kappa for the float32 operations the device forms it with.  kappa is built by the rules of
tests/headtrain_ref64.py, which derives them; LAMBDA, U, SLOPE32, adam, the fold (_Layer), weight_norm_backward and the lrelu rule
are imported from it.  What is particular here:

    conv        a[f][co] is one chain of K = ci kf products and the bias: sqrt(K + 2) U (sum |x w| + |b|), incoming errors in
                quadrature.  A row whose products are all zero is b itself: no operation rounds, the error is the bias's own.
    BatchNorm   the device's form: rstd = 1 / sqrtf(var + eps) (U for the sum, 2 U each for sqrtf and the division), s = gamma rstd
                (U), t = fma(-mean, s, beta) (U), z = fma(y, s, t) (U).  eps is the float32 constant (EPS32); the reference's
                double run uses 1e-3.
    dgamma      the device's order: q = dz ((y - mean) rstd) elementwise, three operations, then the sum.
    rows        db, dbeta, dgamma and dW contract over the columns and the layer's frequency rows: incoming errors are added
                linearly, the summation sqrt(n + 1) U sum |a b| for any order, which covers the row-block partials.
    dX          one chain of kf co products.

The two non-smooth points:

    kink        headtrain_ref64's rule: where |a| <= LAMBDA sigma(a) the side the device saw is not known, the backward factor may
                be 1 or 0.2 and kappa takes the whole difference (counted in `ambiguous_kink`).  a == 0 with zero error is decided:
                slope 0.2, as torch has it.
    pool route  the two rows of a pair share s and t, so only what is particular to a row can turn the comparison: its error of a,
                the roundings of lrelu and of the fma, and the pair's difference of y times the error of s.  Where |z0 - z1| is
                within LAMBDA times that, the route is ambiguous: kappa of dz takes the whole |dp| on both rows and the element
                is counted (`ambiguous_pool`).  Equal values with zero error of that kind are decided, the first row: a scale
                of exactly zero makes both rows t itself.  So is a pair whose two rows are the same operations on the same
                numbers -- equal operand windows, value for value and error for error: their a are equal on the device whatever
                the roundings were (`ties` counts both kinds).  Layer 1's windows have zero error, so there this is "equal values
                with zero error"; deeper layers inherit it from equal windows below.

`flaw` builds deliberately wrong models, the controls: see FLAWS."""
import numpy as np

from headtrain_ref64 import LAMBDA, SLOPE32, U, _Layer, adam, weight_norm_backward

FLAWS = ("tie_second", "both_rows", "larger_acc", "lrelu1", "slope1_at0", "pad_wrap", "pad_clamp", "taps_reversed", "dx_untransposed",
         "dgamma_no_mean", "no_dbeta", "no_proj", "no_bias_correction")
FAMILIES = ("default", "edge")
COLS, BINS, IN, OUT_BINS, OUT = 64, 128, 3, 32, 64
LAYERS = ((1, 32, 3, 3, True), (3, 64, 32, 3, True), (5, 64, 64, 1, False))      # (index, co, ci, kf, pooled)
P = "_audio_encoder._layers."
EPS32 = float(np.float32(1e-3))
TRAINABLE = ("weight_g", "weight_v", "bias", "_ext_post_bn.weight", "_ext_post_bn.bias")
CONSTANT = ("_ext_post_bn.running_mean", "_ext_post_bn.running_var")


def names():
    """the 15 trainable tensors in the order of the device's flat buffers"""
    return tuple(f"{P}{L}.{k}" for L, *_ in LAYERS for k in TRAINABLE)


def constant_names():
    return tuple(f"{P}{L}.{k}" for L, *_ in LAYERS for k in CONSTANT)


def shapes():
    out = {}
    for L, co, ci, kf, _ in LAYERS:
        out.update({f"{P}{L}.weight_g": (co, 1, 1, 1), f"{P}{L}.weight_v": (co, ci, kf, 1)})
        out.update({f"{P}{L}.{k}": (co,) for k in TRAINABLE[2:] + CONSTANT})
    return out


def case(R, seed, family="default"):
    """Seeded float32 inputs of R columns: params (trainable and constant tensors), feat [R][128][3], dC [R][32][64].
    "default": kaiming-scale v, g = ||v|| uniform(0.8, 1.2), bias N(0, 0.05), BatchNorm weight uniform(0.5, 1.5), bias N(0, 0.1),
    running_mean N(0.1, 0.1), running_var uniform(0.05, 0.5): what a trained checkpoint holds after lrelu; features N(0, 1) times a
    per-channel scale (1, 0.5, 0.25), the scale of train_batch's normalised mel and its two deltas.
    "edge": about a fifth of every layer's BatchNorm weights negative and one of layers 1 and 3 exactly zero (a dead channel: every
    pair of it ties on different rows, the one tie whose route the parameter gradients can see -- dgamma; between equal rows
    either route gives the same sums); column 0 all zero (exact ties through the stack); layer 1's channels 0 .. 7 with zero bias
    (a == 0 exactly in that column); column 1 constant along frequency (only the padded borders differ); layer 3's
    running_var[0] = 1e-4; the other columns' energy concentrated in bins 0, 1, 126 and 127 (ten times the rest).
    dC = (gaussian + 1) / R: a common component, as a loss gradient has."""
    assert family in FAMILIES, family
    rs = np.random.RandomState(seed)
    f32 = np.float32
    params = {}
    for L, co, ci, kf, _ in LAYERS:
        n = f"{P}{L}."
        v = rs.normal(0, np.sqrt(2.0 / (ci * kf)), (co, ci, kf, 1)).astype(f32)
        nrm = np.sqrt((v.astype(np.float64) ** 2).reshape(co, -1).sum(1))
        params[n + "weight_g"] = (nrm * rs.uniform(0.8, 1.2, co)).astype(f32).reshape(co, 1, 1, 1)
        params[n + "weight_v"] = v
        params[n + "bias"] = rs.normal(0, 0.05, co).astype(f32)
        params[n + "_ext_post_bn.weight"] = rs.uniform(0.5, 1.5, co).astype(f32)
        params[n + "_ext_post_bn.bias"] = rs.normal(0, 0.1, co).astype(f32)
        params[n + "_ext_post_bn.running_mean"] = rs.normal(0.1, 0.1, co).astype(f32)
        params[n + "_ext_post_bn.running_var"] = rs.uniform(0.05, 0.5, co).astype(f32)
    feat = (rs.normal(0, 1, (R, BINS, IN)) * np.array([1.0, 0.5, 0.25])).astype(f32)
    if family == "edge":
        for L, co, *_ in LAYERS:
            neg = rs.permutation(co)[:max(1, co // 5)]
            params[f"{P}{L}._ext_post_bn.weight"][neg] *= f32(-1)
        params[f"{P}1.bias"][:8] = 0
        params[f"{P}1._ext_post_bn.weight"][8] = 0
        params[f"{P}3._ext_post_bn.weight"][1] = 0
        params[f"{P}3._ext_post_bn.running_var"][0] = f32(1e-4)
        feat[:, 2:126] *= f32(0.1)
        feat[0] = 0
        if R > 1:
            feat[1] = rs.normal(0, 1, (1, IN)).astype(f32)
    dC = ((rs.normal(0, 1, (R, OUT_BINS, OUT)) + 1.0) / R).astype(f32)
    return dict(family=family, params=params, feat=feat, dC=dC)


# Seeded features for a checkpoint's own tensors: (R, seed) of the "default" family's features, which the operator tests put in
# front of the synthetic checkpoint (tests/test_gpu_conv_train_op.py) and the CPU test holds under the ambiguity cap.
CHECKPOINT_CASES = {"forward": (12 * COLS, 91), "train_step": (6 * COLS, 92)}
AMBIGUOUS_CAP = 1e-3


def checkpoint_case(state_dict, which):
    """(params of the conv stack taken from `state_dict`, names with or without "_model.", feat [R][128][3]) of CHECKPOINT_CASES"""
    rows, seed = CHECKPOINT_CASES[which]
    take = lambda n: np.asarray(state_dict["_model." + n] if "_model." + n in state_dict else state_dict[n], np.float32)
    return {n: take(n) for n in names() + constant_names()}, case(rows, seed, "default")["feat"]


def under_cap(r):
    """the ambiguous elements of either kind are at most AMBIGUOUS_CAP of each layer's elements"""
    return all(max(r["ambiguous_kink"][L], r["ambiguous_pool"][L]) <= AMBIGUOUS_CAP * n for L, n in r["elements"].items())


def _f64(a):
    return np.asarray(a, np.float64)


def _src(F, kf, d, pad):
    """row f of tap d reads row src[f]; ok[f]: it is inside the column (zero padding) -- the controls wrap or clamp instead"""
    s = np.arange(F) + d - kf // 2
    ok = (s >= 0) & (s < F)
    if pad == "wrap":
        return s % F, np.ones(F, bool)
    if pad == "clamp":
        return np.clip(s, 0, F - 1), np.ones(F, bool)
    return np.clip(s, 0, F - 1), ok


def _windows(X, kf, pad):
    """[R][F][ci] -> [R][F][ci kf]: v's own order, ci outer, tap inner"""
    R, F, ci = X.shape
    out = np.zeros((R, F, ci, kf))
    for d in range(kf):
        s, ok = _src(F, kf, d, pad)
        out[:, :, :, d] = X[:, s, :] * ok[None, :, None]
    return out.reshape(R, F, ci * kf)


def _unwindow(D, ci, kf, pad):
    """the transpose of _windows: [R][F][ci kf] -> [R][F][ci]"""
    R, F, _ = D.shape
    D = D.reshape(R, F, ci, kf)
    out = np.zeros((R, F, ci))
    for d in range(kf):
        s, ok = _src(F, kf, d, pad)
        for f in range(F):
            if ok[f]:
                out[:, s[f], :] += D[:, f, :, d]
    return out


class _Conv:
    """a layer's fold: headtrain_ref64's weight norm over v as [co][ci kf], and the BatchNorm's s, t, rstd with their sigmas"""

    def __init__(self, spec, params, dparams, eps):
        L, co, ci, kf, pooled = spec
        n = f"{P}{L}"
        self.n, self.co, self.ci, self.kf, self.pooled, self.K = n, co, ci, kf, pooled, ci * kf
        as2d = lambda d: {n + ".weight_g": d[n + ".weight_g"], n + ".weight_v": _f64(d[n + ".weight_v"]).reshape(co, -1), n + ".bias": d[n + ".bias"]}
        self.f = _Layer(dict(name=n, K=self.K), as2d(params), as2d(dparams) if dparams else None)
        sig = lambda k: _f64(dparams[n + k]) / LAMBDA if dparams else np.zeros(co)
        gam, bet = _f64(params[n + "._ext_post_bn.weight"]), _f64(params[n + "._ext_post_bn.bias"])
        self.mean, var = _f64(params[n + "._ext_post_bn.running_mean"]), _f64(params[n + "._ext_post_bn.running_var"])
        self.rstd = 1.0 / np.sqrt(var + eps)
        self.erstd = 4.5 * U * self.rstd                     # U (var + eps) halves through the root; sqrtf and the division 2 U each
        self.s = gam * self.rstd
        self.es = np.abs(gam) * self.erstd + sig("._ext_post_bn.weight") * self.rstd + U * np.abs(self.s)
        self.t = bet - self.mean * self.s
        self.et = sig("._ext_post_bn.bias") + np.abs(self.mean) * self.es + U * np.abs(self.t)


def run(params, feat, dC=None, dparams=None, flaw=None, slope=SLOPE32, eps=EPS32, kdC=None):
    """float32 inputs -> dict: C [R][32][64], grads {name: array} in float64, their kappas k_C and k_grads, and per layer the
    counts `ambiguous_kink`, `ambiguous_pool`, `ties` (decided exact ties) and `elements` ({layer index: int}).  dC None: forward
    only; kdC: the kappa dC comes with (the frequency LSTM's k_dC).  Also `dW` {layer: [co][ci kf]} and `winner` {layer: bool [R][F/2][co], True where the second row won}."""
    assert flaw is None or flaw in FLAWS, flaw
    pad = "wrap" if flaw == "pad_wrap" else "clamp" if flaw == "pad_clamp" else "zero"
    neg = 1.0 if flaw == "lrelu1" else slope
    X, eX = _f64(feat), np.zeros(np.shape(feat))
    R = len(X)
    convs = [_Conv(s, params, dparams, eps) for s in LAYERS]
    kept, counts = [], dict(ambiguous_kink={}, ambiguous_pool={}, ties={}, elements={})
    for c in convs:
        f = c.f
        Xw, eXw = _windows(X, c.kf, pad), _windows(eX, c.kf, pad)
        a = Xw @ f.W.T + f.b
        prod = np.abs(Xw) @ np.abs(f.W).T
        e2 = (eXw * eXw) @ (f.W * f.W).T + (Xw * Xw) @ (f.eW * f.eW).T + f.eb * f.eb
        e = np.sqrt(e2 + np.where(prod > 0, np.sqrt(c.K + 2) * U * (prod + np.abs(f.b)), 0.0) ** 2)
        y = np.where(a >= 0, a, neg * a)
        ey = e + U * np.abs(y)
        kink = (np.abs(a) <= LAMBDA * e) & ~((a == 0) & (e == 0))
        z = y * c.s + c.t
        rz = np.where(y * c.s != 0, U * np.abs(z), 0.0)       # fma(y, s, t) is t itself where the product is zero
        ez = ey * np.abs(c.s) + np.abs(y) * c.es + c.et + rz
        L = int(c.n.rsplit(".", 1)[1])
        counts["ambiguous_kink"][L] = int(kink.sum())
        counts["elements"][L] = int(a.size)
        k = dict(c=c, Xw=Xw, eXw=eXw, a=a, y=y, ey=ey, kink=kink)
        if c.pooled:
            z0, z1, a0, a1 = z[:, 0::2], z[:, 1::2], a[:, 0::2], a[:, 1::2]
            row = ey * np.abs(c.s) + rz                       # what is particular to a row
            pair = row[:, 0::2] + row[:, 1::2] + np.abs(y[:, 0::2] - y[:, 1::2]) * c.es
            same = ((Xw[:, 0::2] == Xw[:, 1::2]) & (eXw[:, 0::2] == eXw[:, 1::2])).all(2)[:, :, None] | ((z0 == z1) & (pair == 0))
            amb = (np.abs(z0 - z1) <= LAMBDA * pair) & ~same
            if flaw == "larger_acc":
                second = a1 > a0
            elif flaw == "tie_second":
                second = z1 >= z0
            else:
                second = z1 > z0
            X = np.where(second, z1, z0)
            eX = np.where(amb, np.maximum(ez[:, 0::2], ez[:, 1::2]), np.where(second, ez[:, 1::2], ez[:, 0::2]))
            counts["ambiguous_pool"][L] = int(amb.sum())
            counts["ties"][L] = int((same & (z0 == z1)).sum())
            k.update(second=second, amb=amb)
        else:
            X, eX = z, ez
            counts["ambiguous_pool"][L] = 0
            counts["ties"][L] = 0
        kept.append(k)
    out = dict(C=X, k_C=LAMBDA * eX, **counts)
    out["winner"] = {int(k["c"].n.rsplit(".", 1)[1]): k["second"] for k in kept if k["c"].pooled}
    if dC is None:
        return out

    grads, k_grads, dWs = {}, {}, {}
    dp, edp = _f64(dC), np.zeros(np.shape(dC)) if kdC is None else _f64(kdC) / LAMBDA
    for k in reversed(kept):
        c, f, a, y, ey = k["c"], k["c"].f, k["a"], k["y"], k["ey"]
        n = c.n
        if c.pooled:
            second, amb = k["second"], k["amb"]
            dz, edz = np.zeros_like(a), np.zeros_like(a)
            w0 = np.ones_like(second) if flaw == "both_rows" else ~second
            w1 = np.ones_like(second) if flaw == "both_rows" else second
            dz[:, 0::2], dz[:, 1::2] = dp * w0, dp * w1
            whole = np.where(amb, np.abs(dp) / LAMBDA, 0.0)
            edz[:, 0::2] = np.where(amb | w0, edp, 0.0) + whole
            edz[:, 1::2] = np.where(amb | w1, edp, 0.0) + whole
            nz = dp.size / c.co                               # terms of a channel's dbeta and dgamma: the pooled positions
        else:
            dz, edz, nz = dp, edp, dp.size / c.co
        na = a.size / c.co
        ax = (0, 1)
        grads[n + "._ext_post_bn.bias"] = np.zeros(c.co) if flaw == "no_dbeta" else dz.sum(ax)
        k_grads[n + "._ext_post_bn.bias"] = LAMBDA * (edz.sum(ax) + np.sqrt(nz + 1) * U * np.abs(dz).sum(ax))
        cen = y if flaw == "dgamma_no_mean" else y - c.mean
        xh = cen * c.rstd
        exh = (ey + U * np.abs(cen)) * c.rstd + np.abs(cen) * c.erstd + U * np.abs(xh)
        q = dz * xh
        eq = edz * np.abs(xh) + np.abs(dz) * exh + U * np.abs(q)
        grads[n + "._ext_post_bn.weight"] = q.sum(ax)
        k_grads[n + "._ext_post_bn.weight"] = LAMBDA * (eq.sum(ax) + np.sqrt(nz + 1) * U * np.abs(q).sum(ax))
        fac = np.where((a >= 0) if flaw == "slope1_at0" else (a > 0), 1.0, neg)
        da = dz * c.s * fac
        eda = (edz * np.abs(c.s) + np.abs(dz) * c.es) * np.where(k["kink"], 1.0, fac) + 2 * U * np.abs(da) \
            + np.where(k["kink"], (1.0 - neg) * np.abs(dz * c.s) / LAMBDA, 0.0)
        grads[n + ".bias"] = da.sum(ax)
        k_grads[n + ".bias"] = LAMBDA * (eda.sum(ax) + np.sqrt(na + 1) * U * np.abs(da).sum(ax))
        D, eD = da.reshape(-1, c.co), eda.reshape(-1, c.co)
        Xw, eXw = k["Xw"].reshape(-1, c.K), k["eXw"].reshape(-1, c.K)
        dW = D.T @ Xw
        edW = eD.T @ np.abs(Xw) + np.abs(D).T @ eXw + np.sqrt(na + 1) * U * (np.abs(D).T @ np.abs(Xw))
        if flaw == "taps_reversed":
            dW = dW.reshape(c.co, c.ci, c.kf)[:, :, ::-1].reshape(c.co, c.K)
        dWs[int(n.rsplit(".", 1)[1])] = dW
        dg, kdg, dv, kdv = weight_norm_backward(f, c.K, dW, edW, flaw)
        grads[n + ".weight_g"], k_grads[n + ".weight_g"] = dg.reshape(c.co, 1, 1, 1), kdg.reshape(c.co, 1, 1, 1)
        grads[n + ".weight_v"], k_grads[n + ".weight_v"] = dv.reshape(c.co, c.ci, c.kf, 1), kdv.reshape(c.co, c.ci, c.kf, 1)
        if c.ci == IN:
            break
        Wd = f.W
        if flaw == "dx_untransposed":
            Wd = Wd.reshape(c.co, c.ci, c.kf)[:, :, ::-1].reshape(c.co, c.K)
        dp = _unwindow(da @ Wd, c.ci, c.kf, pad)
        e2 = _unwindow((eda * eda) @ (f.W * f.W) + (da * da) @ (f.eW * f.eW), c.ci, c.kf, pad)
        mag = _unwindow(np.abs(da) @ np.abs(f.W), c.ci, c.kf, pad)
        edp = np.sqrt(e2 + (np.sqrt(c.kf * c.co + 1) * U * mag) ** 2)
    out.update(grads=grads, k_grads=k_grads, dW=dWs)
    return out


def train_steps(c, steps, flaw=None, lr=1e-4, slope=SLOPE32, eps=EPS32):
    """`steps` full steps on the case `c` (the same batch every step) in float64, the errors carried from step to step:
    -> (params, exp_avg, exp_avg_sq, k_params, k_exp_avg, k_exp_avg_sq, first step's run).  The constants ride in params unchanged."""
    tn = names()
    p = {n: _f64(v) for n, v in c["params"].items()}
    m = {n: np.zeros_like(p[n]) for n in tn}
    v = {n: np.zeros_like(p[n]) for n in tn}
    ep = {n: np.zeros_like(p[n]) for n in tn}
    em = {n: np.zeros_like(p[n]) for n in tn}
    ev = {n: np.zeros_like(p[n]) for n in tn}
    first = None
    for t in range(1, steps + 1):
        r = run(p, c["feat"], c["dC"], dparams=ep, flaw=flaw, slope=slope, eps=eps)
        first = first or r
        for n in tn:
            p[n], m[n], v[n], ep[n], em[n], ev[n] = adam(p[n], r["grads"][n], m[n], v[n], t, lr=lr, ep=ep[n], eg=r["k_grads"][n],
                                                         em=em[n], ev=ev[n], flaw=flaw)
    return p, m, v, ep, em, ev, first
