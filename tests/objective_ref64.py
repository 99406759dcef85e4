"""Float64 restatement of the training objective (include/sdfa_objective.h): the four losses, the per-row records and the
analytic gradients with respect to the PCA coefficients, each with a propagated error scale kappa for the float32 operations
the device forms it with.  Every factor is derived from the operation count or a published error bound; none is fitted.

    expansion   p^ = fl(means + coef . compT^T), K products accumulated in float32 in some order, split over two
                accumulators that are then added, plus the mean:  |p^ - p| <= (K + 2) U (sum_k |coef compT| + |means|) = xp
    e()         scale / plain: e = p, error xp.  rotat: e = exp(p): exp(p) expm1(xp) for the argument, K_EXP U exp(p + xp)
                for expf itself (score_ref64.K_EXP); the truth's exp errs by K_EXP U exp(t)
    squares     the bound of DESIGN section 12 (score_ref64.records) with those e() errors:  |delta d^2| <= 2 |d| eps + eps^2,
                eps = U (|d| + xp + xt) + xp + xt;  motion: eps = U (|dp| + |dt| + |m| + 2 (xdp + xdt)) + xdp + xdt
    losses      sum_r w_r kappa(rec_r) / (N n), the double accumulation, and U |L| for the single rounding to float32
    g           g = fl(d^ e^(p)) on rotat columns (one more rounding), d^ elsewhere:  |delta g| <= eps (e + xe) + |d| xe + U |g|
    gradients   c sum_col (|delta g| |compT| + C U |g compT|) + U |grad|: C, the length of the contraction, bounds the float32
                accumulation in ANY order (the partials are then added in double and rounded once)

The reference's own float32 route (F.linear, exp, mse_loss, sum, mean, autograd) rounds in places the device does not (the
square, the sums over 6 or 3, over the triangles and over the batch, the chain of scalar factors in backward): ref32_extra_*
count those roundings.  They are reported next to the ratios the tests print and are part of no bound: the float32 fixture and the
torch route on the GPU are held to kappa alone."""
import numpy as np

from score_ref64 import K_EXP, U, U64


def parts_of(bases, layout, W):
    """[(compT, means, coefficient slice, truth columns, exp?)]"""
    if layout == "dgrad":
        j = np.arange(W)
        ks, kr = bases["compT_s"].shape[1], bases["compT_r"].shape[1]
        return [(bases["compT_s"], bases["means_s"], slice(0, ks), j[j % 9 < 6], False),
                (bases["compT_r"], bases["means_r"], slice(ks, ks + kr), j[j % 9 >= 6], True)]
    return [(bases["compT_s"], bases["means_s"], slice(0, bases["compT_s"].shape[1]), np.arange(W), False)]


def half_weights(weight):
    """h_k = fl(weight[k] + weight[B + k]), the float32 sum the reference forms."""
    w = np.asarray(weight, np.float32)
    B = w.shape[0] // 2
    return (w[B:] + w[:B]).astype(np.float64)


def losses64(coef, bases, truth, weight, layout):
    """The four losses (ps, ms, pr, mr) as a float64 function of float64 coefficients: what the finite differences take."""
    coef = np.asarray(coef, np.float64)
    N, W = truth.shape
    B = N // 2
    n = W // 9 if layout == "dgrad" else W
    w, h = np.asarray(weight, np.float64), half_weights(weight)
    out = np.zeros(4)
    for pi, (compT, means, sl, cols, use_exp) in enumerate(parts_of(bases, layout, W)):
        p = coef[:, sl] @ np.asarray(compT, np.float64).T + np.asarray(means, np.float64)
        t = np.asarray(truth, np.float64)[:, cols]
        ep, et = (np.exp(p), np.exp(t)) if use_exp else (p, t)
        out[2 * pi] = (w * ((ep - et) ** 2).sum(1)).sum() / (N * n)
        m = (ep[B:] - ep[:B]) - (et[B:] - et[:B])
        out[2 * pi + 1] = (h * (m ** 2).sum(1)).sum() / (B * n)
    return out


def residuals64(coef, bases, truth, layout):
    """Per basis (e(p), d, m, |compT|) in float64 at float64 coefficients: the predicted e() values [N][C], the position
    residuals [N][C] and the motion residuals [B][C].  What a bound on the distance of two coefficient sets' losses is built from."""
    coef = np.asarray(coef, np.float64)
    N, W = truth.shape
    B = N // 2
    out = []
    for compT, means, sl, cols, use_exp in parts_of(bases, layout, W):
        A = np.asarray(compT, np.float64)
        p = coef[:, sl] @ A.T + np.asarray(means, np.float64)
        t = np.asarray(truth, np.float64)[:, cols]
        ep, et = (np.exp(p), np.exp(t)) if use_exp else (p, t)
        out.append((ep, ep - et, (ep[B:] - ep[:B]) - (et[B:] - et[:B]), np.abs(A)))
    return out


def model(coef, bases, truth, weight, layout):
    """float32 inputs -> dict: loss [4], rec [N][4], grad [2][N][Kc] in float64, their kappas k_loss, k_rec, k_grad, and the
    extra allowances ref32_extra_loss, ref32_extra_grad for the reference's float32 reductions."""
    coef32, truth32 = np.asarray(coef, np.float32), np.asarray(truth, np.float32)
    N, W = truth32.shape
    B = N // 2
    n = W // 9 if layout == "dgrad" else W
    w, h = np.asarray(weight, np.float32).astype(np.float64), half_weights(weight)
    Kc = coef32.shape[1]
    loss, k_loss, x_loss = np.zeros(4), np.zeros(4), np.zeros(4)
    rec, k_rec = np.zeros((N, 4)), np.zeros((N, 4))
    grad, k_grad, x_grad = np.zeros((2, N, Kc)), np.zeros((2, N, Kc)), np.zeros((2, N, Kc))
    for pi, (compT, means, sl, cols, use_exp) in enumerate(parts_of(bases, layout, W)):
        A, mu, cf = np.asarray(compT, np.float64), np.asarray(means, np.float64), coef32[:, sl].astype(np.float64)
        C, K = A.shape
        p = cf @ A.T + mu
        xarg = (K + 2) * U * (np.abs(cf) @ np.abs(A).T + np.abs(mu))
        t = truth32[:, cols].astype(np.float64)
        if use_exp:
            ep, et = np.exp(p), np.exp(t)
            xp = ep * np.expm1(xarg) + K_EXP * U * ep * np.exp(xarg)
            xt = K_EXP * U * et
            de = ep                                          # e'(p)
        else:
            ep, et, xp, xt, de = p, t, xarg, np.zeros_like(t), np.ones_like(p)
        # position term
        d = ep - et
        eps = U * (np.abs(d) + xp + xt) + xp + xt
        sq_b = 2 * np.abs(d) * eps + eps * eps
        rec[:, 2 * pi] = (d * d).sum(1)
        k_rec[:, 2 * pi] = sq_b.sum(1) + (C + 8) * U64 * rec[:, 2 * pi]
        # motion term
        dp, dt = ep[B:] - ep[:B], et[B:] - et[:B]
        xdp, xdt = xp[B:] + xp[:B], xt[B:] + xt[:B]
        m = dp - dt
        eps_m = U * (np.abs(dp) + np.abs(dt) + np.abs(m) + 2 * (xdp + xdt)) + xdp + xdt
        mq_b = 2 * np.abs(m) * eps_m + eps_m * eps_m
        rec[B:, 2 * pi + 1] = (m * m).sum(1)
        k_rec[B:, 2 * pi + 1] = mq_b.sum(1) + (C + 8) * U64 * rec[B:, 2 * pi + 1]
        # losses
        loss[2 * pi] = (w * rec[:, 2 * pi]).sum() / (N * n)
        loss[2 * pi + 1] = (h * rec[B:, 2 * pi + 1]).sum() / (B * n)
        k_loss[2 * pi] = (w * k_rec[:, 2 * pi]).sum() / (N * n) + ((N + 8) * U64 + U) * loss[2 * pi]
        k_loss[2 * pi + 1] = (h * k_rec[B:, 2 * pi + 1]).sum() / (B * n) + ((N + 8) * U64 + U) * loss[2 * pi + 1]
        # the reference's float32 reduction: the square, G - 1 additions of a group, n - 1 additions and a division over the
        # groups, the weight, rows - 1 additions and a division over the batch; the motion term also rounds h_k's product
        G = C // n
        x_loss[2 * pi] = (1 + (G - 1) + n + 1 + N) * U * loss[2 * pi]
        x_loss[2 * pi + 1] = (1 + (G - 1) + n + 1 + B) * U * loss[2 * pi + 1]
        # gradients: g (unscaled) and its error, term p on every row, term m on the pair
        xde = xp if use_exp else np.zeros_like(p)            # error of e'(p)
        rnd = U if use_exp else 0.0                          # the product d * e' is rounded on rotat columns only
        gp = d * de
        dgp = eps * (de + xde) + np.abs(d) * xde + rnd * np.abs(gp)
        gm = np.concatenate((-m * de[:B], m * de[B:]))
        m2, em2 = np.concatenate((m, m)), np.concatenate((eps_m, eps_m))
        dgm = em2 * (de + xde) + np.abs(m2) * xde + rnd * np.abs(gm)
        cp = 2 * w / (N * n)
        cm = 2 * np.concatenate((h, h)) / (B * n)
        absA = np.abs(A)
        for term, (g, dg, c) in enumerate(((gp, dgp, cp), (gm, dgm, cm))):
            val = c[:, None] * (g @ A)
            grad[term][:, sl] = val
            k_grad[term][:, sl] = c[:, None] * (dg @ absA + C * U * (np.abs(g) @ absA)) + (U + 8 * U64) * np.abs(val)
            # the reference's backward rounds the scalar chain (1 / rows, the weight, 1 / n, the factor 2, the residual's sign
            # and, on rotat columns, exp's derivative) in float32: eight roundings on g at the most
            x_grad[term][:, sl] = c[:, None] * (8 * U * (np.abs(g) @ absA))
    return dict(loss=loss, rec=rec, grad=grad, k_loss=k_loss, k_rec=k_rec, k_grad=k_grad, ref32_extra_loss=x_loss, ref32_extra_grad=x_grad)


def case(layout, T_or_W, Ks, Kr, B, seed, weights="unit", coef_scale=1.0):
    """Seeded float32 inputs: bases like the synthetic heads' (compT ~ N(0, 0.02), means ~ N(0, 0.01)), coefficients N(0, 1),
    truth = the float64 prediction of OTHER coefficients plus noise, so the residuals are of the predictions' size; rotat
    arguments stay far below 3 in magnitude."""
    rs = np.random.RandomState(seed)
    f32 = np.float32
    N = 2 * B
    bases = {}
    if layout == "dgrad":
        T, W = T_or_W, 9 * T_or_W
        bases["compT_s"], bases["means_s"] = rs.normal(0, 0.02, (6 * T, Ks)).astype(f32), rs.normal(0, 0.01, 6 * T).astype(f32)
        bases["compT_r"], bases["means_r"] = rs.normal(0, 0.02, (3 * T, Kr)).astype(f32), rs.normal(0, 0.01, 3 * T).astype(f32)
        Kc = Ks + Kr
    else:
        W = T_or_W
        bases["compT_s"], bases["means_s"] = rs.normal(0, 0.02, (W, Ks)).astype(f32), rs.normal(0, 0.01, W).astype(f32)
        Kc = Ks
    coef = (rs.normal(0, 1, (N, Kc)) * coef_scale).astype(f32)
    other = rs.normal(0, 1, (N, Kc)) * coef_scale
    truth = np.zeros((N, W))
    for compT, means, sl, cols, _ in parts_of(bases, layout, W):
        truth[:, cols] = other[:, sl] @ np.asarray(compT, np.float64).T + np.asarray(means, np.float64)
    truth = (truth + rs.normal(0, 0.01, truth.shape)).astype(f32)
    # uniform on 0.2 .. 2 in steps of 2^-10: then h_k is exact in float32 and a double-precision run of the reference, which
    # adds the weights in double, has the same h_k
    weight = np.ones(N, f32) if weights == "unit" else (np.round(rs.uniform(0.2, 2.0, N) * 1024) / 1024).astype(f32)
    return dict(layout=layout, coef=coef, bases=bases, truth=truth, weight=weight)
