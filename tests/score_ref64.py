"""Float64 restatement of the validation losses (include/sdfa_score.h): the per-frame records, the reference's criterion on
a collated batch, and the error bound of the float32 operations the device forms its terms with.  The blended truth enters
as float32 rows (blend32 restates sdfa_seek_rows' three roundings); everything after it is exact up to float64."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32: one rounded operation on a value x errs by at most U |x|
# Twice the ulp bound of the device's expf.  HIP's math API documentation (docs/reference/math_api, "Single precision
# mathematical functions") lists expf with a maximum error of 1 ULP; 1 ulp of a value v is at most 2 * U * |v|, so one exp
# contributes K_EXP * U * exp(x).  The ROCm installation this was written on ships no copy of that table (no documentation
# file under its prefix mentions expf), so the value stands on the published table, not on a local file.
K_EXP = 2.0
U64 = 2.0 ** -53


def blend32(track, src, w):
    """t[f] = fl(fl(w0 R[s0]) + fl(w1 R[s1])) in float32."""
    track = np.asarray(track, np.float32)
    w = np.asarray(w, np.float32)
    return (track[src[:, 0]] * w[:, 0:1] + track[src[:, 1]] * w[:, 1:2]).astype(np.float32)


def rotat_mask(W, layout):
    return (np.arange(W) % 9 >= 6) if layout == "dgrad" else np.zeros(W, bool)


def records(pred, truth, clip_frame_off, layout):
    """(rec [F][4], bound [F][4]) float64: the record of include/sdfa_score.h and how far float32 terms may move each sum.
        |delta(d^2)| <= 2 |d| eps + eps^2, eps the error of the float32 difference d:
        plain terms   eps = U |d|
        motion terms  eps = U (|dp| + |dt| + |m|)                 dp, dt the two inner differences, m their difference
        exp terms     every exp adds K_EXP U e^x to eps
    plus the double accumulation, U64 per addition on the running sum."""
    p, t = np.asarray(pred, np.float64), np.asarray(truth, np.float64)
    F, W = p.shape
    rot = rotat_mask(W, layout)
    ep, et = np.where(rot, np.exp(p), p), np.where(rot, np.exp(t), t)
    xp, xt = np.where(rot, K_EXP * U * ep, 0.0), np.where(rot, K_EXP * U * et, 0.0)      # error of each e() value
    first = np.zeros(F, bool)
    first[np.asarray(clip_frame_off[:-1], np.int64)] = True
    d = ep - et
    eps = U * (np.abs(d) + xp + xt) + xp + xt
    sq, sq_b = d * d, 2 * np.abs(d) * eps + eps * eps
    dp, dt = np.zeros_like(p), np.zeros_like(p)
    dp[1:], dt[1:] = ep[1:] - ep[:-1], et[1:] - et[:-1]
    xdp, xdt = np.zeros_like(p), np.zeros_like(p)
    xdp[1:], xdt[1:] = xp[1:] + xp[:-1], xt[1:] + xt[:-1]
    m = dp - dt
    eps_m = U * (np.abs(dp) + np.abs(dt) + np.abs(m) + 2 * (xdp + xdt)) + xdp + xdt
    mq, mq_b = m * m, 2 * np.abs(m) * eps_m + eps_m * eps_m
    mq[first], mq_b[first] = 0.0, 0.0
    rec, bound = np.zeros((F, 4)), np.zeros((F, 4))
    for slot, (v, b, cols) in enumerate(((sq, sq_b, ~rot), (sq, sq_b, rot), (mq, mq_b, ~rot), (mq, mq_b, rot))):
        rec[:, slot] = v[:, cols].sum(1)
        bound[:, slot] = b[:, cols].sum(1) + (int(cols.sum()) + 8) * U64 * rec[:, slot]
    return rec, bound


def collate(fc):
    """The validation samples of a clip of fc frames (datasets/sliding_window.py:66-76): pairs (i, i + 1), the last frame
    pairing with its predecessor again; the batch is [a; b]."""
    a = np.concatenate((np.arange(fc - 1), [fc - 2]))
    b = np.concatenate((np.arange(1, fc), [fc - 1]))
    return a, b


def criterion64(pred, truth, weights, layout):
    """PLoss and MLoss (speech_anime/model/criterion.py:7-73) in float64 on the batch [a; b] of ONE clip's rows [fc][W]:
    {"scalar_ps", "scalar_pr", "scalar_ms", "scalar_mr", "scalar_ploss", "scalar_mloss"} as get_loss names them (plain: ps and
    ms carry the whole loss, pr = mr = 0)."""
    p, t = np.asarray(pred, np.float64), np.asarray(truth, np.float64)
    fc, W = p.shape
    a, b = collate(fc)
    idx = np.concatenate((a, b))
    wt = np.ones(fc) if weights is None else np.asarray(weights, np.float64)
    wb = wt[idx]
    out = {}
    parts = (("s", np.arange(W)[~rotat_mask(W, layout)], False), ("r", np.arange(W)[rotat_mask(W, layout)], True))
    for tag, cols, use_exp in parts:
        if cols.size == 0:
            out["scalar_p" + tag] = out["scalar_m" + tag] = 0.0
            continue
        x, y = p[idx][:, cols], t[idx][:, cols]
        if use_exp:
            x, y = np.exp(x), np.exp(y)
        if layout == "dgrad":                  # (N, 1, T, 6 | 3): sum over the last dimension, mean over the others
            per = 6 if tag == "s" else 3
            reduce = lambda z: z.reshape(z.shape[0], -1, per).sum(-1).mean(-1)      # noqa: E731
        else:
            reduce = lambda z: z.mean(-1)                                            # noqa: E731
        out["scalar_p" + tag] = float((reduce((x - y) ** 2) * wb).mean())
        bhs = fc
        mp, mt = x[bhs:] - x[:bhs], y[bhs:] - y[:bhs]
        out["scalar_m" + tag] = float((reduce((mp - mt) ** 2) * (wb[bhs:] + wb[:bhs])).mean())
    out["scalar_ploss"] = out["scalar_ps"] + out["scalar_pr"]
    out["scalar_mloss"] = out["scalar_ms"] + out["scalar_mr"]
    return out


def tracks(n, W, seed, scale=0.05):
    """Seeded float32 rows that move smoothly from row to row, small enough for exp to stay near 1."""
    rs = np.random.RandomState(seed)
    walk = np.cumsum(rs.normal(0, scale / 4, (n, W)), axis=0) + rs.normal(0, scale, (1, W))
    return walk.astype(np.float32)
