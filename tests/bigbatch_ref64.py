"""The float64 value of a training step on a PERIODIC batch, however large, from the float64 models of a few frames: what lets
tests/test_gpu_bigbatch_train.py hold the four GPU trainers to float64 at the largest batches their headers accept.

The batch.  A pool of POOL = 7 distinct frames (rows, for the head) comes from the ref module's own case(...).  Frame n of the large
batch is pool frame j_n and its incoming gradient is 2^{k_n} times pool gradient j_n, j_n in 0 .. 6 and k_n in {-1, 0, 1} from a
seeded generator (`draw`).  7 is odd and the draw is random so that an index that wraps by a power of two lands on another pool
frame and another weight.  A sparse pass keeps the incoming gradient on a set S of frames (`keep`) and sets it to exactly zero
elsewhere.

The gradients.  Every backward is linear in the incoming gradient, so with A_j = sum_{n kept, j_n = j} 2^{k_n} (`weights`) a
gradient is sum_j A_j (frame j's own gradient), and the ref modules' per-frame operands (their run(..., pieces=True)) give it
exactly.  kappa follows the modules' own rules and nothing else: errors that come in over the rows add linearly, so the
first-order part is sum_j |A_j| times frame j's, and the summation part is the modules' "n products summed in ANY order",
sqrt(R + 1) U sum_j |A_j| |a|^T |b|_j with R the number of summed rows that are not exactly zero -- frames kept times 64 for the
contractions over (n, t), frames kept for those over n (the attention layer's dWq and dWc, the head), frames kept times 2,048 for
the frequency LSTM's contractions over (column, step), whose frame is 64 columns.  Every sigma of a backward
is homogeneous of degree one in the incoming gradient, so the weights carry through.  One Adam step is headtrain_ref64.adam.

tests/test_bigbatch_ref64_cpu.py pins all of this against the modules' plain run on a materialised batch.

Controls are wrong models from other weights (`without`, `twice`, `misread`): frames left out, a row block counted twice, a frame
read from another index.  How far a control lies from the right model is a property of the float64 models and is measured with
them alone; where one frame of S_blocks does not lie 10 x kappa away in one pass over the whole set (the BiLSTM layer: its kappa
is a few percent of a frame's own gradient), the set is run as several interleaved passes (`passes`, VARIANTS below)."""
import numpy as np

import attntrain_ref64 as AT
import freqtrain_ref64 as FT
import headtrain_ref64 as HD
import lstmtrain_ref64 as LS
from headtrain_ref64 import LAMBDA, U, adam

POOL = 7
K_VALUES = (-1, 0, 1)
TINY = 2.0 ** -100          # a non-zero pool value below this is left out of the scaled bit comparison (a share of at most TINY_SHARE)
TINY_REF = 2.0 ** -90       # the float64 models' pool dX / dH / dz have no non-zero element below this
TINY_SHARE = 1e-6


# ---------------------------------------------------------------------------------------------------- the construction
def draw(N, seed):
    """-> (j, k): frame n is pool frame j[n], its incoming gradient 2^k[n] times the pool's"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, POOL, N), rs.randint(K_VALUES[0], K_VALUES[-1] + 1, N)


def weights(j, k, keep=None):
    """-> (A [POOL], number of kept frames); keep: None (every frame), a boolean mask or an index array"""
    j, k = np.asarray(j), np.asarray(k)
    if keep is not None:
        j, k = j[keep], k[keep]
    return np.bincount(j, weights=2.0 ** k, minlength=POOL), len(j)


def edge_frames(N, tile, block, seed):
    """S_edges: the first and last frame of the first tile, of the last whole tile and of the last (possibly ragged) tile, the two
    frames either side of the middle block boundary, and 8 seeded frames; ascending, each once"""
    whole, ntiles, nblk = N // tile, -(-N // tile), -(-N // block)
    mid = (nblk // 2) * block
    s = [0, min(tile, N) - 1, (whole - 1) * tile, whole * tile - 1, (ntiles - 1) * tile, N - 1, mid - 1, mid]
    s += list(np.random.RandomState(seed).choice(N, 8, replace=False))
    return np.unique(np.asarray([x for x in s if 0 <= x < N], np.int64))


def block_frames(N, block, every, seed):
    """S_blocks: one seeded frame in every `every`-th block of `block` frames"""
    rs = np.random.RandomState(seed)
    return np.asarray([rs.randint(lo, min(lo + block, N)) for lo in range(0, N, block * every)], np.int64)


def without(A, j, k, frames):
    """control: the frames `frames` left out"""
    return A - weights(j, k, frames)[0]


def twice(A, j, k, frames):
    """control: the frames `frames` counted twice"""
    return A + weights(j, k, frames)[0]


def passes(S, groups):
    """S_blocks as `groups` interleaved sparse passes"""
    return [S[g::groups] for g in range(groups)]


def dense_controls(model, j, k, N, tile, tiles):
    """-> (the right model of the dense pass, {control: wrong model}): the last `tiles` tiles' frames left out, and counted twice.
    model(keep=, A=, frames=, step=) is a trainer's *_periodic on its pool."""
    right = model()
    last = np.arange((-(-N // tile) - tiles) * tile, N)
    wrong = lambda A: model(A=A, frames=right["frames"], step=False)
    return right, {f"the last {tiles} tiles left out": wrong(without(right["A"], j, k, last)),
                   f"the last {tiles} row blocks counted twice": wrong(twice(right["A"], j, k, last))}


def block_controls(model, j, k, S, off):
    """-> (the right model of the sparse pass S, {control: wrong model}, the pool frames' unit distances): one frame of S left out,
    and one frame of S read from frame n - off.  Which frame: the one whose loss the float64 model sees best, by the distances d_j
    of the models that lack one unit of pool frame j (the gradients are linear in the weights, so a frame's loss lies 2^k d_j
    away).  The choice reads the float64 model alone."""
    right = model(keep=S, step=False)
    wrong = lambda A: model(A=A, frames=right["frames"], step=False)
    d = np.asarray([distance(right, wrong(right["A"] - e)) for e in np.eye(POOL)])
    seen = lambda n: 2.0 ** k[n] * d[j[n]]
    drop = max(S, key=seen)
    far = [n for n in S if n >= off and j[n - off] != j[n]]
    assert far, "no frame of S can be misread"
    mis = max(far, key=lambda n: max(seen(n), seen(n - off)))
    return right, {f"frame {drop} of S left out": wrong(without(right["A"], j, k, [drop])),
                   f"frame {mis} of S read from frame {mis - off}": wrong(misread(right["A"], j, k, mis, off))}, d


def misread(A, j, k, n, off):
    """control: frame n read from frame n - off of the dense batch (its pool frame, its weight)"""
    A = A.copy()
    A[j[n]] -= 2.0 ** k[n]
    A[j[n - off]] += 2.0 ** k[n - off]
    return A


def distance(right, wrong):
    """the largest |wrong gradient - right gradient| / (right kappa) over every gradient element"""
    worst = 0.0
    for n, g in right["grads"].items():
        kap = right["k_grads"][n]
        d = np.abs(wrong["grads"][n] - g)
        worst = max(worst, float((d[kap > 0] / kap[kap > 0]).max(initial=0.0)))
    return worst


def _table(L, eL, R, eR, per, post=None):
    """A contraction over rows, frame by frame, for L, R [POOL][r][.] and their sigmas: the frame's own value g_j = L_j^T R_j, the
    first-order part fo_j = eL_j^T |R_j| + |L_j|^T eR_j of its sigma, and ab_j = |L_j|^T |R_j|, which the summation part weighs;
    per: rows a frame adds to the sum; post: the gradient's own layout"""
    T = lambda x: x.transpose(0, 2, 1)
    aL, aR = np.abs(L), np.abs(R)
    fo = T(eL) @ aR
    if eR is not None:
        fo = fo + T(aL) @ eR
    return dict(g=T(L) @ R, fo=fo, ab=T(aL) @ aR, per=per, post=post or (lambda x: x))


def _combine(t, A, B, frames):
    """-> (value, sigma) of the table's contraction over the batch with frame weights A (B = |A|), `frames` frames not zero"""
    g = np.tensordot(A, t["g"], 1)
    e = np.tensordot(B, t["fo"], 1) + np.sqrt(frames * t["per"] + 1) * U * np.tensordot(B, t["ab"], 1)
    return t["post"](g), t["post"](e)


def _pick(j, k, keep, A, frames):
    if A is None:
        A, frames = weights(j, k, keep)
    assert frames is not None
    return np.asarray(A, np.float64), np.abs(A), int(frames)


def _result(pool, grads, kg, A, frames, step):
    out = dict(grads=grads, k_grads=kg, A=A, frames=frames)
    if step:                                                    # one Adam step from zero moments
        out["params1"], out["k_params1"] = {}, {}
        for n, g in grads.items():
            p = np.asarray(pool["params"][n], np.float64)
            r = adam(p, g, np.zeros_like(p), np.zeros_like(p), 1, eg=kg[n])
            out["params1"][n], out["k_params1"][n] = r[0], r[3]
    return out


def _plain(pool, j, k, keep, A, frames, step):
    A, B, frames = _pick(j, k, keep, A, frames)
    grads, kg = {}, {}
    for n, t in pool["tables"].items():
        g, e = _combine(t, A, B, frames)
        grads[n], kg[n] = g, LAMBDA * e
    return _result(pool, grads, kg, A, frames, step)


# ---------------------------------------------------------------------------------------------------- the BiLSTM layer
def lstm_pool(layer, params, X_pool, dY_pool):
    """the pool's float64 run (Y, dX and their kappas included) and its per-frame tables"""
    assert len(X_pool) == POOL
    r = LS.run(layer, params, X_pool, dY_pool, pieces=True)
    nm = LS.names(layer)
    tables = {}
    for d, p in enumerate(r.pop("pieces")):
        tables[nm[d]] = _table(p["dG"], p["e_dG"], p["X"], p["e_X"], LS.TS)
        tables[nm[2 + d]] = _table(p["dG"], p["e_dG"], p["hprev"], p["e_hprev"], LS.TS)
    return dict(run=r, params=params, tables=tables)


def lstm_periodic(layer, params, X_pool, dY_pool, j, k, keep=None, A=None, frames=None, pool=None, step=True):
    """-> dict grads, k_grads, params1, k_params1 (after one Adam step; step=False leaves them out) of the periodic batch (j, k) with
    the incoming gradient kept on `keep`; A / frames: other weights and the number of frames that are not zero, for the controls;
    pool: lstm_pool(...) if at hand"""
    return _plain(pool or lstm_pool(layer, params, X_pool, dY_pool), j, k, keep, A, frames, step)


# ---------------------------------------------------------------------------------------------------- the attention layer
def attn_pool(params, H_pool, dz_pool):
    assert len(H_pool) == POOL
    r = AT.run(params, H_pool, dz_pool, pieces=True)
    p = r.pop("pieces")
    f3 = lambda x: x[:, None, :]                               # a frame is one row of the contractions over n
    ds, e_ds = p["ds"][:, :, None], p["e_ds"][:, :, None]
    shaped = lambda n: (lambda x: x.reshape(AT.SHAPES[n]))
    tables = {
        AT.V: _table(ds, e_ds, p["u"], p["e_u"], AT.TS, shaped(AT.V)),
        AT.B: _table(p["dpre"], p["e_dpre"], np.ones((POOL, AT.TS, 1)), None, AT.TS, shaped(AT.B)),
        AT.WK: _table(p["dpre"], p["e_dpre"], p["H"].reshape(POOL, AT.TS, AT.D), None, AT.TS),
        AT.WQ: _table(f3(p["dqp"]), f3(p["e_dqp"]), f3(p["qc"]), f3(p["e_qc"]), 1),
        AT.WC: _table(f3(p["dqc"]), f3(p["e_dqc"]), f3(p["hq"]), None, 1,
                      lambda x: np.ascontiguousarray(x.reshape(AT.D, AT.KW, AT.D).transpose(0, 2, 1))),
    }
    return dict(run=r, params=params, tables=tables)


def attn_periodic(params, H_pool, dz_pool, j, k, keep=None, A=None, frames=None, pool=None, step=True):
    """as lstm_periodic, for the attention layer: dv, db and dWk sum over the rows (n, t), dWq and dWc over the frames"""
    return _plain(pool or attn_pool(params, H_pool, dz_pool), j, k, keep, A, frames, step)


# ---------------------------------------------------------------------------------------------------- the head
def head_pool(head, params, z_pool, sid_pool, dcoef_pool):
    assert len(z_pool) == POOL
    r = HD.run(head, params, z_pool, sid_pool, dcoef_pool, pieces=True)
    f3 = lambda x: x[:, None, :]
    tables = {}
    for n, (D, eD, X, eX) in r.pop("pieces").items():
        tables[n + ".bias"] = _table(f3(D), f3(eD), np.ones((POOL, 1, 1)), None, 1, lambda x: x[:, 0])
        tables[n] = _table(f3(D), f3(eD), f3(X), f3(eX), 1)
    return dict(run=r, params=params, tables=tables, head=head, fold=r.pop("fold"))


def head_periodic(head, params, z_pool, sid_pool, dcoef_pool, j, k, keep=None, A=None, frames=None, pool=None, step=True):
    """as lstm_periodic, for the head: a frame is a row, the speaker id belongs to the pool row, and the weight norm's backward
    (headtrain_ref64.weight_norm_backward) follows the sum over the rows"""
    pool = pool or head_pool(head, params, z_pool, sid_pool, dcoef_pool)
    A, B, frames = _pick(j, k, keep, A, frames)
    grads, kg = {}, {}
    for L in HD.layers_of(head):
        n = L["name"]
        g, e = _combine(pool["tables"][n + ".bias"], A, B, frames)
        grads[n + ".bias"], kg[n + ".bias"] = g, LAMBDA * e
        dW, edW = _combine(pool["tables"][n], A, B, frames)
        grads[n + ".weight_g"], kg[n + ".weight_g"], grads[n + ".weight_v"], kg[n + ".weight_v"] = HD.weight_norm_backward(pool["fold"][n], L["K"], dW, edW)
    return _result(pool, grads, kg, A, frames, step)


# ---------------------------------------------------------------------------------------------------- the frequency LSTM
def freq_pool(params, C_pool, dX0_pool):
    """the pool's float64 run (X0, dC and their kappas per frame) and its per-frame tables.  A frame is 64 columns: C_pool
    [POOL 64][32][64], dX0_pool [POOL 64][256].  dWp and dbp sum over the columns, 64 rows a frame; dW_ih, dW_hh and the bias
    gradient over the pairs (column, step), 2,048 rows a frame.  bias_ih and bias_hh of a direction share one table (the same
    gradient) and each takes its own Adam step."""
    assert len(C_pool) == len(dX0_pool) == POOL * FT.COLS
    r = FT.run(params, C_pool, dX0_pool, pieces=True)
    p = r.pop("pieces")
    nm = FT.names()
    cols = lambda x: x.reshape(POOL, FT.COLS, -1)
    pairs = lambda x: x.reshape(POOL, FT.COLS * FT.NS, -1)
    tables = {
        nm[8]: _table(cols(p["D"]), cols(p["e_D"]), cols(p["HF"]), cols(p["e_HF"]), FT.COLS),
        nm[9]: _table(cols(p["D"]), cols(p["e_D"]), np.ones((POOL, FT.COLS, 1)), None, FT.COLS, lambda x: x[:, 0]),
    }
    ones = np.ones((POOL, FT.COLS * FT.NS, 1))
    for d, q in enumerate(p["dirs"]):
        dG, e_dG = pairs(q["dG"]), pairs(q["e_dG"])
        tables[nm[d]] = _table(dG, e_dG, pairs(q["Cf"]), pairs(q["eCf"]), FT.COLS * FT.NS)
        tables[nm[2 + d]] = _table(dG, e_dG, pairs(q["hprev"]), pairs(q["e_hprev"]), FT.COLS * FT.NS)
        tables[nm[4 + d]] = tables[nm[6 + d]] = _table(dG, e_dG, ones, None, FT.COLS * FT.NS, lambda x: x[:, 0])
    for n, shape in (("X0", (FT.COLS, FT.NO)), ("dC", (FT.COLS, FT.NS, FT.NI))):
        r[n], r["k_" + n] = r[n].reshape((POOL,) + shape), r["k_" + n].reshape((POOL,) + shape)
    return dict(run=r, params=params, tables=tables)


def freq_periodic(params, C_pool, dX0_pool, j, k, keep=None, A=None, frames=None, pool=None, step=True):
    """as lstm_periodic, for the frequency LSTM and its projection"""
    return _plain(pool or freq_pool(params, C_pool, dX0_pool), j, k, keep, A, frames, step)


# ---------------------------------------------------------------------------------------------------- the cases
# What tests/test_gpu_bigbatch_train.py runs and tests/test_bigbatch_ref64_cpu.py pins, per trainer variant.  N: the batches.
# tile / block: frames (rows) of a recurrence tile (row tile) and of a row block of the split dW contractions; S_blocks takes one
# frame in every `every`-th block; a misread frame comes from `off` frames earlier.  pool_seed: the seed of the ref module's case.
# dense_tiles and groups are measured on the CPU with the float64 models alone (test_bigbatch_ref64_cpu.py asserts them):
# dense_tiles is the smallest whole number of last tiles whose loss, or double count, lies 10 x kappa from the dense pass's right
# model at both N; groups is the smallest number of interleaved passes S_blocks is run as so that the loss of one frame of a pass,
# and its misreading, lie 10 x kappa from that pass's right model at both N.
VARIANTS = {
    "lstm-l0": dict(N=(3072, 3041), tile=32, block=32, every=1, off=2048, pool_seed=700, dense_tiles=31, groups=6),
    "lstm-l1": dict(N=(3072, 3041), tile=32, block=32, every=1, off=2048, pool_seed=701, dense_tiles=47, groups=13),
    "attn": dict(N=(32768, 32761), tile=16, block=16, every=32, off=2048, pool_seed=902, dense_tiles=216, groups=1),
    "head-dgrad": dict(N=(2 ** 18 + 2,), tile=64, block=64, every=64, off=2 ** 16, pool_seed=720, dense_tiles=11, groups=1),
    "head-offsets": dict(N=(2 ** 18 + 2,), tile=64, block=64, every=64, off=2 ** 16, pool_seed=727, dense_tiles=10, groups=1),
    # the frequency LSTM: a frame is 64 columns, the periodic unit a frame (two recurrence tiles per direction), a row block 8 frames;
    # 1,024 frames are 2^31 gate floats, the distance at which a 32-bit gate index would alias.  Measured: the last 4 frames lost or
    # counted twice lie 10.5 x kappa away at N = 2,048 and 47.3 x at 1,033 (3 frames: 9.05 x and 36.4 x; 1 frame: 5.76 x and 15.3 x),
    # on dbp, whose kappa is 2e-4 of the gradient; dW_ih, dW_hh and db (kappa 2 - 26 % of the gradient) do not see them (0.7 - 2.8 x).
    # S_blocks in ONE pass of 256 / 130 frames: the best-seen frame lost lies 134 / 322 x away, a frame read from 1,024 earlier 113 / 130 x
    "freq": dict(N=(2048, 1033), tile=1, block=8, every=1, off=1024, pool_seed=740, dense_tiles=4, groups=1),
}
_POOLS = {}


def pool_case(variant):
    """the ref module's case the pool is taken from: 7 frames; for the head 8 rows, whose first 7 are the pool (the head takes
    even batches only, so the device runs the pool as the 8 rows)"""
    kind, _, which = variant.partition("-")
    seed = VARIANTS[variant]["pool_seed"]
    if kind == "lstm":
        return LS.case(int(which[1]), POOL, seed, "carry")
    if kind == "attn":
        return AT.case(POOL, seed, "peaked")
    if kind == "freq":
        return FT.case(FT.COLS * POOL, seed, "carry")
    return HD.case(which, (POOL + 1) // 2, seed)


def pool_of(variant):
    """the variant's pool tables, made once"""
    if variant not in _POOLS:
        c = pool_case(variant)
        kind = variant.partition("-")[0]
        if kind == "lstm":
            _POOLS[variant] = lstm_pool(c["layer"], c["params"], c["X"], c["dY"])
        elif kind == "attn":
            _POOLS[variant] = attn_pool(c["params"], c["H"], c["dz"])
        elif kind == "freq":
            _POOLS[variant] = freq_pool(c["params"], c["C"], c["dX0"])
        else:
            _POOLS[variant] = head_pool(c["head"], c["params"], c["z"][:POOL], c["sid"][:POOL], c["dcoef"][:POOL])
    return _POOLS[variant]


def sets(variant, N):
    """-> (j, k, S_edges, S_blocks) of the variant's batch of N frames"""
    v = VARIANTS[variant]
    j, k = draw(N, 31 + N)
    return j, k, edge_frames(N, v["tile"], v["block"], 41 + N), block_frames(N, v["block"], v["every"], 51 + N)


def model_of(variant, N):
    """model(keep=None, A=None, frames=None, step=True): the variant's periodic model of its batch of N frames"""
    pool = pool_of(variant)
    j, k = draw(N, 31 + N)

    def model(keep=None, A=None, frames=None, step=True):
        if "head" in pool:
            return head_periodic(pool["head"], None, None, None, None, j, k, keep, A, frames, pool, step)
        return _plain(pool, j, k, keep, A, frames, step)
    return model
