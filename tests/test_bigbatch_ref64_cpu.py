"""tests/bigbatch_ref64.py pinned before any GPU is involved: the float64 value and kappa of a training step on a periodic batch,
built from the pool's per-frame operands, against the ref modules' plain run on the same batch written out frame by frame.

    the periodic model is the plain run     N = 14 (and 15 for the BiLSTM layer and the attention layer, 17 for the frequency LSTM:
                                            two whole row blocks and a frame): every gradient within 1e-12
                                            of the array's largest magnitude (both are float64 sums of the same terms in another
                                            order, whose difference is bounded by the terms, not by an element that cancels), every
                                            kappa within 1e-12 relative, with R the written-out batch's row count; the Adam step is
                                            headtrain_ref64.adam of that gradient and kappa, bit for bit; a frame's Y and dX are the
                                            pool frame's, times 2^k
    the sparse rule                         incoming gradients exactly zero on all but three frames of 14: the periodic model with
                                            R = the rows of those three frames is `run` on those three frames alone
    the subnormal condition                 the float64 pool dX / dH / dz has no non-zero element below 2^-90, so the 2^-100 the GPU
                                            test leaves out of its scaled bit comparison takes nothing from the reference
    the controls' strength                  at the sizes the GPU test runs (the model costs the same at any N): each wrong model of
                                            bigbatch_ref64.dense_controls and block_controls lies at least 10 x kappa from the right
                                            one, with the dense_tiles and groups of bigbatch_ref64.VARIANTS

Measured (pytest -s prints every figure).  One lost tile is NOT seen by the dense pass: kappa there grows with sqrt(rows) U and with
the linearly added first-order errors of every row.  The last tiles whose loss (or double count) reaches 10 x kappa: 31 of 96
(layer 0, 10.1 - 10.3 x; 30 tiles 9.83 x at N = 3,041) and 47 of 96 (layer 1, 10.1 - 10.3 x; 46 tiles 9.9 x) for the BiLSTM layer, 216
of 2,048 row blocks for the attention layer (10.0 - 10.2 x; 215 blocks 9.94 x), 11 and 10 of 4,097 row tiles for the dgrad and the
offsets head (10.2 and 10.1 x; one fewer 9.3 and 9.0 x).  One frame of S_blocks -- the one the float64 model sees best -- in a single
pass over all of it lies 1.9 - 3.5 x kappa away for the BiLSTM layer (96 frames), 13.7 - 16.3 x for the attention layer (64 frames)
and 2.6e4 - 2.9e4 x for the head (65 rows): the BiLSTM's S_blocks is therefore run as 6 (layer 0) and 13 (layer 1) interleaved
passes of 16 and 7 - 8 frames, the smallest numbers at which the two controls of every pass lie 10 x kappa away at both N.  Over all
frames of S_blocks the loss of one lies 2.4 - 31 x kappa from its pass's model (BiLSTM), 0.07 - 16 x (attention; a pool frame whose
largest align is 0.98 has next to no gradient: no gradient check resolves such a frame, the bit comparison of its dH does),
3.8e3 - 2.9e4 x (head).  The frequency LSTM (a frame is 64 columns; N = 2,048 and 1,033): its dbp and dWp sum exact incoming
gradients, their kappa is 2e-4 and 9e-4 of the gradient, and the last 4 frames lost or counted twice lie 10.5 x (N = 2,048) and 47.3 x
(1,033) away (3 frames 9.05 x and 36.4 x), while dW_ih, dW_hh and db, whose kappa is 2 - 26 % of the gradient, see them at 0.7 - 2.8 x
only; S_blocks runs as ONE pass of 256 and 130 frames, in which the best-seen frame's loss lies 134 and 322 x away and its misreading
from 1,024 frames earlier 113 and 130 x; over all its frames a loss lies 31.9 - 322 x away.  The module takes 60 s, 32 s of them
the frequency LSTM's float64 runs."""
import numpy as np
import pytest

import attntrain_ref64 as AT
import bigbatch_ref64 as BB
import freqtrain_ref64 as FT
import headtrain_ref64 as HD
import lstmtrain_ref64 as LS

# the frequency LSTM's float64 run takes seconds per 576 columns: its written-out batches are 14 frames and 17 (two whole row blocks and a frame)
SMALL = [(v, N) for v in BB.VARIANTS for N in ((14,) if v.startswith("head") else (14, 17) if v == "freq" else (14, 15))]
LARGE = [(v, N) for v, d in BB.VARIANTS.items() for N in d["N"]]
ids = lambda cases: [f"{v}-N{n}" for v, n in cases]


def plain(variant, frames, w):
    """the ref module's plain run on the batch whose frame i is pool frame frames[i] with its incoming gradient times w[i]"""
    c = BB.pool_case(variant)
    f32 = np.float32
    if variant.startswith("lstm"):
        return LS.run(c["layer"], c["params"], c["X"][frames], (c["dY"][frames] * w[:, None, None]).astype(f32))
    if variant == "attn":
        return AT.run(c["params"], c["H"][frames], (c["dz"][frames] * w[:, None]).astype(f32))
    if variant == "freq":
        C4, dX3 = c["C"].reshape(BB.POOL, FT.COLS, FT.NS, FT.NI), c["dX0"].reshape(BB.POOL, FT.COLS, FT.NO)
        r = FT.run(c["params"], C4[frames].reshape(-1, FT.NS, FT.NI), (dX3[frames] * w[:, None, None]).astype(f32).reshape(-1, FT.NO))
        for n in ("X0", "k_X0", "dC", "k_dC"):                  # per frame, as the pool's
            r[n] = r[n].reshape((len(frames), FT.COLS) + r[n].shape[1:])
        return r
    return HD.run(c["head"], c["params"], c["z"][frames], c["sid"][frames], (c["dcoef"][frames] * w[:, None]).astype(f32))


def periodic(variant, j, k, keep=None):
    """through the module's public entry point"""
    c, pool = BB.pool_case(variant), BB.pool_of(variant)
    if variant.startswith("lstm"):
        return BB.lstm_periodic(c["layer"], c["params"], c["X"], c["dY"], j, k, keep, pool=pool)
    if variant == "attn":
        return BB.attn_periodic(c["params"], c["H"], c["dz"], j, k, keep, pool=pool)
    if variant == "freq":
        return BB.freq_periodic(c["params"], c["C"], c["dX0"], j, k, keep, pool=pool)
    P = BB.POOL
    return BB.head_periodic(c["head"], c["params"], c["z"][:P], c["sid"][:P], c["dcoef"][:P], j, k, keep, pool=pool)


OUT = {"lstm": ("Y", "dX"), "attn": ("z", "align", "dH"), "head": ("coef", "dz"), "freq": ("X0", "dC")}          # forward outputs first, dX / dH / dz last


def same(variant, per, ref):
    worst = 0.0
    for n, g in ref["grads"].items():
        scale = np.abs(g).max()
        d = float(np.abs(per["grads"][n].reshape(g.shape) - g).max() / scale)
        assert d <= 1e-12, (variant, n, d)
        kd = np.abs(per["k_grads"][n].reshape(g.shape) - ref["k_grads"][n])
        assert (kd <= 1e-12 * ref["k_grads"][n]).all(), (variant, n, float((kd / np.maximum(ref["k_grads"][n], 1e-300)).max()))
        p = np.asarray(BB.pool_case(variant)["params"][n], np.float64)
        # Adam's first step is lr g / (|g| + eps) and its kappa divides by sqrt(v) less its own error: neither is a
        # 1e-12-conditioned function of the gradient where that is near eps.  The step is held as what it is,
        # headtrain_ref64.adam of the periodic model's own gradient and kappa, bit for bit
        r = HD.adam(p, per["grads"][n], np.zeros_like(p), np.zeros_like(p), 1, eg=per["k_grads"][n])
        assert per["grads"][n].shape == p.shape and (per["params1"][n] == r[0]).all() and (per["k_params1"][n] == r[3]).all(), (variant, n)
        worst = max(worst, d)
    return worst


@pytest.mark.parametrize("variant,N", SMALL, ids=ids(SMALL))
def test_periodic_model_is_the_plain_run_on_the_written_out_batch(variant, N):
    j, k = BB.draw(N, 7 + N)
    assert len(set(j)) > 3 and set(k) == set(BB.K_VALUES)
    ref = plain(variant, j, 2.0 ** k)
    per = periodic(variant, j, k)
    assert per["frames"] == N
    worst = same(variant, per, ref)
    # a frame's outputs are the pool frame's: the forward's as they are, the backward's times 2^k
    pool = BB.pool_of(variant)["run"]
    names = OUT[variant.partition("-")[0]]
    for n in names:
        w = 2.0 ** k if n == names[-1] else np.ones(N)
        want = pool[n][j] * w.reshape((N,) + (1,) * (pool[n].ndim - 1))
        assert (np.abs(ref[n] - want) <= 1e-12 * np.abs(want).max()).all(), (variant, n)
    print(f"\n{variant} N = {N}: periodic model against the plain run, largest gradient difference {worst:.2e} of the array's scale")


@pytest.mark.parametrize("variant", list(BB.VARIANTS))
def test_sparse_rule_is_the_run_on_the_kept_frames_alone(variant):
    N = 14
    j, k = BB.draw(N, 7 + N)
    S = np.sort(np.random.RandomState(3).choice(N, 3, replace=False))
    per = periodic(variant, j, k, S)
    assert per["frames"] == 3
    same(variant, per, plain(variant, j[S], 2.0 ** k[S]))
    # the whole batch with exact zeros off S: the same values (its kappa counts every row, the rule counts those of S)
    w = np.zeros(N)
    w[S] = 2.0 ** k[S]
    full = plain(variant, j, w)
    names = OUT[variant.partition("-")[0]]
    off = np.setdiff1d(np.arange(N), S)
    assert (full[names[-1]][off] == 0).all() and (full["k_" + names[-1]][off] == 0).all()
    for n, g in full["grads"].items():
        assert np.abs(per["grads"][n].reshape(g.shape) - g).max() <= 1e-12 * np.abs(g).max(), (variant, n)
        assert (per["k_grads"][n].reshape(g.shape) <= full["k_grads"][n] * (1 + 1e-12)).all(), (variant, n)


@pytest.mark.parametrize("variant", list(BB.VARIANTS))
def test_pool_gradients_have_no_element_near_the_subnormal_range(variant):
    pool = BB.pool_of(variant)["run"]
    a = np.abs(pool[OUT[variant.partition("-")[0]][-1]])
    nz = a[a > 0]
    print(f"\n{variant}: the smallest non-zero |pool dX| is 2^{np.log2(nz.min()):.1f}; {int((a == 0).sum())} exact zeros")
    assert nz.size and nz.min() >= BB.TINY_REF > BB.TINY


@pytest.mark.parametrize("variant,N", LARGE, ids=ids(LARGE))
def test_controls_lie_ten_kappa_from_the_right_model(variant, N):
    v = BB.VARIANTS[variant]
    j, k, S_edges, S_blocks = BB.sets(variant, N)
    assert len(np.unique(S_edges)) == len(S_edges) >= 12 and S_edges[0] == 0 and S_edges[-1] == N - 1
    assert len(S_blocks) == -(-N // (v["block"] * v["every"])) and (S_blocks // (v["block"] * v["every"]) == np.arange(len(S_blocks))).all()
    model = BB.model_of(variant, N)
    right, wrong = BB.dense_controls(model, j, k, N, v["tile"], v["dense_tiles"])
    assert right["frames"] == N
    for what, w in wrong.items():
        r = BB.distance(right, w)
        print(f"\n{variant} N = {N}, dense pass: {what}: {r:.3g} x kappa from the right model")
        assert r >= 10.0, (variant, N, what, r)
    if v["dense_tiles"] > 1:
        fewer = min(BB.distance(right, w) for w in BB.dense_controls(model, j, k, N, v["tile"], v["dense_tiles"] - 1)[1].values())
        print(f"{variant} N = {N}, dense pass: {v['dense_tiles'] - 1} tiles: {fewer:.3g} x kappa")
    one = BB.block_controls(model, j, k, S_blocks, v["off"])
    print(f"{variant} N = {N}, S_blocks in one pass of {len(S_blocks)} frames: " + ", ".join(f"{what}: {BB.distance(one[0], w):.3g}" for what, w in one[1].items()))
    seen = []
    for g, S in enumerate(BB.passes(S_blocks, v["groups"])):
        right, wrong, d = BB.block_controls(model, j, k, S, v["off"])
        assert right["frames"] == len(S)
        for what, w in wrong.items():
            r = BB.distance(right, w)
            print(f"{variant} N = {N}, S_blocks pass {g} of {len(S)} frames: {what}: {r:.3g} x kappa")
            assert r >= 10.0, (variant, N, g, what, r)
        seen += [2.0 ** k[n] * d[j[n]] for n in S]
    print(f"{variant} N = {N}: the loss of a frame of S_blocks lies {min(seen):.3g} to {max(seen):.3g} x kappa from its pass's right model, "
          f"{np.mean(np.asarray(seen) >= 10.0):.0%} of the frames 10 x or more, {np.mean(np.asarray(seen) > 1.0):.0%} more than 1 x")
