"""The four GPU trainers at the largest batches their headers accept, against float64: one BiLSTM layer (csrc/lstmtrain.hip) at
N = 3,072 = SDFA_LSTMTRAIN_MAX_FRAMES (96 whole recurrence tiles and row blocks) and 3,041 (95 whole plus one frame), layers 0 and 1,
family "carry"; the attention layer (csrc/attntrain.hip) at N = 32,768 = SDFA_ATTNTRAIN_MAX_FRAMES and 32,761 (2,047 row blocks plus
9 frames), family "peaked"; both heads (csrc/headtrain.hip) at N = 2^18 + 2 = 262,146 rows (4,096 whole row tiles and a 2-row
tail).  THE HEAD IS NOT EXERCISED BETWEEN 262,146 ROWS AND ITS LIMIT OF 2^21: at 2^21 rows the dgrad head's workspace alone is 36 GiB,
which is not something to hold on a shared card.  Every case of these three holds less than 12 GiB on the device and asserts so.

The frequency LSTM and its projection (csrc/freqtrain.hip), family "carry", at N = 2,048 = SDFA_FREQTRAIN_MAX_FRAMES -- 256 whole
row blocks of 8 frames, 256 partials in the reduce, 2^17 columns, the last gate float at index 2^32 - 1 and the second direction's
gates exactly 2^31 floats behind the first's -- and at N = 1,033: 129 whole row blocks and one of a single frame (64 of 512 columns,
both recurrences' grids ending inside a block), just past the 1,024 frames at which the gate offsets cross 2^31.  A frame is 64
columns; the periodic unit is a frame (tile = 1), a row block 8 frames, a misread frame comes from 1,024 frames earlier, where a
32-bit gate index would alias.  This trainer keeps 14 MiB per frame: its workspace is 30.2 GiB at 2,048 frames, and with C and dC
(1 GiB each), X0, dX0 and the sparse dX0 (0.125 GiB each) and the comparison slices a case holds 33.1 GiB (asserted below 34 GiB;
16.9 GiB, below 18, at N = 1,033).  That is acceptable where the head's 36 GiB was not because it is what ONE train_step at the
header's limit holds in use and what the committed benchmark (tools/freqtrain_bench.py, profiles/freqtrain_bench.json) already held;
the head's 36 GiB lie beyond any batch its training loop forms.  Everything is freed between cases; the bit comparisons run on the
device in slices of 256 frames (a slice of the expected dC and its scaled copy: 256 MiB), and nothing of the batch's size goes to
the host.

The float64 models cannot be run at these sizes, so the batch is periodic (tests/bigbatch_ref64.py, pinned on the CPU by
tests/test_bigbatch_ref64_cpu.py): frame n is one of 7 pool frames, j_n, with its incoming gradient times 2^{k_n}, built on the
device by a gather.  The headers' contracts ("a frame's Y and dX do not depend on the other frames of the batch") and the linearity
of a backward in its incoming gradient then state every per-frame output BIT FOR BIT, and every gradient as sum_j A_j (frame j's
float64 gradient) with a kappa built by the ref modules' own rules; no figure is fitted and no factor is applied to kappa.

Each case:  (a) the pool alone (N = 7; the head takes even batches, so its 7 pool rows run with an eighth) against the ref module's
float64 run, every output within 1 x kappa;  (b) the dense pass: Y / z, align / coef of every frame have the pool frame's bits,
dX / dH / dz of every frame the bits of 2^{k_n} times the pool frame's (compared on the device in slices of 1,024 frames; a non-zero
pool value below 2^-100 would be left out, a share of at most 1e-6 -- none is), every gradient element within 1 x kappa of the
periodic model, the parameters after one Adam step within 1 x kappa;  (c) sparse passes, the incoming gradient exactly zero off a
set S: dX exactly zero off S, the scaled pool bits on S, the gradients within 1 x kappa of the periodic model over S with R counting
S's rows only -- S_edges (the first and last frame of the first tile, of the last whole tile and of the last tile, both sides of the
middle block boundary, 8 seeded frames) and S_blocks (a seeded frame in every row block of the BiLSTM layer, in every 32nd of the
attention layer, in every 64th row tile of the head);  (d) two dense passes leave the same gradient bits, and after the large passes
the same trainer on the same grown workspace leaves the pool run's bits again.

Controls are wrong models; the device must lie more than 1 x kappa from each, and the float64 models say on the CPU that each lies
at least 10 x kappa from the right one.  Dense pass: the last tiles left out, the last row blocks counted twice.  ONE lost tile is
not seen there (kappa grows with sqrt(rows) U and with every row's first-order error): the smallest whole number of tiles that
reaches 10 x is 31 of 96 (layer 0) and 47 of 96 (layer 1) for the BiLSTM layer, 216 of 2,048 for the attention layer, 11 and 10 of
4,097 for the dgrad and offsets head (measured on the CPU: 10.0 - 10.3 x; one tile fewer 9.0 - 10.2 x and below 10 at one of the two
N).  S_blocks carries the per-block claim: one frame of a pass left out, and one read from frame n - 2,048 (n - 2^16 for the head).
In a single pass over all of S_blocks one frame lies 13.7 - 16.3 x (attention) and 2.6e4 - 2.9e4 x (head) away, but only 1.9 - 3.5 x
for the BiLSTM layer, whose kappa is a few percent of a frame's own gradient: its S_blocks runs as 6 (layer 0) and 13 (layer 1)
interleaved passes of 16 and 7 - 8 frames, the smallest numbers at which both controls of every pass reach 10 x.  The controls take
the frame of the pass whose loss the float64 model sees best; across all frames of S_blocks the loss of one lies 2.4 - 31 x kappa from
its pass's model (BiLSTM), 0.07 - 16 x (attention: a saturated softmax leaves a frame next to no gradient; its dH bits are still
held), 3.8e3 - 2.9e4 x (head).

What it found.  The head's dW | db contraction was ONE accumulator chain over every row of the batch; at 262,146 rows the dense pass
missed kappa (1.10 x on the trunk's weight_v gradient of the dgrad head, 2.83 x on a bias gradient of the offsets head): a chain that
adds the same few addends to an ever larger partial sum rounds them the same way every time, which the rule "n products in any
order" (independent roundings) does not cover.  csrc/headtrain.hip now contracts in row blocks of 4,096 rows and adds the blocks'
partials in ascending order; batches of up to 4,096 rows are one block and keep their bits.

Measured on an MI355X (pytest -s prints every figure), largest |gpu - ref64| / kappa: the pool 0.0100 (Y, BiLSTM), 0.0064 (dH), 0.060 (a
head gradient); dense gradients 5e-5 (BiLSTM), 0.0123 (attention), 0.053 / 0.069 (dgrad / offsets head); sparse passes 0.0001, 0.0007,
0.091; parameters after one Adam step 0.0047, 0.0047, 0.049.  Every per-frame output of every pass has the pool's bits, no element is
left out as tiny.  The device lies 10.0 - 10.3 x kappa from the dense controls and 10.1 - 17.5 x (BiLSTM), 13.7 - 16.3 x (attention),
2.6e4 - 2.9e4 x (head) from the S_blocks controls.  Held on the device: 4.0 / 4.8 GiB (BiLSTM layer 0 / 1), 11.6 GiB (attention), 6.6 / 3.3
GiB (heads).  Broken copies of the library turn it red: a reduce that stops one block early only at large batches, and a products
kernel that reads the row block before its own for blk >= 64, pass the dense pass and fail the S_edges gradients at 2.6 - 22 x kappa
(BiLSTM, attention) and 163 - 4.6e3 x (head).  A case takes 0.3 - 2.6 s (the first of a variant makes its float64 pool model), the module 11 s.

The frequency LSTM, measured on an MI355X.  IT STAYS INSIDE KAPPA AT 2,048 FRAMES; nothing in csrc/freqtrain.hip was changed.  Largest
|gpu - ref64| / kappa: the pool 0.0053 (X0), 0.0024 (dC), 0.070 (a gradient); dense gradients 0.0044 (N = 2,048) and 0.0049 (1,033);
sparse passes 0.0166 and 0.0140 (S_edges), 0.0206 and 0.0156 (S_blocks, one pass of 256 and 130 frames); parameters after one Adam step
0.0385 and 0.0401.  Every frame's X0 and dC of every pass has the pool's bits, no element is left out as tiny, dC is exactly zero
off S.  The device lies 10.5 x (N = 2,048) and 47.3 x (1,033) kappa from both dense controls (the last 4 frames lost, counted twice),
134 and 322 x from a pass of S_blocks with a frame left out, 113 and 130 x from one with a frame read from 1,024 frames earlier.  Held:
33.07 and 16.93 GiB.  A case takes 2.7 s (N = 2,048, with the float64 pool model; 1.0 s of it on the device passes and comparisons)
and 0.6 s (N = 1,033).  Broken copies of the library, every access of each inside the workspace, turn both cases red:
    freqtrain_reduce_kernel stopping one partial early when nblk >= 128     the dense pass's gradients (part b), _proj.weight at 16.4 x
                                                                            kappa (N = 2,048, 1,856,188 elements) and 11.0 x (1,033)
    products taking r0 from blk - 1 for blk >= 128                          the dense pass's gradients (part b), _proj.weight at 6.3 x
                                                                            kappa (N = 2,048, 788,449 elements) and 25.9 x (1,033)
    the dC tiles reading GatesCat's second direction from the first         the dense pass's dC bits (part b): 264,241,152 elements
    (dstride taken as 0) from the gate float offset g0 * 512 = 2^25 on,     differ at N = 2,048 (every element from frame 32 on),
    frame 32 (g0, the pair index, never reaches 2^25: it ends at 2^22)      131,203,072 at N = 1,033
Unlike the other three trainers, whose dense pass lets the first two pass, this trainer's dbp and dWp sum exact incoming gradients
and have a kappa of 2e-4 and 9e-4 of the gradient: one lost or repeated row block of 256 or 130 is seen by the dense pass itself."""
import gc
import time

import numpy as np
import pytest
import torch

import bigbatch_ref64 as BB
import freqtrain_ref64 as FT
import headtrain_ref64 as HD

pytestmark = pytest.mark.gpu

CASES = [(v, N) for v, d in BB.VARIANTS.items() for N in d["N"]]
SLICE = {"freq": 256}                 # frames of one bit comparison on the device: 1,024, and 256 for the frequency LSTM, whose frame's
                                      # dC is 512 KiB (a slice of the expected dC and its scaled copy are 256 MiB)
MEMORY_CAP = {("freq", 2048): 34 * 2 ** 30, ("freq", 1033): 18 * 2 ** 30}      # bytes a case may hold on the device: 12 GiB, but for these
P = BB.POOL


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Lstm:
    fwd_names, bwd_name = ("Y",), "dX"

    def __init__(self, variant):
        from sdfa_amd.lstmtrain import LstmTrainer
        c = BB.pool_case(variant)
        self.params = c["params"]
        self.tr = LstmTrainer(c["params"], layer=c["layer"])
        self.fin, self.bin = (dev(c["X"]),), dev(c["dY"])
        self.ref = BB.pool_of(variant)["run"]

    def forward(self, X):
        return (self.tr.forward(X),)

    def backward(self, dY):
        return self.tr.backward(dY)


class Attn:
    fwd_names, bwd_name = ("z", "align"), "dH"

    def __init__(self, variant):
        from sdfa_amd.attntrain import AttnTrainer
        c = BB.pool_case(variant)
        self.params = c["params"]
        self.tr = AttnTrainer(c["params"])
        self.fin, self.bin = (dev(c["H"]),), dev(c["dz"])
        self.ref = BB.pool_of(variant)["run"]

    def forward(self, H):
        return self.tr.forward(H)

    def backward(self, dz):
        return self.tr.backward(dz)


class Head:
    fwd_names, bwd_name = ("coef",), "dz"

    def __init__(self, variant):
        from sdfa_amd.headtrain import HeadTrainer
        c = BB.pool_case(variant)                              # 8 rows: the pool and one more, an even batch
        self.params = c["params"]
        self.tr = HeadTrainer(c["params"], c["head"])
        self.fin, self.bin = (dev(c["z"]), dev(c["sid"])), dev(c["dcoef"])
        self.ref = HD.run(c["head"], c["params"], c["z"], c["sid"], c["dcoef"])

    def forward(self, z, sid):
        return (self.tr.forward(z, sid, check_ids=False),)

    def backward(self, dcoef):
        return self.tr.backward(dcoef)


class Freq:
    fwd_names, bwd_name = ("X0",), "dC"

    def __init__(self, variant):
        from sdfa_amd.freqtrain import FreqTrainer
        c = BB.pool_case(variant)                              # 7 frames of 64 columns, shaped as tests/test_gpu_freqtrain.py shapes them
        self.params = c["params"]
        self.tr = FreqTrainer(c["params"])
        self.fin, self.bin = (dev(c["C"].reshape(P, FT.COLS, FT.NS, FT.NI)),), dev(c["dX0"].reshape(P, FT.COLS, FT.NO))
        self.ref = BB.pool_of(variant)["run"]

    def forward(self, C4):
        return (self.tr.forward(C4),)

    def backward(self, dX3):
        return self.tr.backward(dX3, want_dC=True)


KINDS = {"lstm": Lstm, "attn": Attn, "head": Head, "freq": Freq}


def ratio(what, got, val, kap, worst):
    d = np.abs(np.asarray(got, np.float64).reshape(val.shape) - val)
    assert np.isfinite(d).all(), what
    r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), r)
    bad = d > kap
    assert not bad.any(), (what, int(bad.sum()), r, float(d.max()))


def grads_within(what, got, model, worst):
    for n, g in model["grads"].items():
        ratio(f"{what}:{n}", got[n], g, model["k_grads"][n], worst)


def away(got, wrong, right):
    """the largest |device gradient - wrong model| / (right model's kappa)"""
    worst = 0.0
    for n, g in wrong["grads"].items():
        kap = right["k_grads"][n]
        d = np.abs(np.asarray(got[n], np.float64).reshape(g.shape) - g)
        worst = max(worst, float((d[kap > 0] / kap[kap > 0]).max(initial=0.0)))
    return worst


def bits(t):
    return t.contiguous().view(torch.int32)


def scaled(pool, w):
    return pool * w.view((-1,) + (1,) * (pool.dim() - 1))


def frames_have_pool_bits(got, pool, jd, wd=None, frames=None, SLICE=1024):
    """-> (elements of `got` whose bits are not the pool frame's (times the frame's weight), elements left out as tiny); frames:
    the frames compared (all of them by default).  On the device, SLICE frames at a time."""
    tiny = (pool != 0) & (pool.abs() < BB.TINY) if wd is not None else None
    idx = torch.arange(len(got), device=got.device) if frames is None else frames
    bad = torch.zeros((), dtype=torch.int64, device=got.device)
    out = torch.zeros((), dtype=torch.int64, device=got.device)
    for s in range(0, len(idx), SLICE):
        f = idx[s:s + SLICE]
        want = pool[jd[f]]
        g = got[s:s + SLICE] if frames is None else got[f]
        ne = bits(g) != bits(want if wd is None else scaled(want, wd[f]))
        if tiny is not None:
            skip = tiny[jd[f]]
            out += skip.sum()
            ne &= ~skip
        bad += ne.sum()
    return int(bad), int(out)


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


def same_bits(a, b):
    return all((a[n].view(np.uint32) == b[n].view(np.uint32)).all() for n in a)


@pytest.mark.parametrize("variant,N", CASES, ids=[f"{v}-N{n}" for v, n in CASES])
def test_largest_batches_against_float64(variant, N):
    try:
        largest_batch(variant, N)
    finally:
        gc.collect()
        torch.cuda.empty_cache()


def largest_batch(variant, N):
    v = BB.VARIANTS[variant]
    ad = KINDS[variant.partition("-")[0]](variant)
    tr, names = ad.tr, ad.fwd_names + (ad.bwd_name,)
    SL, cap = SLICE.get(variant, 1024), MEMORY_CAP.get((variant, N), 12 * 2 ** 30)
    t0 = time.perf_counter()
    say = lambda s: print(f"\n{variant} N = {N}: {s}")

    # (a) the pool alone against the ref module's float64 run
    def pool_pass():
        out = ad.forward(*ad.fin) + (ad.backward(ad.bin),)
        return out, tr.grads()

    pool_out, pool_grads = pool_pass()
    worst = {}
    for n, t in zip(names, pool_out):
        ratio(n, t.cpu().numpy(), ad.ref[n], ad.ref["k_" + n], worst)
    grads_within("grad", pool_grads, ad.ref, worst)
    say(f"the pool at N = {len(ad.bin)}, largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {r:.4f}" for k, r in worst.items()))
    pool_fwd, pool_bwd = [t[:P] for t in pool_out[:-1]], pool_out[-1][:P]

    # the periodic batch, gathered on the device
    j, k, S_edges, S_blocks = BB.sets(variant, N)
    model = BB.model_of(variant, N)
    jd, wd = dev(j), dev((2.0 ** k).astype(np.float32))
    fin = tuple(t[:P][jd] for t in ad.fin)
    bin_dense = scaled(ad.bin[:P][jd], wd)
    ws_bytes = tr.workspace_bytes(N)
    slices = 4 * SL * pool_bwd[0].numel() * 4                  # a slice of the expected dX, its scaled copy, the comparison
    total = pool_bwd[0].numel() * N

    def large_pass(b, what):
        out = ad.forward(*fin) + (ad.backward(b),)
        held = ws_bytes + nbytes(*fin, bin_dense, b if b is not bin_dense else None, *out) + slices
        assert tr._ws.numel() == ws_bytes and held < cap, (what, held)
        return out, held

    # (b) the dense pass
    out, held = large_pass(bin_dense, "dense")
    for n, t, p in zip(names, out, pool_fwd):
        bad, _ = frames_have_pool_bits(t, p, jd, SLICE=SL)
        assert bad == 0, (n, bad)
    bad, left_out = frames_have_pool_bits(out[-1], pool_bwd, jd, wd, SLICE=SL)
    assert bad == 0 and left_out <= BB.TINY_SHARE * total, (ad.bwd_name, bad, left_out)
    del out
    g_dense = tr.grads()
    right, wrong = BB.dense_controls(model, j, k, N, v["tile"], v["dense_tiles"])
    worst = {}
    grads_within("grad", g_dense, right, worst)
    say(f"dense pass, {held / 2 ** 30:.2f} GiB on the device, every frame's " + ", ".join(names) + f" bit for bit ({left_out} tiny elements left out); "
        f"largest |gpu - ref64| / kappa on a gradient {worst['grad']:.4f}")
    for what, w in wrong.items():
        r = away(g_dense, w, right)
        say(f"dense pass, {what}: the device lies {r:.3g} x kappa from this wrong model")
        assert r > 1.0, (what, r)

    # (c) the sparse passes
    sparse = [("S_edges", S_edges, False)] + [(f"S_blocks pass {g}", S, True) for g, S in enumerate(BB.passes(S_blocks, v["groups"]))]
    worst, nearest = {}, {}
    for what, S, controls in sparse:
        Sd = dev(S)
        b = torch.zeros_like(bin_dense)
        b[Sd] = bin_dense[Sd]
        out, held_s = large_pass(b, what)
        held = max(held, held_s)
        dX = out[-1]
        off_S = torch.ones(N, dtype=torch.bool, device=dX.device)
        off_S[Sd] = False
        not_zero = torch.cat([(dX[s:s + SL].reshape(len(dX[s:s + SL]), -1) != 0).any(1) for s in range(0, N, SL)])
        assert not bool(not_zero[off_S].any()), f"{what}: {ad.bwd_name} is not zero off S"
        bad, left = frames_have_pool_bits(dX, pool_bwd, jd, wd, Sd, SLICE=SL)
        assert bad == 0 and left <= BB.TINY_SHARE * total, (what, bad, left)
        del out, dX, b
        got = tr.grads()
        if controls:
            right_s, wrong_s, _ = BB.block_controls(model, j, k, S, v["off"])
        else:
            right_s, wrong_s = model(keep=S, step=False), {}
        assert right_s["frames"] == len(S)
        grads_within(what.split(" pass")[0], got, right_s, worst)
        for name, w in wrong_s.items():
            r = away(got, w, right_s)
            key = "left out" if "left out" in name else f"read from {v['off']} frames earlier"
            nearest[key] = min(nearest.get(key, np.inf), r)
            assert r > 1.0, (what, name, r)
    say(f"sparse passes ({len(S_edges)} frames of S_edges; {len(S_blocks)} of S_blocks in {v['groups']} passes), largest |gpu - ref64| / kappa on a gradient: "
        + ", ".join(f"{k_} {r:.4f}" for k_, r in worst.items())
        + "; the device lies at least " + ", ".join(f"{r:.3g} x kappa from a model with a frame {k_}" for k_, r in nearest.items()))

    # (d) the pool again on the grown workspace, then the dense pass again, and one Adam step
    ws = tr._ws
    again_out, again_grads = pool_pass()
    assert tr._ws is ws and ws.numel() == ws_bytes
    for n, a, b in zip(names, again_out, pool_out):
        assert torch.equal(bits(a), bits(b)), n
    assert same_bits(again_grads, pool_grads)
    del again_out
    out, _ = large_pass(bin_dense, "dense again")
    del out
    assert same_bits(tr.grads(), g_dense)
    tr.step()
    params, worst = tr.parameters(), {}
    for n in right["params1"]:
        ratio(f"param:{n}", params[n], right["params1"][n], right["k_params1"][n], worst)
    say(f"the pool's bits again after the large passes; the dense pass's gradient bits again; after one Adam step the largest "
        f"|gpu - ref64| / kappa on a parameter {worst['param']:.4f}; at most {held / 2 ** 30:.2f} GiB held; the case took "
        f"{time.perf_counter() - t0:.1f} s")
