"""The conv stack's training step on the device (csrc/convtrain.hip, include/sdfa_convtrain.h) against the float64 model of
tests/convtrain_ref64.py on its seeded cases, both families ("default"; "edge": negative BatchNorm scales, an all-zero column, a
constant column, zero biases, a tiny running_var, energy at the borders): C, every gradient element and every parameter after one
Adam step within 1 x kappa (where kappa is 0 the value must be exact).  kappa is derived in convtrain_ref64.py and pinned on the
CPU (tests/test_convtrain_ref64_cpu.py); nothing here is fitted, and no constant factor is applied.

Shapes.  N = 1: the smallest batch, a partial row block.  N = 2.  N = 9 = BLOCK_FRAMES + 1: a whole row block and one of a single
frame, a two-deep reduce.

Further: each wrong model of convtrain_ref64.FLAWS lies more than 1 x kappa from the device somewhere, at N = 1 and at N = 2; on
the "edge" family the all-zero column's C has the same bits along every interior frequency row, and with dC confined to that column
the gradients follow the first-row rule and not the second-row one; two runs give the same bits; a frame's C has the same bits at
N = 1 and inside N = 2; a workspace poisoned with NaN changes nothing; the running statistics keep their bits across Adam steps and
ride in the resumable state, which a trainer with other statistics refuses;
the refusals hold with real buffers.  pytest -s prints every figure and the ambiguity counts, which
tests/test_convtrain_ref64_cpu.py holds under 1e-3 of each layer's elements for these very cases.

Measured on an MI355X: the largest |gpu - ref64| / kappa is 0.049 on C (edge, N = 9), 0.075 on a gradient (layer 5's bias, edge, N = 2)
and 0.103 on a parameter after one step (layer 5's BatchNorm bias, edge, N = 1); the controls lie 7.7 (slope 1 at a == 0, N = 2) to 2.3e5 (wrapped padding)
x kappa from the device; the zero column alone: first-row rule 0.010, second-row rule 852 x kappa.  The module takes 6 s."""
import functools

import numpy as np
import pytest
import torch

import convtrain_ref64 as R

pytestmark = pytest.mark.gpu

BLOCK_FRAMES = 8                                    # SDFA_CONVTRAIN_BLOCK_FRAMES
SHAPES = [(family, N) for family in R.FAMILIES for N in (1, 2, BLOCK_FRAMES + 1)]


@functools.lru_cache(maxsize=None)
def case(family, N):
    return R.case(R.COLS * N, 700 + N + (0 if family == "default" else 5000), family)


@functools.lru_cache(maxsize=None)
def model(family, N):
    return R.train_steps(case(family, N), 1)


def trainer(c, **kw):
    from sdfa_amd.convtrain import ConvTrainer
    return ConvTrainer(c["params"], **kw)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def feat_of(c, frames=None):
    return dev(c["feat"].reshape(-1, R.COLS, R.BINS, R.IN)[:frames])


def dC_of(c, frames=None):
    return dev(c["dC"].reshape(-1, R.COLS, R.OUT_BINS, R.OUT)[:frames])


def one_pass(tr, c, frames=None, dC=None):
    feat = feat_of(c, frames)
    Cout = tr.forward(feat)
    tr.backward(feat, dC_of(c, frames) if dC is None else dC)
    return Cout


@functools.lru_cache(maxsize=None)
def device(family, N):
    c = case(family, N)
    tr = trainer(c)
    Cout = one_pass(tr, c)
    out = dict(C=Cout.cpu().numpy().reshape(-1, R.OUT_BINS, R.OUT), grads=tr.grads())
    tr.step()
    out["params1"] = tr.parameters()
    assert tr.step_count == 1
    return out


def ratio(what, got, val, kap, worst):
    d = np.abs(np.asarray(got, np.float64).reshape(val.shape) - val)
    assert np.isfinite(d).all(), what
    r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), r)
    bad = d > kap
    assert not bad.any(), (what, int(bad.sum()), r, float(d.max()))


def counts(first):
    return {L: (first["ambiguous_kink"][L], first["ambiguous_pool"][L], first["ties"][L], first["elements"][L]) for L in first["elements"]}


@pytest.mark.parametrize("family,N", SHAPES, ids=[f"{f}-N{n}" for f, n in SHAPES])
def test_step_within_kappa(family, N):
    p, m, v, kp, km, kv, first = model(family, N)
    got = device(family, N)
    print(f"\n{family} N = {N}: per layer (ambiguous kink, ambiguous pool route, decided ties, elements) {counts(first)}")
    worst = {}
    ratio("C", got["C"], first["C"], first["k_C"], worst)
    for n in first["grads"]:
        kind = n[len(R.P):]
        ratio(f"grad {kind}:{n}", got["grads"][n], first["grads"][n], first["k_grads"][n], worst)
        ratio(f"param1 {kind}:{n}", got["params1"][n], p[n], kp[n], worst)
    print(f"{family} N = {N}: largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {r:.4f}" for k, r in worst.items()))


def distance(got, w, first, kp, params1=None):
    worst = 0.0
    if params1 is not None:
        for n in params1:
            worst = max(worst, float((np.abs(got["params1"][n].astype(np.float64) - params1[n]) / np.maximum(kp[n], 1e-300)).max()))
        return worst
    worst = float((np.abs(got["C"] - w["C"]) / np.maximum(first["k_C"], 1e-300)).max())
    for n in w["grads"]:
        worst = max(worst, float((np.abs(got["grads"][n].astype(np.float64) - w["grads"][n]) / np.maximum(first["k_grads"][n], 1e-300)).max()))
    return worst


@pytest.mark.parametrize("N", (1, 2))
@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_outside_kappa_of_the_device(flaw, N):
    c, got = case("edge", N), device("edge", N)
    p, m, v, kp, km, kv, first = model("edge", N)
    if flaw == "no_bias_correction":
        wp = R.train_steps(c, 1, flaw=flaw)[0]
        worst = distance(got, None, first, kp, {n: wp[n] for n in R.names()})
    else:
        worst = distance(got, R.run(c["params"], c["feat"], c["dC"], flaw=flaw), first, kp)
    print(f"\n{flaw}, N = {N}: the device lies {worst:.3g} x kappa from this wrong model")
    assert worst > 1.0, (flaw, worst)


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all()


def test_zero_column_ties_exactly_and_routes_to_the_first_row():
    c = case("edge", 1)
    assert not c["feat"][0].any()
    Cz = device("edge", 1)["C"][0]                           # column 0: [32][64]
    assert same_bits(Cz[1:31], np.broadcast_to(Cz[1], (30, R.OUT))), "the all-zero column's interior rows are one computation"
    assert not same_bits(Cz[0], Cz[1])                       # the padded border does differ
    # dC on that column alone: every pooled pair of it is an exact tie (layer 1) or an interior tie (layer 3)
    dC = np.zeros_like(c["dC"])
    dC[0] = c["dC"][0]
    tr = trainer(c)
    one_pass(tr, c, dC=dev(dC.reshape(1, R.COLS, R.OUT_BINS, R.OUT)))
    g = tr.grads()
    first = R.run(c["params"], c["feat"], dC)
    second = R.run(c["params"], c["feat"], dC, flaw="tie_second")
    assert first["ties"][1] >= 64 * 32 and first["ties"][3] >= 31 * 64
    worst, away = {}, 0.0
    for n in first["grads"]:
        ratio(f"grad:{n}", g[n], first["grads"][n], first["k_grads"][n], worst)
        away = max(away, float((np.abs(g[n].astype(np.float64) - second["grads"][n]) / np.maximum(first["k_grads"][n], 1e-300)).max()))
    print(f"\nzero column alone: first-row rule {worst['grad']:.4f} x kappa, second-row rule {away:.3g} x kappa from the device")
    assert away > 1.0, away


def test_same_inputs_same_bits_and_a_frame_does_not_depend_on_the_batch():
    c = case("edge", 2)
    a, b = trainer(c), trainer(c)
    Ca, Cb = one_pass(a, c), one_pass(b, c)
    assert torch.equal(Ca, Cb)
    ga, gb = a.grads(), b.grads()
    for n in ga:
        assert same_bits(ga[n], gb[n]), n
    C1 = one_pass(b, c, 1)
    assert torch.equal(C1, Ca[:1])
    gc = b.grads()
    assert any(not same_bits(gc[n], ga[n]) for n in ga)       # the gradients do sum over the batch


def test_poisoned_workspace_is_never_read():
    c = case("default", BLOCK_FRAMES + 1)
    clean = trainer(c)
    Cc = one_pass(clean, c)
    tr = trainer(c)
    ws = torch.full((tr.workspace_bytes(BLOCK_FRAMES + 1) // 4,), float("nan"), dtype=torch.float32, device="cuda").view(torch.uint8)
    tr._ws = ws
    Cp = one_pass(tr, c)
    assert tr._ws is ws
    assert torch.equal(Cc, Cp)
    gc, gp = clean.grads(), tr.grads()
    for n in gc:
        assert same_bits(gc[n], gp[n]), n


def test_constants_keep_their_bits_and_are_not_state():
    from sdfa_amd import _lib
    from sdfa_amd._lib import lib
    c = case("default", 1)
    tr = trainer(c)
    for _ in range(2):
        one_pass(tr, c)
        tr.step()
    stats = tr.running_stats()
    assert set(stats) == set(R.constant_names())
    for n, a in stats.items():
        assert same_bits(a, c["params"][n]), n
    moved = tr.parameters()
    assert set(moved) == set(R.names()) and all((moved[n] != c["params"][n]).any() for n in moved)
    assert set(k[len("_model."):] for k in tr.conv_state_dict()) == set(R.names())
    # the resumable state carries the statistics, and a trainer enabled with other ones refuses it by name
    state = tr.state_dict()
    assert set(state["constants"]) == set(R.constant_names())
    assert trainer(c).load_state_dict(state).step_count == 2
    other = dict(c["params"])
    name = R.constant_names()[3]
    other[name] = c["params"][name] + np.float32(0.125)
    with pytest.raises(ValueError, match="taken with another .*" + name.replace(".", r"\.")):
        trainer(dict(c, params=other)).load_state_dict(state)
    with pytest.raises(ValueError, match="carries no running statistics"):
        trainer(c).load_state_dict({k: v for k, v in state.items() if k != "constants"})
    n = R.constant_names()[0].encode()
    a = np.zeros(32, np.float32)
    for what in (1, 2, 3):
        assert lib.sdfa_convtrain_get_tensor(tr._h, n, what, a.ctypes.data, a.size) == _lib.EINVAL
        assert n in lib.sdfa_last_error()
        assert lib.sdfa_convtrain_set_state(tr._h, n, what, a.ctypes.data, a.size) == _lib.EINVAL
    assert lib.sdfa_convtrain_set_state(tr._h, n, 0, a.ctypes.data, a.size) == _lib.EINVAL
    assert lib.sdfa_convtrain_set_grad(tr._h, n, a.ctypes.data, a.size) == _lib.EINVAL
    assert n in lib.sdfa_last_error()


def test_refusals_with_real_buffers():
    from sdfa_amd import _lib
    from sdfa_amd._lib import SdfaError, lib
    from sdfa_amd._packed import ptr, stream
    N = 2
    c = case("default", N)
    tr = trainer(c)
    feat, dC = feat_of(c), dC_of(c)
    with pytest.raises(SdfaError):
        tr.backward(feat, dC)                                # no forward yet
    Cout = tr.forward(feat)
    with pytest.raises(SdfaError) as e:
        tr.backward(feat[:1], dC[:1])                        # not the forward's N
    assert "no forward" in str(e.value)
    need = tr.workspace_bytes(N)
    assert lib.sdfa_convtrain_forward(tr._h, ptr(feat), N, ptr(Cout), ptr(tr._ws), need - 1, stream()) == _lib.EINVAL
    assert b"workspace" in lib.sdfa_last_error()
    assert lib.sdfa_convtrain_forward(tr._h, ptr(feat), N, ptr(Cout), tr._ws.data_ptr() + 4, need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_forward(tr._h, None, N, ptr(Cout), ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_forward(tr._h, ptr(feat), N, None, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_forward(tr._h, ptr(feat), 0, ptr(Cout), ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_forward(tr._h, ptr(feat), 2049, ptr(Cout), ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_backward(tr._h, None, ptr(dC), N, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_backward(tr._h, ptr(feat), None, N, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_adam(tr._h, -1.0, 0.9, 0.999, 1e-8, stream()) == _lib.EINVAL
    assert lib.sdfa_convtrain_adam(tr._h, 1e-4, 1.0, 0.999, 1e-8, stream()) == _lib.EINVAL
    a = np.zeros(32, np.float32)
    assert lib.sdfa_convtrain_set_tensor(tr._h, R.names()[2].encode(), a.ctypes.data, a.size) == _lib.ESTATE
    assert lib.sdfa_convtrain_set_tensor(tr._h, R.constant_names()[0].encode(), a.ctypes.data, a.size) == _lib.ESTATE
    # a refused call changes nothing: the earlier forward still stands
    tr.backward(feat, dC)
    with pytest.raises(SdfaError):
        tr.backward(feat, dC)                                # the backward consumed the kept pre-activations
    tr.forward(feat)
    tr.step()
    with pytest.raises(SdfaError):
        tr.backward(feat, dC)                                # the kept activations belong to the old parameters
