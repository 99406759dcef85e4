"""The attention layer's training step on the device (csrc/attntrain.hip, include/sdfa_attntrain.h) against the float64 model of
tests/attntrain_ref64.py on its seeded cases, both families ("flat": Glorot-sized, largest align about 0.05; "peaked": largest
align above 0.5 in at least half the frames): z, align, dH, every gradient element, the parameters after one step, and the
parameters and both Adam moments after three steps on the same batch, each within 1 x kappa (where kappa is 0 the value must be
exact).  kappa is derived in attntrain_ref64.py and pinned on the CPU (tests/test_attntrain_ref64_cpu.py); nothing here is
fitted, and no constant factor is applied.

Shapes.  N = 1: the smallest batch, one row block.  N = 2.  N = 100: the reference's 2 x 50; seven row blocks of dWk, the last one
of 4 frames; the dWc / dWq contraction over n ends inside a chunk (100 = 64 + 36).  N = 40 = 2 x BLOCK_FRAMES + 8 with
BLOCK_FRAMES = 16 (SDFA_ATTNTRAIN_BLOCK_FRAMES): three partial blocks of the dWk / dv / db split, the last one ragged.

Further: each wrong model of attntrain_ref64.FLAWS lies more than 1 x kappa from the device somewhere; Adam alone on gradients
set by hand (exact zeros, 1e-12, 1e-8 = eps, 1e4) within its kappa, zero-gradient elements bit for bit unchanged; two runs give
the same bits; the first 100 frames of a larger batch give the same z, align and dH bits; a null d_dH changes no other output; a
workspace poisoned with NaN past what the call writes changes nothing; the refusals hold with real buffers.

sdfa_encoder_memory: z and align are bitwise sdfa_encoder_forward's, H is bitwise debug tap 3 of a keep-intermediates engine on
the same input -- at 72 frames, inside one workspace chunk, and at 200 frames on an engine whose workspace holds one 128-frame
chunk (the smallest the engine accepts), which crosses a chunk boundary.

From the second step on kappa of a parameter is vacuous wherever the first gradient's kappa reaches the gradient itself (Adam
divides by sqrt(v)): the three-step comparison is kept because it also catches NaN and a wrong step count, the one-step
comparison and Adam alone carry the optimiser's check.

Measured on an MI355X (pytest -s prints every figure): the largest |gpu - ref64| / kappa is 0.0017 on z, 0.0043 on align, 0.0090 on
dH (all peaked, N = 100), 0.0025 on a gradient (proj_qry, peaked N = 1), 0.0080 on a parameter after one step; the reference's own
float32 run needs 0.007 x kappa on the fixture: the rules (sqrt(n + 1) U sum |a b| per sum, linear addition over the rows, LAMBDA) are
loose for this layer, and no factor is applied either way.  The controls lie 54 (taps reversed) to 3.7e10 (window at 30) x kappa from
the device, Adam without bias correction 32 (2.5e5 on set gradients); Adam alone 0.122.  The module takes 11 s."""
import functools

import numpy as np
import pytest
import torch

import attntrain_ref64 as R

pytestmark = pytest.mark.gpu

BLOCK_FRAMES = 16                                   # SDFA_ATTNTRAIN_BLOCK_FRAMES
N_THREE_BLOCKS = 2 * BLOCK_FRAMES + 8               # 40 <= 320: blocks of 16, 16 and 8 frames
SHAPES = [(family, N) for family in R.FAMILIES for N in (1, 2, 100, N_THREE_BLOCKS)]
STEPS = 3


@functools.lru_cache(maxsize=None)
def case(family, N):
    return R.case(N, 200 + N + (0 if family == "flat" else 1000), family)


@functools.lru_cache(maxsize=None)
def model(family, N):
    return R.train_steps(case(family, N), STEPS)


@functools.lru_cache(maxsize=None)
def model1(family, N):
    return R.train_steps(case(family, N), 1)


def trainer(c):
    from sdfa_amd.attntrain import AttnTrainer
    return AttnTrainer(c["params"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def one_pass(tr, c, frames=None, want_dH=True):
    sl = slice(None, frames)
    z, align = tr.forward(dev(c["H"][sl]))
    dH = tr.backward(dev(c["dz"][sl]), want_dH=want_dH)
    return z, align, dH


@functools.lru_cache(maxsize=None)
def device(family, N):
    """z, align, dH, first-step gradients, parameters after one step, and parameters / moments after STEPS steps, as numpy"""
    c = case(family, N)
    tr = trainer(c)
    out = {}
    for t in range(STEPS):
        z, align, dH = one_pass(tr, c)
        if t == 0:
            out.update(z=z.cpu().numpy(), align=align.cpu().numpy(), dH=dH.cpu().numpy(), grads=tr.grads())
        tr.step()
        if t == 0:
            out["params1"] = tr.parameters()
    out["params"] = tr.parameters()
    out["exp_avg"], out["exp_avg_sq"] = tr.moments()
    assert tr.step_count == STEPS
    return out


def ratio(what, got, val, kap, worst):
    d = np.abs(np.asarray(got, np.float64).reshape(val.shape) - val)
    assert np.isfinite(d).all(), what
    r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), r)
    bad = d > kap
    assert not bad.any(), (what, int(bad.sum()), r, float(d.max()))


@pytest.mark.parametrize("family,N", SHAPES, ids=[f"{f}-N{n}" for f, n in SHAPES])
def test_step_within_kappa(family, N):
    p, m, v, kp, km, kv, first = model(family, N)
    p1, _, _, kp1, _, _, _ = model1(family, N)
    got = device(family, N)
    worst = {}
    for what in ("z", "align", "dH"):
        ratio(what, got[what], first[what], first["k_" + what], worst)
    n_el = 0
    for n in first["grads"]:
        kind = n.rsplit(".10.", 1)[1]
        ratio(f"grad {kind}:{n}", got["grads"][n], first["grads"][n], first["k_grads"][n], worst)
        ratio(f"param1 {kind}:{n}", got["params1"][n], p1[n], kp1[n], worst)
        ratio(f"param3 {kind}:{n}", got["params"][n], p[n], kp[n], worst)
        ratio(f"exp_avg {kind}:{n}", got["exp_avg"][n], m[n], km[n], worst)
        ratio(f"exp_avg_sq {kind}:{n}", got["exp_avg_sq"][n], v[n], kv[n], worst)
        n_el += first["grads"][n].size
    print(f"\n{family} N = {N}: {n_el} gradient elements, largest align {first['align'].max():.3f}; largest |gpu - ref64| / kappa: "
          + ", ".join(f"{k} {r:.4f}" for k, r in worst.items()))


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_outside_kappa_of_the_device(flaw):
    family, N = "peaked", N_THREE_BLOCKS
    c, got = case(family, N), device(family, N)
    worst = 0.0
    if flaw == "no_bias_correction":
        right = model1(family, N)
        wp = R.train_steps(c, 1, flaw=flaw)[0]
        for n in wp:
            worst = max(worst, float((np.abs(got["params1"][n].astype(np.float64) - wp[n]) / np.maximum(right[3][n], 1e-300)).max()))
    else:
        first = model(family, N)[6]
        w = R.run(c["params"], c["H"], c["dz"], flaw=flaw)
        for what in ("z", "align", "dH"):
            worst = max(worst, float((np.abs(got[what] - w[what]) / np.maximum(first["k_" + what], 1e-300)).max()))
        for n in w["grads"]:
            worst = max(worst, float((np.abs(got["grads"][n].astype(np.float64) - w["grads"][n]) / np.maximum(first["k_grads"][n], 1e-300)).max()))
    print(f"\n{flaw}: the device lies {worst:.3g} x kappa from this wrong model")
    assert worst > 1.0, (flaw, worst)


def test_adam_alone_on_set_gradients():
    c = case("flat", 1)
    tr = trainer(c)
    rs = np.random.RandomState(5)
    special = np.asarray([0.0, 1e-12, 1e-8, 1e4, -1e-12, -1e-8, -1e4, 0.0], np.float32)
    grads, state = {}, {}
    for n, a in c["params"].items():
        g = (rs.normal(0, 1e-3, a.shape)).astype(np.float32)
        flat = g.reshape(-1)
        flat[:flat.size // 2] = np.resize(special, flat.size // 2)
        grads[n] = g
        state[n] = (np.asarray(a, np.float64), np.zeros(a.shape), np.zeros(a.shape), 0.0, 0.0, 0.0)
    worst = 0.0
    wrong = 0.0
    for t in (1, 2, 3):
        tr.set_grads(grads)
        tr.step()
        params = tr.parameters()
        m, v = tr.moments()
        for n in grads:
            p0, m0, v0, kp0, km0, kv0 = state[n]
            if t == 1:
                flawed = R.adam(p0, grads[n], m0, v0, t, flaw="no_bias_correction")[0]
            state[n] = R.adam(p0, grads[n], m0, v0, t, ep=kp0, em=km0, ev=kv0)
            if t == 1:
                wrong = max(wrong, float((np.abs(params[n].astype(np.float64) - flawed) / np.maximum(state[n][3], 1e-300)).max()))
            for got, val, kap in ((params[n], state[n][0], state[n][3]), (m[n], state[n][1], state[n][4]), (v[n], state[n][2], state[n][5])):
                d = np.abs(got.astype(np.float64) - val)
                assert (d <= kap).all(), (n, t, float((d / np.maximum(kap, 1e-300)).max()))
                worst = max(worst, float((d[kap > 0] / kap[kap > 0]).max()))
    for n in grads:
        zero = grads[n] == 0
        assert zero.any() and (params[n][zero].view(np.uint32) == c["params"][n][zero].view(np.uint32)).all(), n
        assert (m[n][zero] == 0).all() and (v[n][zero] == 0).all()
        assert (params[n][~zero] != c["params"][n][~zero]).mean() > 0.5, n
    print(f"\nAdam alone, three steps: largest |gpu - ref64| / kappa {worst:.4f}; without bias correction the first step lies {wrong:.3g} x kappa away")
    assert wrong > 1.0, wrong


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all()


def test_same_inputs_same_bits_and_frames_do_not_depend_on_the_batch():
    c = case("peaked", 132)
    a, b = trainer(c), trainer(c)
    za, aa, dHa = one_pass(a, c)
    zb, ab, dHb = one_pass(b, c)
    assert torch.equal(za, zb) and torch.equal(aa, ab) and torch.equal(dHa, dHb)
    ga, gb = a.grads(), b.grads()
    for n in ga:
        assert same_bits(ga[n], gb[n]), n
    # the first 100 frames alone: the same z, align and dH bits
    zc, ac, dHc = one_pass(b, c, 100)
    assert torch.equal(zc, za[:100]) and torch.equal(ac, aa[:100]) and torch.equal(dHc, dHa[:100])
    gc = b.grads()
    assert any(not same_bits(gc[n], ga[n]) for n in ga)       # the gradients do sum over the batch


def test_null_dH_changes_no_other_output():
    c = case("peaked", N_THREE_BLOCKS)
    a, b = trainer(c), trainer(c)
    za, aa, dHa = one_pass(a, c)
    zb, ab, dHb = one_pass(b, c, want_dH=False)
    assert dHa is not None and dHb is None
    assert torch.equal(za, zb) and torch.equal(aa, ab)
    ga, gb = a.grads(), b.grads()
    for n in ga:
        assert same_bits(ga[n], gb[n]), n


def test_poisoned_workspace_is_never_read():
    c = case("flat", N_THREE_BLOCKS)
    clean = trainer(c)
    z, align, dH = one_pass(clean, c)
    tr = trainer(c)
    ws = torch.full((tr.workspace_bytes(300) // 4,), float("nan"), dtype=torch.float32, device="cuda").view(torch.uint8)
    tr._ws = ws
    zp, alignp, dHp = one_pass(tr, c)
    assert tr._ws is ws
    assert torch.equal(z, zp) and torch.equal(align, alignp) and torch.equal(dH, dHp)
    gc, gp = clean.grads(), tr.grads()
    for n in gc:
        assert same_bits(gc[n], gp[n]), n


def test_refusals_with_real_buffers():
    from sdfa_amd import _lib
    from sdfa_amd._lib import SdfaError, lib
    from sdfa_amd._packed import ptr, stream
    c = case("flat", N_THREE_BLOCKS)
    N = N_THREE_BLOCKS
    tr = trainer(c)
    H, dz = dev(c["H"]), dev(c["dz"])
    with pytest.raises(SdfaError):
        tr.backward(dz)                                      # no forward yet
    z, align = tr.forward(H)
    with pytest.raises(SdfaError) as e:
        tr.backward(dz[:N - 2])                              # not the forward's N
    assert "no forward" in str(e.value)
    need = tr.workspace_bytes(N)
    args = (ptr(z), ptr(align))
    assert lib.sdfa_attntrain_forward(tr._h, ptr(H), N, *args, ptr(tr._ws), need - 1, stream()) == _lib.EINVAL
    assert b"workspace" in lib.sdfa_last_error()
    assert lib.sdfa_attntrain_forward(tr._h, ptr(H), N, *args, tr._ws.data_ptr() + 4, need, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_forward(tr._h, None, N, *args, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_forward(tr._h, ptr(H), N, None, ptr(align), ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_forward(tr._h, ptr(H), 0, *args, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_forward(tr._h, ptr(H), 32769, *args, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_backward(tr._h, ptr(H), None, N, None, ptr(tr._ws), need, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_adam(tr._h, -1.0, 0.9, 0.999, 1e-8, stream()) == _lib.EINVAL
    assert lib.sdfa_attntrain_adam(tr._h, 1e-4, 1.0, 0.999, 1e-8, stream()) == _lib.EINVAL
    a = np.zeros(128, np.float32)
    assert lib.sdfa_attntrain_set_tensor(tr._h, R.V.encode(), a.ctypes.data, a.size) == _lib.ESTATE
    # a refused call changes nothing: the earlier forward still stands
    assert tr.backward(dz, want_dH=False) is None
    tr.step()
    with pytest.raises(SdfaError):
        tr.backward(dz)                                      # the kept activations belong to the old parameters


# ---------------------------------------------------------------------------------------------------- sdfa_encoder_memory
@pytest.mark.parametrize("n_frames", [72, 200], ids=["one-chunk", "across-chunks"])
def test_encoder_memory_is_the_encoder_and_debug_tap_3(synth_sd, n_frames):
    from sdfa_amd import ops, synth
    from sdfa_amd.engine import Engine
    sd = synth_sd["offsets"]
    eng = Engine(sd, device="cuda:0", max_frames=128)        # a workspace of one 128-frame chunk: 200 frames take two
    pcm = synth.make_pcm(1, 16000 * n_frames // 60)         # more than n_frames frames (about 120 a second)
    feat, _, _ = eng.mel_frontend([pcm], 16000)
    feat = feat[:n_frames].contiguous()
    assert feat.shape[0] == n_frames
    z0, align0 = eng.encoder(feat)
    H, z, align = eng.encoder_memory(feat)
    assert torch.equal(z, z0) and torch.equal(align, align0)
    H_only, z_none, align_none = eng.encoder_memory(feat, want_z=False, want_align=False)
    assert z_none is None and align_none is None and torch.equal(H_only, H)
    keep = Engine(sd, device="cuda:0", max_frames=256, debug_keep=True)
    taps = []
    for f0 in range(0, n_frames, 128):                       # the tap reads one chunk's workspace
        part = feat[f0:f0 + 128].contiguous()
        keep.encoder(part)
        taps.append(keep.tap(3, part.shape[0]).clone())
    tap = torch.cat(taps).reshape(n_frames, 64, 512)
    assert torch.equal(H, tap)
    assert float(H.abs().max()) <= 1.0 and float(H.abs().mean()) > 1e-3
    Ho, zo, ao = torch.ops.sdfa.encoder_memory(feat, ops.register_model(None, eng))
    assert torch.equal(Ho, H) and torch.equal(zo, z) and torch.equal(ao, align)
