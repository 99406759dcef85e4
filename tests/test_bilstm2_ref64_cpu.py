"""tests/bilstm2_ref64.py -- the float64 model of the masked two-layer BiLSTM step the GPU tests of train_step(bilstm_bottom=True)
compare with -- pinned on the CPU.

With an all-ones mask it is the reference's two-layer torch.nn.LSTM: it reproduces the double run committed in
tests/golden/train_lstm*.npz (every view the fixtures hold of H, of the gradients of both layers and of the parameters after one
and after three Adam steps; dX0 is not formed here: nothing below layer 0 trains) to the 1e-12 relative
tests/test_lstmtrain_ref64_cpu.py asks.  With a seeded Bernoulli
mask it is within 1e-12 relative of torch in double: two single-layer bidirectional nn.LSTM(bias=False) modules with the mask
multiplied in between, autograd and torch.optim.Adam -- the definition of inter-layer dropout given the mask.  Its wrong variants
(bilstm2_ref64.FLAWS) each lie at least 10 x kappa from that torch run on at least one output; the figures are printed per
output.  The ABI of include/sdfa_bilstm.h and the refusal that needs no device.

Measured: ones mask 1.4e-14 relative at most; seeded mask 1.6e-13; the controls 14.9 (the mask left out of the backward), 1.78e3
(applied twice), 55.4 (layer 0 untrained), 3.4e4 (directions swapped) x kappa.  The kappa of the parameters after THREE steps is
vacuous for the two-layer stack (1e25 and more: headtrain_ref64.adam's kappa is unbounded for an element whose gradient lies below
its own kappa, and the next step carries that through both recurrences; lstmtrain_ref64.train_steps on the stack gives the same
figures), so the three-step values are held to torch and the controls clear their margin on first-step outputs.

Without tests/bilstm2_ref64.py and sdfa_amd.bilstmtrain this module fails."""
import os
import re

import numpy as np
import pytest
import torch

import bilstm2_ref64 as B
import lstmtrain_ref64 as R
from gen_golden_train_lstm import CASES, FILES, H_STEPS, ROW_STRIDE, STEPS, inputs

_MEMO = {}
P_KEEP = 0.9


def _fixture(golden):
    if "g" not in _MEMO:
        fx = {}
        for f in FILES:
            g = golden[f]
            fx.update({k: g[k] for k in g.files})
        _MEMO["g"] = fx
    return _MEMO["g"]


def _views(fx, prefix, name, val):
    """[(what, model value, fixture value)] for every view of tensor `name` the fixtures store under `prefix`"""
    out = []
    val = np.asarray(val, np.float64)
    k = f"{prefix}.{name}"
    if k in fx:
        out.append((name, val, fx[k].astype(np.float64)))
    if k + ".steps" in fx:
        out.append((name + ".steps", val[:, list(H_STEPS)], fx[k + ".steps"].astype(np.float64)))
    if k + ".rows" in fx:
        out.append((name + ".rows", val[::ROW_STRIDE], fx[k + ".rows"].astype(np.float64)))
    if k + ".rowsum" in fx:
        out.append((name + ".rowsum", val.sum(1), fx[k + ".rowsum"]))
    if k + ".colsum" in fx:
        out.append((name + ".colsum", val.sum(0), fx[k + ".colsum"]))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_ones_mask_is_the_references_two_layer_double_run(golden, name):
    fx = _fixture(golden)
    c = inputs(name)
    ones = np.ones(c["X"].shape[:2] + (R.NY,), np.float32)
    p3, _, _, _, _, _, first = B.train_steps(c["params"], c["X"], ones, c["dY"], STEPS)
    p1 = B.train_steps(c["params"], c["X"], ones, c["dY"], 1)[0]
    assert (first["k_X1"] == first["k_Y0"]).all()              # a product with 1 is exact: the mask adds nothing to kappa
    vs = _views(fx, f"{name}.f64", "H", first["H"])
    for n in B.names():
        vs += _views(fx, f"{name}.f64.grad", n, first["grads"][n])
        vs += _views(fx, f"{name}.f64.param{STEPS}", n, p3[n])
        vs += _views(fx, f"{name}.f64.param1", n, p1[n])
    assert len(vs) >= 25, len(vs)
    assert {w.split(".")[-1] for w, _, _ in vs} >= {"steps", "rowsum", "colsum"}
    worst = 0.0
    for what, val, ref in vs:
        rel = float(np.abs(val - ref).max() / max(np.abs(ref).max(), 1e-300))
        worst = max(worst, rel)
        assert rel <= 1e-12, (what, rel)
    print(f"{name}: ones mask, largest relative distance to the reference's double run {worst:.2e} over {len(vs)} views")


# ---------------------------------------------------------------------------------------------------- a seeded mask, torch in double
def masked_case(N, seed, family):
    c = R.stack_case(N, seed, family)
    keep = (np.random.RandomState(seed + 1).uniform(size=(N, R.TS, R.NY)) < P_KEEP).astype(np.float32) / np.float32(P_KEEP)
    assert keep.dtype == np.float32 and 0.8 < float((keep > 0).mean()) < 0.97
    return dict(c, keep=keep)


def torch_double(c, steps):
    """two single-layer bidirectional nn.LSTM(bias=False) with the mask multiplied in between: H, both layers' gradients, the
    parameters after 1 and after `steps` torch.optim.Adam steps, in double"""
    if ("torch", id(c)) in _MEMO:
        return _MEMO[("torch", id(c))]
    f64 = torch.float64
    rnn = [torch.nn.LSTM(R.IN_DIM[l], R.NH, num_layers=1, bias=False, bidirectional=True, batch_first=True).to(f64).train() for l in (0, 1)]
    short = len(R.P)
    with torch.no_grad():
        for l in (0, 1):
            named = dict(rnn[l].named_parameters())
            for n in R.names(l):
                named[n[short:].replace(f"_l{l}", "_l0")].copy_(torch.from_numpy(c["params"][n]).to(f64))
    X, keep, dH = (torch.from_numpy(c[k]).to(f64) for k in ("X", "keep", "dY"))
    opt = torch.optim.Adam([p for r in rnn for p in r.parameters()], lr=1e-4, weight_decay=0)
    out = {}

    def read(attr):
        res = {}
        for l in (0, 1):
            named = dict(rnn[l].named_parameters())
            for n in R.names(l):
                t = named[n[short:].replace(f"_l{l}", "_l0")]
                res[n] = (t.grad if attr == "grad" else t).detach().numpy().copy()
        return res
    for step in range(steps):
        opt.zero_grad()
        Y0, _ = rnn[0](X)
        X1 = Y0 * keep
        X1.retain_grad()
        H, _ = rnn[1](X1)
        (H * dH).sum().backward()
        if step == 0:
            out.update(H=H.detach().numpy().copy(), X1=X1.detach().numpy().copy(), dX1=X1.grad.numpy().copy(), grads=read("grad"))
        opt.step()
        if step == 0:
            out["params1"] = read("data")
    out["params"] = read("data")
    _MEMO[("torch", id(c))] = out
    return out


MASKED = {"default": masked_case(2, 71, "default"), "carry": masked_case(2, 72, "carry")}


def _model(family, flaw=None, steps=STEPS):
    key = (family, flaw, steps)
    if key not in _MEMO:
        c = MASKED[family]
        _MEMO[key] = B.train_steps(c["params"], c["X"], c["keep"], c["dY"], steps, flaw=flaw)
    return _MEMO[key]


def _outputs(family, flaw=None):
    """[(what, model value, kappa)] of the masked step: H, X1, dX1, every gradient, every parameter after one and three steps"""
    p3, _, _, k3, _, _, first = _model(family, flaw)
    p1, _, _, k1, _, _, _ = _model(family, flaw, 1)
    out = [("H", first["H"], first["k_H"]), ("X1", first["X1"], first["k_X1"]), ("dX1", first["dX1"], first["k_dX1"])]
    for n in B.names():
        s = n[len(R.P):]
        out += [("grad " + s, first["grads"][n], first["k_grads"][n]), ("param1 " + s, p1[n], k1[n]), (f"param{STEPS} " + s, p3[n], k3[n])]
    return out


def _torch_outputs(family):
    t = torch_double(MASKED[family], STEPS)
    out = [t["H"], t["X1"], t["dX1"]]
    for n in B.names():
        out += [t["grads"][n], t["params1"][n], t["params"][n]]
    return out


@pytest.mark.parametrize("family", sorted(MASKED))
def test_seeded_mask_is_torch_in_double(family):
    worst = 0.0
    got, ref = _outputs(family), _torch_outputs(family)
    assert len(got) == len(ref) == 3 + 3 * 8
    for (what, val, _), r in zip(got, ref):
        rel = float(np.abs(val - r).max() / max(np.abs(r).max(), 1e-300))
        worst = max(worst, rel)
        assert rel <= 1e-12, (what, rel)
    # the mask does something: a tenth of X1 is zero, and the masked positions pass no gradient into layer 0
    first = _model(family)[6]
    keep = MASKED[family]["keep"]
    assert (first["X1"][keep == 0] == 0).all() and (first["dY0"][keep == 0] == 0).all() and (first["dX1"][keep == 0] != 0).any()
    print(f"{family}: seeded mask, largest relative distance to torch in double {worst:.2e} over {len(got)} outputs")


@pytest.mark.parametrize("flaw", B.FLAWS)
def test_controls_are_outside_kappa_of_torch_in_double(flaw):
    """kappa is not too loose: each wrong model lies at least 10 x kappa (of the right model) from torch's double run on at least
    one output.  kappa is used as it stands, never scaled.  Every output's figure is printed: where a control does not move an
    output at all (layer 0 left untrained leaves H of the first step and all of layer 1's first-step values as they are; the mask
    left out of the backward leaves the whole forward) the figure is the double run's own round-off, 1e-11 x kappa or less, and the
    control is judged on the outputs it does move."""
    family = "carry"
    ref = _torch_outputs(family)
    ratios = {}
    for (what, _, kap), (_, val, _), r in zip(_outputs(family), _outputs(family, flaw), ref):
        ratios[what] = float((np.abs(val - r) / np.maximum(kap, 1e-300)).max())
    worst = max(ratios.values())
    print(f"{flaw}: {worst:.3g} x kappa at most; " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert worst >= 10.0, (flaw, ratios)
    if flaw == "layer0_untrained":          # judged where it acts: layer 0's own gradients and parameters
        assert max(v for k, v in ratios.items() if "_l0" in k) >= 10.0 and ratios["H"] < 1e-6
    if flaw == "mask_not_in_backward":      # the forward is untouched; layer 0's gradients are where it shows
        assert max(ratios["H"], ratios["X1"], ratios["dX1"]) < 1e-6 and max(v for k, v in ratios.items() if k.startswith("grad") and "_l0" in k) >= 10.0


# ---------------------------------------------------------------------------------------------------- the ABI, without a device
def test_library_exports_what_the_header_declares():
    from sdfa_amd import _lib, bilstmtrain
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sdfa_bilstm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_[a-z0-9_]+)\s*\(", text))
    assert declared == {"sdfa_bilstm_abi_version", "sdfa_encoder_x0"} == set(bilstmtrain.SYMBOLS), declared ^ set(bilstmtrain.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    version = int(re.search(r"#define\s+SDFA_BILSTM_ABI_VERSION\s+(\d+)", text).group(1))
    assert _lib.lib.sdfa_bilstm_abi_version() == version == bilstmtrain.ABI_VERSION
    for macro, value in (("STEPS", bilstmtrain.STEPS), ("FEATURES", bilstmtrain.FEATURES)):
        assert int(re.search(rf"#define\s+SDFA_BILSTM_{macro}\s+(\d+)", text).group(1)) == value, macro
    assert (bilstmtrain.STEPS, bilstmtrain.FEATURES) == (R.TS, R.IN_DIM[0])
    # the versions the other headers carry are what they were
    from sdfa_amd import attntrain, headtrain, lstmtrain
    assert (_lib.ABI_VERSION, lstmtrain.ABI_VERSION, attntrain.ABI_VERSION, headtrain.ABI_VERSION) == (5, 1, 1, 1)


def test_encoder_x0_refuses_null_arguments_without_a_device():
    from sdfa_amd import _lib, bilstmtrain  # noqa: F401
    lib = _lib.lib
    assert lib.sdfa_encoder_x0(None, None, 2, None, None, 0, None) == _lib.EINVAL        # the null X0 first, as sdfa_encoder_layer0's X1
    assert b"encoder_x0" in lib.sdfa_last_error()
    import ctypes as C
    x0 = (C.c_float * 4)()
    assert lib.sdfa_encoder_x0(None, None, 2, C.addressof(x0), None, 0, None) == _lib.ESTATE      # then the model, as every encoder entry point
