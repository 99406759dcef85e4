"""tests/freqtrain_ref64.py -- the float64 model the GPU tests of the frequency LSTM's training step compare with -- pinned on the
CPU: against the reference's own FreqLstm (layer 6 of the audio encoder), autograd and torch.optim.Adam
(tests/golden/train_freq*.npz, written by tests/gen_golden_train_freq.py: double run to 1e-12 relative, float32 run within
1 x kappa), against its own wrong variants (each more than 10 x kappa from the fixture somewhere; the figures are printed),
against central differences, the forget gates of the "carry" family, and the ABI of include/sdfa_freqtrain.h with the refusals
that need no device (the handle's refusals call by call: tests/test_freqtrain_refusals_cpu.py)."""
import os
import re

import numpy as np
import pytest

import freqtrain_ref64 as R
from gen_golden_train_freq import CASES, C_STEPS, FILES, FULL, STEPS, inputs, row_stride

_MEMO = {}


def fixture(golden):
    if "g" not in _MEMO:
        fx = {}
        for f in FILES:
            g = golden[f]
            fx.update({k: g[k] for k in g.files})
        _MEMO["g"] = fx
    return _MEMO["g"]


def model(name, flaw=None, steps=STEPS):
    key = (name, flaw, steps)
    if key not in _MEMO:
        _MEMO[key] = R.train_steps(inputs(name), steps, flaw=flaw)
    return _MEMO[key]


def views(fx, prefix, name, val, kap):
    """[(what, model value, kappa, fixture value)] for every stored view of tensor `name` under `prefix`"""
    out = []
    val, kap = np.asarray(val, np.float64), np.asarray(kap, np.float64)
    k = f"{prefix}.{name}"
    if k in fx:
        out.append((name, val, kap, fx[k].astype(np.float64)))
    if k + ".steps" in fx:
        out.append((name + ".steps", val[:, list(C_STEPS)], kap[:, list(C_STEPS)], fx[k + ".steps"].astype(np.float64)))
    if k + ".rows" in fx:
        out.append((name + ".rows", val[::row_stride(name)], kap[::row_stride(name)], fx[k + ".rows"].astype(np.float64)))
    if k + ".rowsum" in fx:
        out.append((name + ".rowsum", val.sum(1), kap.sum(1), fx[k + ".rowsum"]))
    if k + ".colsum" in fx:
        out.append((name + ".colsum", val.sum(0), kap.sum(0), fx[k + ".colsum"]))
    return out


def all_views(fx, name, tag, flaw=None):
    p, m, v, ep, em, ev, first = model(name, flaw)
    out = []
    for what in ("X0", "dC"):
        out += views(fx, f"{name}.{tag}", what, first[what], first["k_" + what])
    for n in first["grads"]:
        out += views(fx, f"{name}.{tag}.grad", n, first["grads"][n], first["k_grads"][n])
        out += views(fx, f"{name}.{tag}.param{STEPS}", n, p[n], ep[n])
        out += views(fx, f"{name}.{tag}.param1", n, first["params1"][n], first["k_params1"][n])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref64_is_the_references_double_run(golden, name):
    fx = fixture(golden)
    vs = all_views(fx, name, "f64")
    assert len(vs) >= 30, len(vs)
    worst = 0.0
    for what, val, _, ref in vs:
        rel = float(np.abs(val - ref).max() / max(np.abs(ref).max(), 1e-300))
        worst = max(worst, rel)
        assert rel <= 1e-12, (what, rel)
    print(f"{name}: largest relative distance to the reference's double run {worst:.2e} over {len(vs)} views")


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_float32_run_within_kappa(golden, name):
    """kappa is not too small: the reference's float32 route -- other kernels, another order, other activation functions,
    autograd's own backward -- lies within 1 x kappa of the model.  The parameters after three steps are not compared: their
    kappa is carried through a second and third step and says nothing."""
    fx = fixture(golden)
    vs = [v for v in all_views(fx, name, "f32") if not v[0].endswith("sum")]
    assert len(vs) >= 10, len(vs)
    worst = {}
    for what, val, kap, ref in vs:
        d = np.abs(val - ref)
        ratio = float((d / np.maximum(kap, 1e-300)).max())
        worst[what] = max(worst.get(what, 0.0), ratio)
        assert (d <= kap).all(), (what, ratio)
    print(f"{name}: float32-run distances in kappa: " + ", ".join(f"{k.rsplit('.6.', 1)[-1]} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_outside_kappa_of_the_fixture(golden, flaw):
    """kappa is not too loose: each wrong model lies more than 10 x kappa (of the right model) from the reference's double run on
    at least one output."""
    fx = fixture(golden)
    right = all_views(fx, FULL, "f64")
    wrong = all_views(fx, FULL, "f64", flaw)
    worst, where = 0.0, None
    for (what, _, kap, ref), (_, val, _, _) in zip(right, wrong):
        if what.endswith("sum") or ".param" in what:
            continue
        r = float((np.abs(val - ref) / np.maximum(kap, 1e-300)).max())
        if r > worst:
            worst, where = r, what
    print(f"{flaw}: {worst:.3g} x kappa (on {where})")
    assert worst > 10.0, (flaw, worst)


def test_carry_family_keeps_its_cell_state():
    for name, (rows, seed, family) in CASES.items():
        mf = model(name)[6]["mean_f"]
        print(f"{name}: mean forget gate {mf:.3f}")
        assert mf >= 0.9 if family == "carry" else 0.4 < mf < 0.6, (name, mf)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_analytic_gradients_match_central_differences(family):
    c = R.case(3, 7, family)
    r = R.run(c["params"], c["C"], c["dX0"])
    rs = np.random.RandomState(3)
    worst = 0.0
    for n in list(c["params"]) + ["C"]:
        base = np.asarray(c["C"] if n == "C" else c["params"][n], np.float64)
        ana = r["dC"] if n == "C" else r["grads"][n]
        for i in range(2):
            idx = tuple(rs.randint(0, s) for s in base.shape)
            h = 1e-4 * max(abs(base[idx]), 1e-1)
            vals = []
            for sgn in (1, -1):
                pert = base.copy()
                pert[idx] += sgn * h
                vals.append(R.loss(c["params"] if n == "C" else dict(c["params"], **{n: pert}), pert if n == "C" else c["C"], c["dX0"]))
            num = (vals[0] - vals[1]) / (2 * h)
            scale = max(abs(ana[idx]), float(np.abs(ana).max()) * 1e-3)
            worst = max(worst, abs(num - ana[idx]) / scale)
            assert abs(num - ana[idx]) <= 1e-6 * scale, (n, idx, num, ana[idx])
    print(f"{family}: largest central-difference distance {worst:.2e} of the gradient's size")


# ---------------------------------------------------------------------------------------------------- the ABI, without a device
def test_library_exports_what_the_header_declares():
    from sdfa_amd import _lib, freqtrain
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sdfa_freqtrain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_freqtrain_\w+|sdfa_encoder_conv)\s*\(", text))
    assert "sdfa_encoder_conv" in declared and len(declared) == 17, sorted(declared)
    assert declared == set(freqtrain.SYMBOLS), declared ^ set(freqtrain.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    version = int(re.search(r"#define\s+SDFA_FREQTRAIN_ABI_VERSION\s+(\d+)", text).group(1))
    assert _lib.lib.sdfa_freqtrain_abi_version() == version == freqtrain.ABI_VERSION
    for macro, value in (("COLUMNS", freqtrain.COLUMNS), ("STEPS", freqtrain.STEPS), ("IN", freqtrain.IN), ("HIDDEN", freqtrain.HIDDEN),
                         ("GATES", freqtrain.GATES), ("OUT", freqtrain.OUT), ("TILE_COLUMNS", freqtrain.TILE_COLUMNS),
                         ("BLOCK_FRAMES", freqtrain.BLOCK_FRAMES), ("MAX_FRAMES", freqtrain.MAX_FRAMES)):
        assert int(re.search(rf"#define\s+SDFA_FREQTRAIN_{macro}\s+(\d+)", text).group(1)) == value, macro
    assert freqtrain.MAX_FRAMES >= 2048
    assert freqtrain.tensor_shapes() == R.shapes()
    assert list(freqtrain.tensor_shapes()) == list(R.names())
    assert (R.COLS, R.NS, R.NI, R.NH, R.NG, R.NO, R.NK) == (freqtrain.COLUMNS, freqtrain.STEPS, freqtrain.IN, freqtrain.HIDDEN, freqtrain.GATES,
                                                            freqtrain.OUT, freqtrain.FEATURES)


def test_abi_refusals_without_a_device():
    import ctypes as C
    from sdfa_amd import _lib, freqtrain
    lib = _lib.lib
    h = C.c_void_p(lib.sdfa_freqtrain_create())
    assert h
    try:
        assert lib.sdfa_freqtrain_numel(h) == sum(int(np.prod(s)) for s in R.shapes().values()) == 2296064
        a = np.zeros(512 * 128, np.float32)
        name = R.names()[3].encode()
        assert lib.sdfa_freqtrain_set_tensor(h, name, a.ctypes.data, a.size) == 0
        assert lib.sdfa_freqtrain_set_tensor(h, name, a.ctypes.data, a.size - 1) == _lib.EINVAL
        assert lib.sdfa_freqtrain_set_tensor(h, b"_audio_encoder._layers.9.weight_hh_l0", a.ctypes.data, a.size) == _lib.EINVAL
        assert b"the frequency LSTM has no tensor" in lib.sdfa_last_error()
        assert lib.sdfa_freqtrain_set_tensor(h, name, None, a.size) == _lib.EINVAL
        assert lib.sdfa_freqtrain_finalize(h, None) == _lib.ESTATE
        assert b"is missing" in lib.sdfa_last_error() and b"_lstm.weight_ih_l0\"" in lib.sdfa_last_error()
        assert lib.sdfa_freqtrain_workspace_bytes(h, 0) == _lib.EINVAL
        assert lib.sdfa_freqtrain_workspace_bytes(h, freqtrain.MAX_FRAMES + 1) == _lib.EINVAL
        w1, w100 = lib.sdfa_freqtrain_workspace_bytes(h, 1), lib.sdfa_freqtrain_workspace_bytes(h, 100)
        assert 14 * 1024 * 1024 < w1 < w100 and w1 % 256 == 0 and w100 % 256 == 0
        assert w100 - w1 >= 99 * 14 * 1024 * 1024
        assert lib.sdfa_freqtrain_workspace_bytes(h, freqtrain.MAX_FRAMES) > 2 ** 34
        # an unfinalised handle: every call of the step is refused before it looks at a pointer
        assert lib.sdfa_freqtrain_forward(h, None, 2, None, None, 0, None) == _lib.ESTATE
        assert lib.sdfa_freqtrain_backward(h, None, None, 2, None, None, 0, None) == _lib.ESTATE
        assert lib.sdfa_freqtrain_adam(h, 1e-4, 0.9, 0.999, 1e-8, None) == _lib.ESTATE
        assert lib.sdfa_freqtrain_zero_grad(h, None) == _lib.ESTATE
        assert lib.sdfa_freqtrain_get_tensor(h, name, 0, a.ctypes.data, a.size) == _lib.ESTATE
        assert lib.sdfa_freqtrain_step_count(h) == 0 and lib.sdfa_freqtrain_set_step_count(h, -1) == _lib.EINVAL
    finally:
        lib.sdfa_freqtrain_destroy(h)
    assert lib.sdfa_freqtrain_forward(None, None, 2, None, None, 0, None) == _lib.EINVAL
    assert lib.sdfa_freqtrain_backward(None, None, None, 2, None, None, 0, None) == _lib.EINVAL
    assert lib.sdfa_encoder_conv(None, None, 2, None, None, 0, None) == _lib.EINVAL        # the null C first, as sdfa_encoder_x0's X0
    assert b"encoder_conv: null pointer" in lib.sdfa_last_error()
