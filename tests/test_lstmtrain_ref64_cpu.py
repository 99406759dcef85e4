"""tests/lstmtrain_ref64.py -- the float64 model the GPU tests of the BiLSTM layer's training step compare with -- pinned on the
CPU: its two-layer composition against the reference's own torch.nn.LSTM (layer 9 of the audio encoder), autograd and
torch.optim.Adam (tests/golden/train_lstm*.npz, written by tests/gen_golden_train_lstm.py: double run to 1e-12 relative, float32
run within 1 x kappa), against its own wrong variants (each at least 10 x kappa from the fixture somewhere; the figures are
printed), against central differences, the forget gates of the "carry" family, and the ABI of include/sdfa_lstmtrain.h with the
refusals that need no device."""
import os
import re

import numpy as np
import pytest

import lstmtrain_ref64 as R
from gen_golden_train_lstm import CASES, FILES, FULL, H_STEPS, ROW_STRIDE, STEPS, inputs

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
        out.append((name + ".steps", val[:, list(H_STEPS)], kap[:, list(H_STEPS)], fx[k + ".steps"].astype(np.float64)))
    if k + ".rows" in fx:
        out.append((name + ".rows", val[::ROW_STRIDE], kap[::ROW_STRIDE], fx[k + ".rows"].astype(np.float64)))
    if k + ".rowsum" in fx:
        out.append((name + ".rowsum", val.sum(1), kap.sum(1), fx[k + ".rowsum"]))
    if k + ".colsum" in fx:
        out.append((name + ".colsum", val.sum(0), kap.sum(0), fx[k + ".colsum"]))
    return out


def all_views(fx, name, tag, flaw=None):
    p, m, v, ep, em, ev, first = model(name, flaw)
    out = []
    for what in ("H", "dX0"):
        out += views(fx, f"{name}.{tag}", what, first[what], first["k_" + what])
    for n in first["grads"]:
        out += views(fx, f"{name}.{tag}.grad", n, first["grads"][n], first["k_grads"][n])
        out += views(fx, f"{name}.{tag}.param{STEPS}", n, p[n], ep[n])
    p1, _, _, ep1, _, _, _ = model(name, flaw, 1)
    for n in p1:
        out += views(fx, f"{name}.{tag}.param1", n, p1[n], ep1[n])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_composed_ref64_is_the_references_double_run(golden, name):
    fx = fixture(golden)
    vs = all_views(fx, name, "f64")
    assert len(vs) >= 26, len(vs)
    worst = 0.0
    for what, val, _, ref in vs:
        rel = float(np.abs(val - ref).max() / max(np.abs(ref).max(), 1e-300))
        worst = max(worst, rel)
        assert rel <= 1e-12, (what, rel)
    print(f"{name}: largest relative distance to the reference's double run {worst:.2e} over {len(vs)} views")


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_float32_run_within_kappa(golden, name):
    """kappa is not too small: the reference's float32 route -- other kernels, another order, other activation functions,
    autograd's own backward -- lies within 1 x kappa of the model."""
    fx = fixture(golden)
    vs = [v for v in all_views(fx, name, "f32") if not v[0].endswith("sum")]
    assert len(vs) >= (2 if name == FULL else 10), len(vs)
    worst = {}
    for what, val, kap, ref in vs:
        d = np.abs(val - ref)
        ratio = float((d / np.maximum(kap, 1e-300)).max())
        worst[what] = ratio
        assert (d <= kap).all(), (what, ratio)
    print(f"{name}: float32-run distances in kappa: " + ", ".join(f"{k.rsplit('.9.', 1)[-1]} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_outside_kappa_of_the_fixture(golden, flaw):
    """kappa is not too loose: each wrong model lies at least 10 x kappa (of the right model) from the reference's double run
    on at least one output."""
    fx = fixture(golden)
    right = all_views(fx, FULL, "f64")
    wrong = all_views(fx, FULL, "f64", flaw)
    worst = 0.0
    for (what, _, kap, ref), (_, val, _, _) in zip(right, wrong):
        if what.endswith("sum"):
            continue
        worst = max(worst, float((np.abs(val - ref) / np.maximum(kap, 1e-300)).max()))
    print(f"{flaw}: {worst:.3g} x kappa")
    assert worst >= 10.0, (flaw, worst)


def test_carry_family_keeps_its_cell_state():
    for name, (N, seed, family) in CASES.items():
        first = model(name)[6]
        mf = [first["r0"]["mean_f"], first["r1"]["mean_f"]]
        print(f"{name}: mean forget gate of layer 0, layer 1: {mf[0]:.3f}, {mf[1]:.3f}")
        # in the stack only layer 0 sees the constant feature; layer 1 has it in its own one-layer cases, below
        assert mf[0] >= 0.9 if family == "carry" else all(0.4 < f < 0.6 for f in mf), (name, mf)
    for layer in (0, 1):
        c = R.case(layer, 2, 5, "carry")
        assert R.run(layer, c["params"], c["X"])["mean_f"] >= 0.9


def test_long_range_bptt_matters_in_the_carry_family():
    """the gradient that reaches a direction's first step from dY at steps 32 and later alone: a sizeable share in "carry\""""
    share = {}
    for family in R.FAMILIES:
        c = R.case(1, 2, 9, family)
        dY = c["dY"].copy()
        dY[:, :32, :R.NH] = 0                                  # the forward direction hears only of the second half
        dY[:, :, R.NH:] = 0
        far = np.abs(R.run(1, c["params"], c["X"], dY)["dX"][:, 0]).mean()
        share[family] = float(far / np.abs(R.run(1, c["params"], c["X"], c["dY"])["dX"][:, 0]).mean())
    print(f"share of |dX| at step 0 that comes from 32 steps or more away: {share}")
    assert share["carry"] > 0.05 and share["carry"] > 20 * share["default"], share


@pytest.mark.parametrize("family", R.FAMILIES)
def test_analytic_gradients_match_central_differences(family):
    c = R.stack_case(1, 7, family)
    r = R.stack(c["params"], c["X"], c["dY"])
    rs = np.random.RandomState(3)
    worst = 0.0
    for n in list(c["params"]) + ["X"]:
        base = np.asarray(c["X"] if n == "X" else c["params"][n], np.float64)
        ana = r["dX0"] if n == "X" else r["grads"][n]
        for i in range(2):
            idx = tuple(rs.randint(0, s) for s in base.shape)
            h = 1e-4 * max(abs(base[idx]), 1e-1)
            vals = []
            for sgn in (1, -1):
                pert = base.copy()
                pert[idx] += sgn * h
                vals.append(R.stack_loss(c["params"] if n == "X" else dict(c["params"], **{n: pert}), pert if n == "X" else c["X"], c["dY"]))
            num = (vals[0] - vals[1]) / (2 * h)
            scale = max(abs(ana[idx]), float(np.abs(ana).max()) * 1e-3)
            worst = max(worst, abs(num - ana[idx]) / scale)
            assert abs(num - ana[idx]) <= 1e-6 * scale, (n, idx, num, ana[idx])
    print(f"{family}: largest central-difference distance {worst:.2e} of the gradient's size")


# ---------------------------------------------------------------------------------------------------- the ABI, without a device
def test_library_exports_what_the_header_declares():
    from sdfa_amd import _lib, lstmtrain
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sdfa_lstmtrain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_lstmtrain_\w+|sdfa_encoder_layer0)\s*\(", text))
    assert "sdfa_encoder_layer0" in declared and len(declared) == 17, sorted(declared)
    assert declared == set(lstmtrain.SYMBOLS), declared ^ set(lstmtrain.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    version = int(re.search(r"#define\s+SDFA_LSTMTRAIN_ABI_VERSION\s+(\d+)", text).group(1))
    assert _lib.lib.sdfa_lstmtrain_abi_version() == version == lstmtrain.ABI_VERSION
    for macro, value in (("STEPS", lstmtrain.STEPS), ("HIDDEN", lstmtrain.HIDDEN), ("GATES", lstmtrain.GATES),
                         ("TILE_FRAMES", lstmtrain.TILE_FRAMES), ("BLOCK_FRAMES", lstmtrain.BLOCK_FRAMES), ("MAX_FRAMES", lstmtrain.MAX_FRAMES)):
        assert int(re.search(rf"#define\s+SDFA_LSTMTRAIN_{macro}\s+(\d+)", text).group(1)) == value, macro
    for layer in (0, 1):
        assert lstmtrain.tensor_shapes(layer) == R.shapes(layer)
        assert list(lstmtrain.tensor_shapes(layer)) == list(R.names(layer))


def test_abi_refusals_without_a_device():
    import ctypes as C
    from sdfa_amd import _lib, lstmtrain
    lib = _lib.lib
    for bad in (0, 128, 257, 1024, -256):
        assert not lib.sdfa_lstmtrain_create(bad)
        assert b"input width" in lib.sdfa_last_error()
    for layer, numel in ((0, 1048576), (1, 1572864)):
        h = C.c_void_p(lib.sdfa_lstmtrain_create(R.IN_DIM[layer]))
        assert h
        try:
            assert lib.sdfa_lstmtrain_numel(h) == sum(int(np.prod(s)) for s in R.shapes(layer).values()) == numel
            a = np.zeros(1024 * 256, np.float32)
            name = R.names(layer)[3].encode()
            assert lib.sdfa_lstmtrain_set_tensor(h, name, a.ctypes.data, a.size) == 0
            assert lib.sdfa_lstmtrain_set_tensor(h, name, a.ctypes.data, a.size - 1) == _lib.EINVAL
            assert lib.sdfa_lstmtrain_set_tensor(h, R.names(1 - layer)[3].encode(), a.ctypes.data, a.size) == _lib.EINVAL      # the other layer's
            assert lib.sdfa_lstmtrain_set_tensor(h, (R.P + f"bias_hh_l{layer}").encode(), a.ctypes.data, a.size) == _lib.EINVAL
            assert lib.sdfa_lstmtrain_set_tensor(h, name, None, a.size) == _lib.EINVAL
            assert lib.sdfa_lstmtrain_finalize(h, None) == _lib.ESTATE
            assert b"is missing" in lib.sdfa_last_error() and f"weight_ih_l{layer}\"".encode() in lib.sdfa_last_error()
            assert lib.sdfa_lstmtrain_workspace_bytes(h, 0) == _lib.EINVAL
            assert lib.sdfa_lstmtrain_workspace_bytes(h, lstmtrain.MAX_FRAMES + 1) == _lib.EINVAL
            w1, w100 = lib.sdfa_lstmtrain_workspace_bytes(h, 1), lib.sdfa_lstmtrain_workspace_bytes(h, 100)
            assert 640 * 1024 < w1 < w100 and w1 % 256 == 0 and w100 % 256 == 0
            assert lib.sdfa_lstmtrain_workspace_bytes(h, lstmtrain.MAX_FRAMES) > 0
            # an unfinalised handle: every call of the step is refused before it looks at a pointer
            assert lib.sdfa_lstmtrain_forward(h, None, 2, None, None, 0, None) == _lib.ESTATE
            assert lib.sdfa_lstmtrain_backward(h, None, None, None, 2, None, None, 0, None) == _lib.ESTATE
            assert lib.sdfa_lstmtrain_adam(h, 1e-4, 0.9, 0.999, 1e-8, None) == _lib.ESTATE
            assert lib.sdfa_lstmtrain_zero_grad(h, None) == _lib.ESTATE
            assert lib.sdfa_lstmtrain_get_tensor(h, name, 0, a.ctypes.data, a.size) == _lib.ESTATE
            assert lib.sdfa_lstmtrain_step_count(h) == 0 and lib.sdfa_lstmtrain_set_step_count(h, -1) == _lib.EINVAL
        finally:
            lib.sdfa_lstmtrain_destroy(h)
    assert lib.sdfa_lstmtrain_forward(None, None, 2, None, None, 0, None) == _lib.EINVAL
    assert lib.sdfa_encoder_layer0(None, None, 2, None, None, 0, None) == _lib.EINVAL        # the null X1 first, as sdfa_encoder_memory's H
