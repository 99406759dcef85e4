"""tests/attntrain_ref64.py -- the float64 model the GPU tests of the attention layer's training step compare with -- pinned on
the CPU: against the reference's own BahdanauAttention, autograd and torch.optim.Adam (tests/golden/train_attn.npz and
train_attn_dH.npz, written by tests/gen_golden_train_attn.py: double run to 1e-12 relative, float32 run within 1 x kappa),
against central differences, against its own wrong variants (each more than 1 x kappa from the fixture somewhere; the figures
are printed), the peakedness of the "peaked" family, and the ABI of include/sdfa_attntrain.h with the refusals that need no
device."""
import os
import re

import numpy as np
import pytest

import attntrain_ref64 as R
from gen_golden_train_attn import CASES, DH_STEPS, ROW_STRIDE, STEPS, inputs

_MEMO = {}


def fixture(golden):
    if "g" not in _MEMO:
        g, d = golden["train_attn"], golden["train_attn_dH"]
        _MEMO["g"] = {**{k: g[k] for k in g.files}, **{k: d[k] for k in d.files}}
    return _MEMO["g"]


def model(name, flaw=None):
    key = (name, flaw)
    if key not in _MEMO:
        _MEMO[key] = R.train_steps(inputs(name), STEPS, flaw=flaw)
    return _MEMO[key]


def model1(name, flaw=None):
    """one step: from the second step on kappa of a parameter is vacuous wherever the gradient's kappa reaches the gradient
    (Adam divides by sqrt(v)), so the optimiser's controls are judged after the first"""
    key = (name, flaw, 1)
    if key not in _MEMO:
        _MEMO[key] = R.train_steps(inputs(name), 1, flaw=flaw)
    return _MEMO[key]


def views(fx, prefix, name, val, kap):
    """[(what, model value, kappa, fixture value)] for every stored view of tensor `name` under `prefix`"""
    out = []
    val, kap = np.asarray(val, np.float64), np.asarray(kap, np.float64)
    k = f"{prefix}.{name}"
    if k in fx:
        out.append((name, val.reshape(fx[k].shape), kap.reshape(fx[k].shape), fx[k].astype(np.float64)))
    if k + ".steps" in fx:
        out.append((name + ".steps", val[:, list(DH_STEPS)], kap[:, list(DH_STEPS)], fx[k + ".steps"].astype(np.float64)))
    val2, kap2 = val.reshape(val.shape[0], -1), kap.reshape(kap.shape[0], -1)
    if k + ".rows" in fx:
        out.append((name + ".rows", val2[::ROW_STRIDE], kap2[::ROW_STRIDE], fx[k + ".rows"].astype(np.float64)))
    if k + ".rowsum" in fx:
        out.append((name + ".rowsum", val2.sum(1), kap2.sum(1), fx[k + ".rowsum"]))
    if k + ".colsum" in fx:
        out.append((name + ".colsum", val2.sum(0), kap2.sum(0), fx[k + ".colsum"]))
    return out


def all_views(fx, name, tag, flaw=None):
    p, m, v, ep, em, ev, first = model(name, flaw)
    out = []
    for what in ("z", "align", "dH"):
        out += views(fx, f"{name}.{tag}", what, first[what], first["k_" + what])
    for n in first["grads"]:
        out += views(fx, f"{name}.{tag}.grad", n, first["grads"][n], first["k_grads"][n])
        out += views(fx, f"{name}.{tag}.param{STEPS}", n, p[n], ep[n])
    p1, _, _, ep1, _, _, _ = model1(name, flaw)
    for n in p1:
        out += views(fx, f"{name}.{tag}.param1", n, p1[n], ep1[n])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref64_is_the_references_double_run(golden, name):
    fx = fixture(golden)
    vs = all_views(fx, name, "f64")
    assert len(vs) >= 16, len(vs)
    worst = 0.0
    for what, val, _, ref in vs:
        rel = float(np.abs(val - ref).max() / max(np.abs(ref).max(), 1e-300))
        worst = max(worst, rel)
        assert rel <= 1e-12, (what, rel)
    print(f"{name}: largest relative distance to the reference's double run {worst:.2e} over {len(vs)} views")


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_float32_run_within_kappa(golden, name):
    """kappa is not too small: the reference's float32 route -- other kernels, another order, autograd's own backward -- lies
    within 1 x kappa of the model."""
    fx = fixture(golden)
    vs = [v for v in all_views(fx, name, "f32") if not v[0].endswith("sum")]
    assert len(vs) >= 8, len(vs)
    worst = {}
    for what, val, kap, ref in vs:
        d = np.abs(val - ref)
        ratio = float((d / np.maximum(kap, 1e-300)).max())
        worst[what] = ratio
        assert (d <= kap).all(), (what, ratio)
    print(f"{name}: float32-run distances in kappa: " + ", ".join(f"{k.rsplit('.10.', 1)[-1]} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_outside_kappa_of_the_fixture(golden, flaw):
    """kappa is not too loose: each wrong model lies more than 1 x kappa (of the right model) from the reference's double run
    on at least one output."""
    fx = fixture(golden)
    name = "peaked_n2"
    right = all_views(fx, name, "f64")
    wrong = all_views(fx, name, "f64", flaw)
    worst = 0.0
    for (what, _, kap, ref), (_, val, _, _) in zip(right, wrong):
        if what.endswith("sum"):
            continue
        worst = max(worst, float((np.abs(val - ref) / np.maximum(kap, 1e-300)).max()))
    print(f"{flaw}: {worst:.3g} x kappa")
    assert worst > 1.0, (flaw, worst)


def test_peaked_family_is_peaked_and_flat_is_flat():
    for name, (N, seed, family) in CASES.items():
        a = model(name)[6]["align"]
        mx = a.max(1)
        print(f"{name}: largest align per frame {np.round(mx, 3)}")
        if family == "peaked":
            assert (mx > 0.5).mean() >= 0.5, (name, mx)
        else:
            assert (mx < 0.2).all(), (name, mx)
    mx = R.run(R.case(40, 140, "peaked")["params"], R.case(40, 140, "peaked")["H"])["align"].max(1)
    assert (mx > 0.5).mean() >= 0.5, mx


@pytest.mark.parametrize("family", R.FAMILIES)
def test_analytic_gradients_match_central_differences(family):
    c = R.case(2, 7, family)
    r = R.run(c["params"], c["H"], c["dz"])
    rs = np.random.RandomState(3)
    worst = 0.0
    for n in list(c["params"]) + ["H"]:
        base = np.asarray(c["H"] if n == "H" else c["params"][n], np.float64)
        ana = r["dH"] if n == "H" else r["grads"][n].reshape(base.shape)
        for i in range(4):
            idx = tuple(rs.randint(0, s) for s in base.shape)
            if n == "H" and i < 3:
                idx = (idx[0], R.W0 + i, idx[2])            # the three steps of the query window
            h = 1e-4 * max(abs(base[idx]), 1e-1)             # 1e-5 at least: the loss is O(1) and rounds at 1e-16
            vals = []
            for sgn in (1, -1):
                pert = base.copy()
                pert[idx] += sgn * h
                vals.append(R.loss(c["params"] if n == "H" else dict(c["params"], **{n: pert}), pert if n == "H" else c["H"], c["dz"]))
            num = (vals[0] - vals[1]) / (2 * h)
            scale = max(abs(ana[idx]), float(np.abs(ana).max()) * 1e-3)
            worst = max(worst, abs(num - ana[idx]) / scale)
            assert abs(num - ana[idx]) <= 1e-6 * scale, (n, idx, num, ana[idx])
    print(f"{family}: largest central-difference distance {worst:.2e} of the gradient's size")


# ---------------------------------------------------------------------------------------------------- the ABI, without a device
def test_library_exports_what_the_header_declares():
    from sdfa_amd import _lib, attntrain
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sdfa_attntrain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_attntrain_\w+|sdfa_encoder_memory)\s*\(", text))
    assert "sdfa_encoder_memory" in declared and len(declared) == 17, sorted(declared)
    assert declared == set(attntrain.SYMBOLS), declared ^ set(attntrain.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    version = int(re.search(r"#define\s+SDFA_ATTNTRAIN_ABI_VERSION\s+(\d+)", text).group(1))
    assert _lib.lib.sdfa_attntrain_abi_version() == version == attntrain.ABI_VERSION
    for macro, value in (("STEPS", attntrain.STEPS), ("DIM", attntrain.DIM), ("ATT", attntrain.ATT),
                         ("BLOCK_FRAMES", attntrain.BLOCK_FRAMES), ("MAX_FRAMES", attntrain.MAX_FRAMES)):
        assert int(re.search(rf"#define\s+SDFA_ATTNTRAIN_{macro}\s+(\d+)", text).group(1)) == value, macro
    assert attntrain.tensor_shapes() == R.SHAPES


def test_abi_refusals_without_a_device():
    import ctypes as C
    from sdfa_amd import _lib, attntrain
    lib = _lib.lib
    h = C.c_void_p(lib.sdfa_attntrain_create())
    assert h
    try:
        assert lib.sdfa_attntrain_numel(h) == sum(int(np.prod(s)) for s in R.SHAPES.values()) == 917760
        a = np.zeros(128 * 512, np.float32)
        name = R.WK.encode()
        assert lib.sdfa_attntrain_set_tensor(h, name, a.ctypes.data, a.size) == 0
        assert lib.sdfa_attntrain_set_tensor(h, name, a.ctypes.data, a.size - 1) == _lib.EINVAL
        assert lib.sdfa_attntrain_set_tensor(h, b"_audio_encoder._layers.10.proj_val.weight", a.ctypes.data, a.size) == _lib.EINVAL
        assert lib.sdfa_attntrain_set_tensor(h, name, None, a.size) == _lib.EINVAL
        assert lib.sdfa_attntrain_finalize(h, None) == _lib.ESTATE
        assert b"is missing" in lib.sdfa_last_error() and b"_conv_query.weight" in lib.sdfa_last_error()
        assert lib.sdfa_attntrain_workspace_bytes(h, 0) == _lib.EINVAL
        assert lib.sdfa_attntrain_workspace_bytes(h, attntrain.MAX_FRAMES + 1) == _lib.EINVAL
        w1, w100 = lib.sdfa_attntrain_workspace_bytes(h, 1), lib.sdfa_attntrain_workspace_bytes(h, 100)
        assert 0 < w1 < w100 and w1 % 256 == 0 and w100 % 256 == 0
        assert lib.sdfa_attntrain_workspace_bytes(h, attntrain.MAX_FRAMES) > 0
        # an unfinalised handle: every call of the step is refused before it looks at a pointer
        assert lib.sdfa_attntrain_forward(h, None, 2, None, None, None, 0, None) == _lib.ESTATE
        assert lib.sdfa_attntrain_backward(h, None, None, 2, None, None, 0, None) == _lib.ESTATE
        assert lib.sdfa_attntrain_adam(h, 1e-4, 0.9, 0.999, 1e-8, None) == _lib.ESTATE
        assert lib.sdfa_attntrain_zero_grad(h, None) == _lib.ESTATE
        assert lib.sdfa_attntrain_get_tensor(h, name, 0, a.ctypes.data, a.size) == _lib.ESTATE
        assert lib.sdfa_attntrain_step_count(h) == 0 and lib.sdfa_attntrain_set_step_count(h, -1) == _lib.EINVAL
    finally:
        lib.sdfa_attntrain_destroy(h)
    assert lib.sdfa_attntrain_forward(None, None, 2, None, None, None, 0, None) == _lib.EINVAL
