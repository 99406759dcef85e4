"""tests/headtrain_ref64.py -- the float64 model the GPU tests of the head's training step compare with -- pinned on the CPU:
against the reference's own output-module layers, autograd and torch.optim.Adam (tests/golden/train_head.npz, written by
tests/gen_golden_train_head.py: double run to 1e-12 relative, float32 run within 1 x kappa), against central differences,
against its own wrong variants (each more than 100 x kappa from the fixture somewhere), and the refusals of
include/sdfa_headtrain.h that need no device.

A speaker column that no row uses has an exactly zero gradient in the EFFECTIVE weight W (dW[:, 512 + s] = 0).  Under the
weight norm that is not a zero gradient of weight_v: dv[p, 512 + s] = -s_p (dg_p / ||v_p||) v[p, 512 + s], the projection term,
so the reference moves that column too.  What keeps its bits is an element whose gradient is exactly zero: checked on the
model here and on the device in tests/test_gpu_headtrain.py."""
import numpy as np
import pytest

import headtrain_ref64 as R
from gen_golden_train_head import CASES, ROW_STRIDE, STEPS, inputs

_MEMO = {}


def fixture(golden):
    if "g" not in _MEMO:
        g = golden["train_head"]
        _MEMO["g"] = {k: g[k] for k in g.files}
    return _MEMO["g"]


def model(name, slope, flaw=None):
    key = (name, slope, flaw)
    if key not in _MEMO:
        _MEMO[key] = R.train_steps(inputs(name), STEPS, flaw=flaw, slope=slope)
    return _MEMO[key]


def views(fx, prefix, name, val, kap):
    """[(what, model value, kappa, fixture value)] for every stored view of tensor `name` under `prefix`"""
    out = []
    val, kap = np.asarray(val, np.float64), np.asarray(kap, np.float64)
    k = f"{prefix}.{name}"
    if k in fx:
        out.append((name, val.reshape(fx[k].shape), kap.reshape(fx[k].shape), fx[k].astype(np.float64)))
    if k + ".rows" in fx:
        out.append((name + ".rows", val[::ROW_STRIDE], kap[::ROW_STRIDE], fx[k + ".rows"].astype(np.float64)))
    if k + ".rowsum" in fx:
        out.append((name + ".rowsum", val.sum(1), kap.sum(1), fx[k + ".rowsum"]))
    if k + ".colsum" in fx:
        out.append((name + ".colsum", val.sum(0), kap.sum(0), fx[k + ".colsum"]))
    return out


def all_views(fx, name, tag, slope, flaw=None):
    p, m, v, ep, em, ev, first = model(name, slope, flaw)
    out = views(fx, f"{name}.{tag}", "coef", first["coef"], first["k_coef"]) + views(fx, f"{name}.{tag}", "dz", first["dz"], first["k_dz"])
    for n in first["grads"]:
        out += views(fx, f"{name}.{tag}.grad", n, first["grads"][n], first["k_grads"][n])
        out += views(fx, f"{name}.{tag}.param{STEPS}", n, p[n], ep[n])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref64_is_the_references_double_run(golden, name):
    fx = fixture(golden)
    vs = all_views(fx, name, "f64", 0.2)
    assert len(vs) >= 14
    worst = 0.0
    for what, val, _, ref in vs:
        rel = float(np.abs(val - ref).max() / max(np.abs(ref).max(), 1e-300))
        worst = max(worst, rel)
        assert rel <= 1e-12, (what, rel)
    print(f"{name}: largest relative distance to the reference's double run {worst:.2e} over {len(vs)} views")


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_float32_run_within_kappa(golden, name):
    """kappa is not too small: the reference's float32 route -- other kernels, another order, its own weight-norm backward --
    lies within 1 x kappa of the model."""
    fx = fixture(golden)
    vs = [v for v in all_views(fx, name, "f32", R.SLOPE32) if not v[0].endswith("sum")]
    assert len(vs) >= 2
    worst = 0.0
    for what, val, kap, ref in vs:
        d = np.abs(val - ref)
        ratio = float((d / np.maximum(kap, 1e-300)).max())
        worst = max(worst, ratio)
        assert (d <= kap).all(), (what, ratio)
    print(f"{name}: largest float32-run distance {worst:.3f} x kappa over {len(vs)} views")


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_far_from_the_fixture(golden, flaw):
    """kappa is not too loose: each wrong model lies more than 100 x kappa (of the right model) from the reference's double
    run somewhere."""
    fx = fixture(golden)
    name = "dgrad_b3"
    right = all_views(fx, name, "f64", 0.2)
    wrong = all_views(fx, name, "f64", 0.2, flaw)
    worst = 0.0
    for (what, _, kap, ref), (_, val, _, _) in zip(right, wrong):
        if what.endswith("sum"):
            continue
        worst = max(worst, float((np.abs(val - ref) / np.maximum(kap, 1e-300)).max()))
    print(f"{flaw}: {worst:.3g} x kappa")
    assert worst > 100.0, (flaw, worst)


@pytest.mark.parametrize("head", ["dgrad", "offsets"])
def test_analytic_gradients_match_central_differences(head):
    c = R.case(head, 2, 7)
    r = R.run(head, c["params"], c["z"], c["sid"], c["dcoef"])
    d64 = np.asarray(c["dcoef"], np.float64)

    def loss(params, z):
        return float((R.run(head, params, z, c["sid"])["coef"] * d64).sum())

    rs = np.random.RandomState(3)
    worst = 0.0
    for n in list(c["params"]) + ["z"]:
        base = np.asarray(c["z"] if n == "z" else c["params"][n], np.float64)
        ana = r["dz"] if n == "z" else r["grads"][n].reshape(base.shape)
        for _ in range(3):
            idx = tuple(rs.randint(0, s) for s in base.shape)
            h = 1e-4 * max(abs(base[idx]), 1e-2)
            vals = []
            for sgn in (1, -1):
                pert = base.copy()
                pert[idx] += sgn * h
                params = dict(c["params"]) if n == "z" else dict(c["params"], **{n: pert})
                vals.append(loss(params, pert if n == "z" else c["z"]))
            num = (vals[0] - vals[1]) / (2 * h)
            scale = max(abs(ana[idx]), float(np.abs(ana).max()) * 1e-3)
            worst = max(worst, abs(num - ana[idx]) / scale)
            assert abs(num - ana[idx]) <= 1e-6 * scale, (n, idx, num, ana[idx])
    print(f"{head}: largest central-difference distance {worst:.2e} of the gradient's size")


def test_unused_speaker_column_and_zero_gradients():
    name = "dgrad_b3"
    c = inputs(name)
    absent = sorted(set(range(8)) - set(CASES[name][3]))
    assert absent == [5] and 5 not in c["sid"]
    r = R.run(c["head"], c["params"], c["z"], c["sid"], c["dcoef"])
    for n, dW in r["dW"].items():
        if dW.shape[1] == 520:
            assert (dW[:, 512 + 5] == 0.0).all(), n                 # the effective weight's column has a zero gradient ...
            assert (r["grads"][n + ".weight_v"][:, 512 + 5] != 0.0).any(), n        # ... weight_v's does not: the projection term
    # an element whose gradient is exactly zero at every step keeps its value, with kappa 0
    p = np.asarray(c["params"]["_output_module._layers.0.bias"], np.float64)
    g = np.zeros_like(p)
    g[::2] = 1e-3
    m = v = np.zeros_like(p)
    q = p
    for t in (1, 2, 3):
        q, m, v, kq, km, kv = R.adam(q, g, m, v, t)
    assert (q[1::2] == p[1::2]).all() and (kq[1::2] == 0).all() and (q[::2] != p[::2]).all() and (kq[::2] > 0).all()


# ---------------------------------------------------------------------------------------------------- the ABI, without a device
def test_abi_refusals_without_a_device():
    import ctypes as C
    from sdfa_amd import _lib, headtrain
    lib = _lib.lib
    assert lib.sdfa_headtrain_abi_version() == headtrain.ABI_VERSION
    assert not lib.sdfa_headtrain_create(7) and b"unknown head" in lib.sdfa_last_error()
    for head, code in (("dgrad", headtrain.HEAD_DGRAD), ("offsets", headtrain.HEAD_OFFSETS)):
        h = C.c_void_p(lib.sdfa_headtrain_create(code))
        assert h
        try:
            shapes = headtrain.tensor_shapes(head)
            assert lib.sdfa_headtrain_numel(h) == sum(int(np.prod(s)) for s in shapes.values())
            assert lib.sdfa_headtrain_coef_dim(h) == (265 if head == "dgrad" else 59)
            assert {n for n in shapes} == {L["name"] + s for L in R.layers_of(head) for s in (".weight_g", ".weight_v", ".bias")}
            a = np.zeros(512 * 520, np.float32)
            name = b"_output_module._layers.0.weight_v"
            assert lib.sdfa_headtrain_set_tensor(h, name, a.ctypes.data, a.size) == 0
            assert lib.sdfa_headtrain_set_tensor(h, name, a.ctypes.data, a.size - 1) == _lib.EINVAL
            assert lib.sdfa_headtrain_set_tensor(h, b"_output_module._layers.9.bias", a.ctypes.data, 512) == _lib.EINVAL
            assert lib.sdfa_headtrain_set_tensor(h, name, None, a.size) == _lib.EINVAL
            assert lib.sdfa_headtrain_finalize(h, None) == _lib.ESTATE and b"is missing" in lib.sdfa_last_error()
            assert lib.sdfa_headtrain_workspace_bytes(h, 1) == _lib.EINVAL
            w2, w100 = lib.sdfa_headtrain_workspace_bytes(h, 2), lib.sdfa_headtrain_workspace_bytes(h, 100)
            assert 0 < w2 < w100 and w2 % 256 == 0 and w100 % 256 == 0
            # an unfinalised handle: every call of the step is refused before it looks at a pointer
            assert lib.sdfa_headtrain_forward(h, None, None, 2, None, None, 0, None) == _lib.ESTATE
            assert lib.sdfa_headtrain_backward(h, None, 2, None, None, 0, None) == _lib.ESTATE
            assert lib.sdfa_headtrain_adam(h, 1e-4, 0.9, 0.999, 1e-8, None) == _lib.ESTATE
            assert lib.sdfa_headtrain_zero_grad(h, None) == _lib.ESTATE
            assert lib.sdfa_headtrain_get_tensor(h, name, 0, a.ctypes.data, a.size) == _lib.ESTATE
            assert lib.sdfa_headtrain_step_count(h) == 0 and lib.sdfa_headtrain_set_step_count(h, -1) == _lib.EINVAL
        finally:
            lib.sdfa_headtrain_destroy(h)
    assert lib.sdfa_headtrain_forward(None, None, None, 2, None, None, 0, None) == _lib.EINVAL


def test_refused_training_configurations():
    from speech_anime import hparams as H
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    for key, value, word in (("optim", dict(name="SGD", args=dict(lr=1e-3)), "optim.name"),
                             ("optim", dict(name="Adam", args=dict(lr=1e-4, weight_decay=0.01)), "weight_decay"),
                             ("optim", dict(name="Adam", args=dict(lr=1e-4), lr_scheduler=dict(name="x", args={})), "lr_scheduler"),
                             ("trainer", dict(max_grad_norm=1.0), "clipping"),
                             ("trainer", dict(grad_acc_steps=2), "grad_acc_steps")):
        hp = H.configure({"custom_hparams": "offsets"})
        hp.set_key(key, value)
        with pytest.raises(NotImplementedError, match=word):
            SaberSpeechDrivenAnimation(hp)._head_optimizer_args()
    hp = H.configure({"custom_hparams": "offsets"})
    hp.model.set_key("weight_norm", False)
    with pytest.raises(NotImplementedError, match="weight_norm"):
        SaberSpeechDrivenAnimation(hp)._head_optimizer_args()
    hp = H.configure({"custom_hparams": "offsets"})
    hp.model.set_key("output", dict(pca_trainable=True))
    with pytest.raises(NotImplementedError, match="pca_trainable"):
        SaberSpeechDrivenAnimation(hp)._head_optimizer_args()
    with pytest.raises(RuntimeError, match="enable_head_training"):
        SaberSpeechDrivenAnimation(H.configure({"custom_hparams": "offsets"})).train_step({}, 0)
