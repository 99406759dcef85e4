"""tests/convtrain_ref64.py pinned, without a device: it equals the double run of the reference's own conv stack (tests/golden/
train_conv*.npz, made by tests/gen_golden_train_conv.py from the reference's modules in eval()) to 1e-12 relative; the reference's
float32 run lies within 1 x kappa (kappa is not too small); the analytic gradients agree with central differences on a case with
no ambiguous element and no tie; every control of convtrain_ref64.FLAWS lies more than 10 x kappa from the double run somewhere
(kappa is not too loose); in every committed case and in every case the GPU tests use the ambiguous elements of either kind are
at most 1e-3 of each layer's elements.  And the ABI without a device: the header declares what SYMBOLS lists, the library
exports it, versions and constants agree, null arguments are refused."""
import functools
import os
import re

import numpy as np
import pytest

import convtrain_ref64 as R
from gen_golden_train_conv import CASES, C_ROWS, FILES, STEPS, inputs

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 1e-3


@pytest.fixture(scope="module")
def golden():
    out = {}
    for f in FILES:
        with np.load(os.path.join(HERE, "golden", f + ".npz")) as z:
            out.update({k: z[k] for k in z.files})
    return out


@functools.lru_cache(maxsize=None)
def double_model(name):
    return R.train_steps(inputs(name), STEPS, slope=0.2, eps=1e-3)


@functools.lru_cache(maxsize=None)
def device_model(name):
    return R.train_steps(inputs(name), 1)


def rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def short(n):
    return n[len(R.P):]


@pytest.mark.parametrize("name", list(CASES))
def test_ref64_is_the_references_double_run(golden, name):
    p, m, v, kp, km, kv, first = double_model(name)
    pre = f"{name}.f64"
    worst = rel(first["C"][:, list(C_ROWS)], golden[pre + ".C.rows"])
    p1 = R.train_steps(inputs(name), 1, slope=0.2, eps=1e-3)[0]
    for n in R.names():
        worst = max(worst, rel(first["grads"][n], golden[f"{pre}.grad.{short(n)}"]), rel(p1[n], golden[f"{pre}.param1.{short(n)}"]),
                    rel(p[n], golden[f"{pre}.param{STEPS}.{short(n)}"]))
    print(f"\n{name}: the model against the reference's double run, largest relative distance {worst:.2e}")
    assert worst <= 1e-12, worst


def ambiguity(first):
    return {L: (first["ambiguous_kink"][L], first["ambiguous_pool"][L], first["ties"][L], first["elements"][L]) for L in first["elements"]}


@pytest.mark.parametrize("name", list(CASES))
def test_references_float32_run_within_kappa(golden, name):
    p, m, v, kp, km, kv, first = device_model(name)
    pre = f"{name}.f32"
    worst = {}

    def ratio(what, got, val, kap):
        d = np.abs(got.astype(np.float64) - val)
        r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
        worst[what] = max(worst.get(what, 0.0), r)
        assert (d <= kap).all(), (what, r)

    ratio("C", golden[pre + ".C.rows"], first["C"][:, list(C_ROWS)], first["k_C"][:, list(C_ROWS)])
    for n in R.names():
        ratio("grad", golden[f"{pre}.grad.{short(n)}"], first["grads"][n], first["k_grads"][n])
        ratio("param1", golden[f"{pre}.param1.{short(n)}"], p[n], kp[n])
    print(f"\n{name}: the reference's float32 run, largest distance / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items())
          + f"; (ambiguous kink, pool route, decided ties, elements) {ambiguity(first)}")


GPU_CASES = [(family, N) for family in R.FAMILIES for N in (1, 2, 9)]       # tests/test_gpu_convtrain.py's


@pytest.mark.parametrize("which", list(CASES) + [f"gpu-{f}-N{n}" for f, n in GPU_CASES] + ["gpu-op-edge-N2"] + [f"gpu-op-checkpoint-{k}" for k in R.CHECKPOINT_CASES])
def test_ambiguous_elements_stay_under_the_cap(which):
    if which in CASES:
        first = device_model(which)[6]
    elif which.startswith("gpu-op-checkpoint-"):              # tests/test_gpu_conv_train_op.py's: the synthetic checkpoint's own tensors
        from sdfa_amd import synth
        first = R.run(*R.checkpoint_case(synth.make_state_dict("offsets", 1234), which.rsplit("-", 1)[1]))
    elif which == "gpu-op-edge-N2":
        c = R.case(R.COLS * 2, 77, "edge")
        first = R.run(c["params"], c["feat"], c["dC"])
    else:
        _, family, N = which.split("-")
        N = int(N[1:])
        c = R.case(R.COLS * N, 700 + N + (0 if family == "default" else 5000), family)
        first = R.run(c["params"], c["feat"], c["dC"])
    amb = ambiguity(first)
    print(f"\n{which}: (ambiguous kink, pool route, decided ties, elements) {amb}")
    for L, (kink, pool, _, n) in amb.items():
        assert kink <= CAP * n and pool <= CAP * n, (which, L, kink, pool, n)
    assert R.under_cap(first) and CAP == R.AMBIGUOUS_CAP
    if "edge" in which:
        assert amb[1][2] > 0 and amb[3][2] > 0               # the family does make exact ties


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_controls_are_outside_kappa_of_the_fixture(golden, flaw):
    worst = 0.0
    for name in CASES:
        p, m, v, kp, km, kv, first = device_model(name)
        pre = f"{name}.f64"
        c = inputs(name)
        if flaw == "no_bias_correction":
            wp = R.train_steps(c, 1, flaw=flaw, slope=0.2, eps=1e-3)[0]
            for n in R.names():
                worst = max(worst, float((np.abs(wp[n] - golden[f"{pre}.param1.{short(n)}"]) / np.maximum(kp[n], 1e-300)).max()))
            continue
        w = R.run(c["params"], c["feat"], c["dC"], flaw=flaw, slope=0.2, eps=1e-3)
        rows = list(C_ROWS)
        worst = max(worst, float((np.abs(w["C"][:, rows] - golden[pre + ".C.rows"]) / np.maximum(first["k_C"][:, rows], 1e-300)).max()))
        for n in R.names():
            worst = max(worst, float((np.abs(w["grads"][n] - golden[f"{pre}.grad.{short(n)}"]) / np.maximum(first["k_grads"][n], 1e-300)).max()))
    print(f"\n{flaw}: the reference's double run lies {worst:.3g} x kappa from this wrong model")
    assert worst > 10.0, (flaw, worst)


def test_analytic_gradients_match_central_differences():
    """a case with no ambiguous element and no tie: the loss is smooth in a neighbourhood far wider than the step"""
    for seed in range(900, 940):
        c = R.case(3, seed, "default")
        first = R.run(c["params"], c["feat"], c["dC"], slope=0.2, eps=1e-3)
        if not any(sum(first[k].values()) for k in ("ambiguous_kink", "ambiguous_pool", "ties")):
            break
    else:
        raise AssertionError("no seed without an ambiguous element")
    dC = c["dC"].astype(np.float64)
    loss = lambda p: float((R.run(p, c["feat"], slope=0.2, eps=1e-3)["C"] * dC).sum())
    rs = np.random.RandomState(1)
    worst = 0.0
    for n in R.names():
        ana = first["grads"][n]
        scale = np.abs(ana).max()
        for _ in range(3):
            idx = tuple(rs.randint(0, s) for s in ana.shape)
            h = 1e-6
            up, dn = ({k: np.array(v, np.float64) for k, v in c["params"].items()} for _ in range(2))
            up[n][idx] += h
            dn[n][idx] -= h
            num = (loss(up) - loss(dn)) / (2 * h)
            worst = max(worst, abs(num - ana[idx]) / scale)
            assert abs(num - ana[idx]) <= 1e-6 * scale, (n, idx, num, ana[idx])
    print(f"\nseed {seed}: largest central-difference distance {worst:.2e} of the gradient's size")


# ---------------------------------------------------------------------------------------------------- the ABI, without a device
def test_library_exports_what_the_header_declares():
    from sdfa_amd import _lib, convtrain
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "include", "sdfa_convtrain.h")).read()
    said = text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_convtrain_\w+)\s*\(", text))
    assert len(declared) == 16, sorted(declared)
    assert declared == set(convtrain.SYMBOLS), declared ^ set(convtrain.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    version = int(re.search(r"#define\s+SDFA_CONVTRAIN_ABI_VERSION\s+(\d+)", text).group(1))
    assert _lib.lib.sdfa_convtrain_abi_version() == version == convtrain.ABI_VERSION
    for macro, value in (("COLUMNS", convtrain.COLUMNS), ("BINS", convtrain.BINS), ("IN", convtrain.IN), ("OUT_BINS", convtrain.OUT_BINS),
                         ("OUT", convtrain.OUT), ("NUMEL", convtrain.NUMEL), ("BLOCK_FRAMES", convtrain.BLOCK_FRAMES),
                         ("MAX_FRAMES", convtrain.MAX_FRAMES)):
        assert int(re.search(rf"#define\s+SDFA_CONVTRAIN_{macro}\s+(\d+)", text).group(1)) == value, macro
    assert float(re.search(r"#define\s+SDFA_CONVTRAIN_BN_EPS\s+([0-9.e-]+)f", text).group(1)) == convtrain.BN_EPS == 1e-3
    from sdfa_amd import freqtrain
    assert convtrain.MAX_FRAMES == freqtrain.MAX_FRAMES == 2048
    assert convtrain.tensor_shapes() == {k: s for k, s in R.shapes().items() if "running" not in k}
    assert list(convtrain.tensor_shapes()) == list(R.names()) and list(convtrain.constant_shapes()) == list(R.constant_names())
    assert (R.COLS, R.BINS, R.IN, R.OUT_BINS, R.OUT) == (convtrain.COLUMNS, convtrain.BINS, convtrain.IN, convtrain.OUT_BINS, convtrain.OUT)
    assert tuple(L[:4] for L in R.LAYERS) == convtrain.LAYERS
    assert sum(convtrain.LAUNCHES.values()) == 11 and "4 (forward" in said and "+ 6 (backward" in said
    assert "train() mode" in said and "train() mode" in convtrain.__doc__          # the BatchNorm mode is said where it is read


def test_abi_refusals_without_a_device():
    import ctypes as C
    from sdfa_amd import _lib, convtrain
    lib = _lib.lib
    h = C.c_void_p(lib.sdfa_convtrain_create())
    assert h
    try:
        assert lib.sdfa_convtrain_numel(h) == sum(int(np.prod(R.shapes()[n])) for n in R.names()) == 11168
        a = np.zeros(64 * 32 * 3, np.float32)
        name = R.names()[6].encode()                          # layer 3's weight_v
        assert lib.sdfa_convtrain_set_tensor(h, name, a.ctypes.data, a.size) == 0
        assert lib.sdfa_convtrain_set_tensor(h, name, a.ctypes.data, a.size - 1) == _lib.EINVAL
        assert lib.sdfa_convtrain_set_tensor(h, b"_audio_encoder._layers.6._proj.bias", a.ctypes.data, 256) == _lib.EINVAL
        assert b"the conv stack has no tensor" in lib.sdfa_last_error()
        assert lib.sdfa_convtrain_set_tensor(h, R.constant_names()[3].encode(), a.ctypes.data, 64) == 0
        assert lib.sdfa_convtrain_set_tensor(h, name, None, a.size) == _lib.EINVAL
        assert lib.sdfa_convtrain_finalize(h, None) == _lib.ESTATE
        assert b"is missing" in lib.sdfa_last_error() and b"_layers.1.weight_g\"" in lib.sdfa_last_error()
        assert lib.sdfa_convtrain_workspace_bytes(h, 0) == _lib.EINVAL
        assert lib.sdfa_convtrain_workspace_bytes(h, convtrain.MAX_FRAMES + 1) == _lib.EINVAL
        w1, w100 = lib.sdfa_convtrain_workspace_bytes(h, 1), lib.sdfa_convtrain_workspace_bytes(h, 100)
        assert 6 * 1024 * 1024 < w1 < w100 and w1 % 256 == 0 and w100 % 256 == 0
        assert w100 - w1 >= 99 * 6 * 1024 * 1024
        # an unfinalised handle: every call of the step is refused before it looks at a pointer
        assert lib.sdfa_convtrain_forward(h, None, 2, None, None, 0, None) == _lib.ESTATE
        assert lib.sdfa_convtrain_backward(h, None, None, 2, None, 0, None) == _lib.ESTATE
        assert lib.sdfa_convtrain_adam(h, 1e-4, 0.9, 0.999, 1e-8, None) == _lib.ESTATE
        assert lib.sdfa_convtrain_zero_grad(h, None) == _lib.ESTATE
        assert lib.sdfa_convtrain_get_tensor(h, name, 0, a.ctypes.data, a.size) == _lib.ESTATE
        assert lib.sdfa_convtrain_step_count(h) == 0 and lib.sdfa_convtrain_set_step_count(h, -1) == _lib.EINVAL
    finally:
        lib.sdfa_convtrain_destroy(h)
    assert lib.sdfa_convtrain_forward(None, None, 2, None, None, 0, None) == _lib.EINVAL
    assert lib.sdfa_convtrain_numel(None) == _lib.EINVAL
