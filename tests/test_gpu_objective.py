"""objective_kernel and its finishing kernels (csrc/objective.hip, include/sdfa_objective.h) against the float64 restatement of
tests/objective_ref64.py: every loss, every record and every gradient element within 1 x kappa, the propagated error scale of
the float32 operations the device forms them with (derived there, nothing fitted).

Shapes, the smallest at which each part can go wrong.  The kernel's column block is 128 BASIS columns, not a whole number of
triangles: the scale basis (6 columns per triangle) crosses a block edge between T = 21 and 22 and fills three blocks exactly at
T = 64; the rotat basis (3 per triangle) crosses between T = 42 and 43 and fills three exactly at T = 128; T = 65 / 129 are one
triangle past; 9,976 is FLAME's.  B: 1, and 15 / 16 / 17 around the row tile's 16 pairs, 50 the shipped batch.  K: 1 / 1, 4 / 5,
8 / 9 (the expansion's zero-padded k step of 8 and one more), 32 / 33 (the contraction's coefficient tile), 85 / 180, the cap /
the cap.  PLAIN: W = 1, 129 (one column over a block), 15,069 x 59 (rows not 16-byte aligned), and 65,665 = 513 blocks + 1
column, where the 512 column partitions stop being single blocks.  Weights: unit, and uniform on 0.2 .. 2.

Exact assertions: prediction = truth gives zero losses, records and gradients; outputs prefilled with NaN are fully
overwritten; a repeated call is bitwise equal; the refusals hold with real buffers and launch nothing.  Control: the model of
the batch whose truth rows k and B + k are swapped must NOT fit the device's motion gradients.

Measured on an MI355X (pytest -s prints every figure): the largest |gpu - ref64| / kappa is 0.22 on a record and 0.19 on a gradient
element (T = 1, K = 1 / 1), 0.10 on a loss; from T = 21 on every ratio is below 0.07, and at full width below 0.001 (kappa's
worst-case term for the order of the contraction's additions grows with the number of columns).  The control misses by 1.3e5 x
kappa.  The module takes 4 s."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import objective_ref64 as R
from test_objective_ref64_cpu import POINTERS, call_refused, refusals

pytestmark = pytest.mark.gpu

CASES = {           # name -> (layout, T | W, Ks, Kr, B, seed, weights)
    "T1_K1_B1": ("dgrad", 1, 1, 1, 1, 1, "unit"),
    "T21_K4_5_B15": ("dgrad", 21, 4, 5, 15, 2, "uniform"),
    "T22_K8_9_B16": ("dgrad", 22, 8, 9, 16, 3, "uniform"),
    "T42_K32_33_B17": ("dgrad", 42, 32, 33, 17, 4, "unit"),
    "T43_K85_180_B3": ("dgrad", 43, 85, 180, 3, 5, "uniform"),
    "T64_cap_B2": ("dgrad", 64, 192, 192, 2, 6, "uniform"),
    "T65_K4_5_B50": ("dgrad", 65, 4, 5, 50, 7, "uniform"),
    "T128_K8_9_B1": ("dgrad", 128, 8, 9, 1, 8, "unit"),
    "T129_K85_180_B17": ("dgrad", 129, 85, 180, 17, 9, "uniform"),
    "T9976_K85_180_B50": ("dgrad", 9976, 85, 180, 50, 10, "uniform"),
    "plain_W1_K1_B1": ("plain", 1, 1, 0, 1, 11, "uniform"),
    "plain_W129_K3_B16": ("plain", 129, 3, 0, 16, 12, "unit"),
    "plain_W300_cap_B17": ("plain", 300, 192, 0, 17, 13, "uniform"),
    "plain_W15069_K59_B50": ("plain", 15069, 59, 0, 50, 14, "uniform"),
    "plain_W65665_K3_B1": ("plain", 65665, 3, 0, 1, 15, "uniform"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = R.case(*CASES[name])
    c["model"] = R.model(c["coef"], c["bases"], c["truth"], c["weight"], c["layout"])
    return c


def bases_on_device(c):
    from sdfa_amd import objective as O
    b = {k: torch.from_numpy(v).cuda() for k, v in c["bases"].items()}
    if c["layout"] == "dgrad":
        return O.Bases(O.LAYOUT_DGRAD, b["compT_s"], b["means_s"], b["compT_r"], b["means_r"])
    return O.Bases(O.LAYOUT_PLAIN, b["compT_s"], b["means_s"])


def run_raw(coef, truth, weight, bases):
    """sdfa_objective on outputs prefilled with NaN (and a workspace prefilled with NaN bytes)."""
    from sdfa_amd import objective as O
    from sdfa_amd._lib import lib, check
    N = coef.shape[0]
    need = O.workspace_bytes(N, bases.W, bases.Ks, bases.Kr, bases.layout)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    loss = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    rec = torch.full((N, 4), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((2, N, bases.Kc), float("nan"), dtype=torch.float32, device="cuda")
    dg = bases.layout == O.LAYOUT_DGRAD
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    check(lib.sdfa_objective(p(coef), N, bases.W, bases.Ks, bases.Kr, bases.layout, p(bases.compT_s), p(bases.means_s),
                             p(bases.compT_r) if dg else None, p(bases.means_r) if dg else None, p(truth), p(weight), p(loss), p(rec), p(grad),
                             p(ws), need, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return loss, rec, grad


def device_inputs(c):
    return tuple(torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("coef", "truth", "weight"))


def ratios(got, want, kappa):
    """Largest |got - want| / kappa; where kappa is 0 the value must be exact."""
    got, want, kappa = np.asarray(got, np.float64), np.asarray(want), np.asarray(kappa)
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    zero = kappa == 0
    assert (err[zero] == 0).all(), "an element with no error allowance is not exact"
    return float((err[~zero] / kappa[~zero]).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_losses_records_and_gradients_within_kappa(name):
    """Measured on an MI355X (pytest -s prints every figure): see DESIGN.md section 15 for the largest ratio per output."""
    c = case(name)
    m = c["model"]
    bases = bases_on_device(c)
    loss, rec, grad = run_raw(*device_inputs(c), bases)
    for t in (loss, rec, grad):
        assert not bool(torch.isnan(t).any()), "an output element was not written"
    r_loss = ratios(loss.cpu().numpy(), m["loss"], m["k_loss"])
    r_rec = ratios(rec.cpu().numpy(), m["rec"], m["k_rec"])
    r_grad = ratios(grad.cpu().numpy(), m["grad"], m["k_grad"])
    print(f"{name}: max |gpu - ref64| / kappa: loss {r_loss:.4f} rec {r_rec:.4f} grad {r_grad:.4f}")
    assert r_loss <= 1 and r_rec <= 1 and r_grad <= 1, (name, r_loss, r_rec, r_grad)
    B = c["coef"].shape[0] // 2
    assert not rec[:B, 1].any() and not rec[:B, 3].any()
    if c["layout"] == "plain":
        assert not rec[:, 2:].any() and loss[2] == 0 and loss[3] == 0
    assert (np.abs(m["grad"]).max(axis=(1, 2)) > 0).all()


@pytest.mark.parametrize("name", ["T22_K8_9_B16", "T129_K85_180_B17", "plain_W15069_K59_B50"])
def test_repeated_call_is_bitwise_equal_and_the_binding_agrees(name):
    from sdfa_amd import objective as O
    c = case(name)
    bases = bases_on_device(c)
    d = device_inputs(c)
    first = run_raw(*d, bases)
    again = run_raw(*d, bases)
    api = O.objective(*d, bases)
    torch.cuda.synchronize()
    for a, b, e in zip(first, again, api):
        assert torch.equal(a, b) and torch.equal(a, e)
    assert api[0].dtype == torch.float32 and api[1].dtype == torch.float64 and tuple(api[2].shape) == (2, d[0].shape[0], bases.Kc)


@pytest.mark.parametrize("name", ["T43_K85_180_B3", "T65_K4_5_B50", "plain_W129_K3_B16"])
@pytest.mark.parametrize("kind", ["zero", "one_hot"])
def test_prediction_equal_to_truth_gives_exact_zeros(name, kind):
    """coef = 0 predicts the means exactly; a single coefficient 1 per row predicts fl(compT[:, j] + means), one rounding in any
    order of the K additions (the others add exact zeros)."""
    c = case(name)
    bases = bases_on_device(c)
    N, W = c["truth"].shape
    coef = np.zeros_like(c["coef"])
    truth = np.zeros((N, W), np.float32)
    rs = np.random.RandomState(5)
    for compT, means, sl, cols, _ in R.parts_of(c["bases"], c["layout"], W):
        if kind == "zero":
            truth[:, cols] = means
        else:
            j = rs.randint(0, compT.shape[1], N)
            coef[np.arange(N), sl.start + j] = 1.0
            truth[:, cols] = (compT[:, j].T + means[None, :]).astype(np.float32)
    loss, rec, grad = run_raw(torch.from_numpy(coef).cuda(), torch.from_numpy(truth).cuda(), torch.from_numpy(c["weight"]).cuda(), bases)
    assert not loss.any() and not rec.any() and not grad.any()


def test_control_swapped_truth_pairs_do_not_fit():
    """Swapping rows k and B + k of the truth alone changes the sign of the truth's motion: the model of the swapped batch must
    not fit the device's motion gradients in the swapped rows, nor its motion records.  (It still fits the unswapped rows.)"""
    name = "T22_K8_9_B16"
    c = case(name)
    bases = bases_on_device(c)
    _, rec, grad = run_raw(*device_inputs(c), bases)
    B = c["coef"].shape[0] // 2
    swapped = c["truth"].copy()
    rows = np.asarray([0, 5, B - 1])
    swapped[rows], swapped[B + rows] = c["truth"][B + rows], c["truth"][rows]
    m = R.model(c["coef"], c["bases"], swapped, c["weight"], c["layout"])
    g, r = grad.cpu().numpy(), rec.cpu().numpy()
    hit = np.concatenate((rows, B + rows))
    bad = np.abs(g[1][hit] - m["grad"][1][hit]) / m["k_grad"][1][hit]
    print("control: swapped rows, |gpu - model of the swapped batch| / kappa, smallest over the rows' largest:", bad.max(axis=1).min())
    assert (bad.max(axis=1) > 1).all(), bad.max(axis=1)
    assert (np.abs(r[B + rows][:, [1, 3]] - m["rec"][B + rows][:, [1, 3]]) > m["k_rec"][B + rows][:, [1, 3]]).all()
    keep = np.setdiff1d(np.arange(2 * B), hit)
    assert ratios(g[1][keep], m["grad"][1][keep], m["k_grad"][1][keep]) <= 1


@pytest.mark.parametrize("name,a", refusals(), ids=[k for k, _ in refusals()])
def test_refusals_hold_with_real_buffers(name, a):
    from sdfa_amd import _lib
    lib = _lib.lib
    need = lib.sdfa_objective_workspace_bytes(6, 45, 4, 7, 0)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")      # noqa: E731
    bufs = dict(coef=f(6, 11), compT_s=f(30, 4), means_s=f(30), compT_r=f(15, 7), means_r=f(15), truth=f(6, 45), weight=f(6),
                loss=torch.full((4,), float("nan"), device="cuda"), rec=torch.full((6, 4), float("nan"), dtype=torch.float64, device="cuda"),
                grad=torch.full((2, 6, 11), float("nan"), device="cuda"), ws=torch.zeros(need + 64, dtype=torch.uint8, device="cuda"))
    assert set(bufs) == set(POINTERS)
    rc = call_refused(lib, a, None, {k: v.data_ptr() for k, v in bufs.items()})
    assert rc == _lib.EINVAL, name
    torch.cuda.synchronize()
    for k in ("loss", "rec", "grad"):
        assert bool(torch.isnan(bufs[k]).all()), "a refused call launched something"
