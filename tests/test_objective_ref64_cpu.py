"""CPU checks of the training objective's contract (include/sdfa_objective.h): the float64 restatement tests/objective_ref64.py
is what the reference's PcaInversion, PLoss, MLoss and autograd return (against tests/golden/train_objective.npz, made by the
reference's own modules, in double to 1e-12 and in float32 within the model's error scale kappa); its analytic gradient is the
derivative of its losses (central differences in float64); sdfa_amd.objective.DynamicLossScaler walks the reference scaler's
trajectory bit for bit; the ABI of the header is bound and exported, every host-side refusal is made before a launch, and
get_loss returns the reference's keys."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import objective_ref64 as R
from gen_golden_train_objective import CASES, SCALER_STEPS, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = {"dgrad": (0, 1, 2, 3), "plain": (0, 1)}          # the fixture lists (ps, ms, pr, mr), or (ploss, mloss) for a plain head


def _term_grads(m, layout):
    """The model's grad [2][N][Kc] as d loss_i / d coef in the fixture's order: each loss only reaches its own basis' columns."""
    g = m["grad"]
    if layout == "plain":
        return [g[0], g[1]]
    ks = CASES["dgrad_unit"][2]
    out = []
    for lo, hi in ((0, ks), (ks, g.shape[2])):
        for term in (0, 1):
            z = np.zeros_like(g[term])
            z[:, lo:hi] = g[term][:, lo:hi]
            out.append(z)
    return out


def _term_kappas(m, layout, key):
    k = m[key]
    if layout == "plain":
        return [k[0], k[1]]
    ks = CASES["dgrad_unit"][2]
    out = []
    for lo, hi in ((0, ks), (ks, k.shape[2])):
        for term in (0, 1):
            z = np.zeros_like(k[term])
            z[:, lo:hi] = k[term][:, lo:hi]
            out.append(z)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_is_the_reference_in_double(golden, name):
    g = golden["train_objective"]
    c = inputs(name)
    m = R.model(c["coef"], c["bases"], c["truth"], c["weight"], c["layout"])
    slots = SLOTS[c["layout"]]
    want = g[f"{name}.f64.loss"]
    assert len(want) == len(slots)
    for i, s in enumerate(slots):
        assert abs(m["loss"][s] / want[i] - 1) <= 1e-12, (name, s, m["loss"][s], want[i])
    if c["layout"] == "plain":
        assert m["loss"][2] == m["loss"][3] == 0.0 and not m["rec"][:, 2:].any()
    assert not m["rec"][: c["coef"].shape[0] // 2, 1].any() and not m["rec"][: c["coef"].shape[0] // 2, 3].any()      # motion slots live on rows >= B
    wg = g[f"{name}.f64.grad"]
    for i, ours in enumerate(_term_grads(m, c["layout"])):
        scale = np.abs(wg[i]).max()
        assert scale > 0 and np.abs(ours - wg[i]).max() <= 1e-12 * scale, (name, i, np.abs(ours - wg[i]).max(), scale)
    # a loss does not reach the other basis' coefficients: the reference's autograd says so too
    if c["layout"] == "dgrad":
        ks = CASES[name][2]
        assert not wg[0][:, ks:].any() and not wg[1][:, ks:].any() and not wg[2][:, :ks].any() and not wg[3][:, :ks].any()
    assert np.allclose(R.losses64(c["coef"], c["bases"], c["truth"], c["weight"], c["layout"]), m["loss"], rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_float32_results_lie_within_kappa(golden, name):
    """The reference's own float32 run against the model: |difference| <= kappa, the device's error scale, alone.  (The reference
    also rounds where the device does not -- the square, the sums over 6 or 3, the triangles and the batch; objective_ref64
    counts those as ref32_extra_*, printed here for comparison and not part of the bound.)  Largest ratio over the fixture:
    0.096 on a loss, 0.117 on a gradient element."""
    g = golden["train_objective"]
    c = inputs(name)
    m = R.model(c["coef"], c["bases"], c["truth"], c["weight"], c["layout"])
    worst, worst_wide = 0.0, 0.0
    for i, s in enumerate(SLOTS[c["layout"]]):
        err = abs(g[f"{name}.f32.loss"][i] - m["loss"][s])
        ratio = err / m["k_loss"][s]
        worst, worst_wide = max(worst, ratio), max(worst_wide, err / (m["k_loss"][s] + m["ref32_extra_loss"][s]))
        assert ratio <= 1, (name, "loss", s, ratio)
    grads, kap, ext = _term_grads(m, c["layout"]), _term_kappas(m, c["layout"], "k_grad"), _term_kappas(m, c["layout"], "ref32_extra_grad")
    for i in range(len(grads)):
        err = np.abs(g[f"{name}.f32.grad"][i] - grads[i])
        assert (err[kap[i] == 0] == 0).all()
        ratio = float((err[kap[i] > 0] / kap[i][kap[i] > 0]).max())
        worst, worst_wide = max(worst, ratio), max(worst_wide, float((err[kap[i] > 0] / (kap[i] + ext[i])[kap[i] > 0]).max()))
        assert ratio <= 1, (name, "grad", i, ratio)
    print(name, "largest |reference float32 - model| / kappa =", worst, "; over kappa + the reference's own reductions:", worst_wide)
    # the bound is a bound, not a blanket: it stays a small fraction of the values it guards
    assert (m["k_loss"][list(SLOTS[c["layout"]])] <= 1e-4 * m["loss"][list(SLOTS[c["layout"]])]).all()


@pytest.mark.parametrize("name", ["dgrad_weighted", "plain_weighted", "dgrad_one_pair"])
def test_analytic_gradient_is_the_derivative_of_the_losses(name):
    c = inputs(name)
    m = R.model(c["coef"], c["bases"], c["truth"], c["weight"], c["layout"])
    grads = _term_grads(m, c["layout"])
    coef = c["coef"].astype(np.float64)
    h = 1e-6
    rs = np.random.RandomState(0)
    for _ in range(12):
        r, i = rs.randint(coef.shape[0]), rs.randint(coef.shape[1])
        up, dn = coef.copy(), coef.copy()
        up[r, i] += h
        dn[r, i] -= h
        fd = (R.losses64(up, c["bases"], c["truth"], c["weight"], c["layout"]) - R.losses64(dn, c["bases"], c["truth"], c["weight"], c["layout"])) / (2 * h)
        for k, s in enumerate(SLOTS[c["layout"]]):
            scale = max(np.abs(grads[k]).max(), 1e-30)
            assert abs(fd[s] - grads[k][r, i]) <= 1e-7 * scale, (name, r, i, s, fd[s], grads[k][r, i])


def test_scaler_walks_the_references_trajectory(golden):
    from sdfa_amd.objective import DynamicLossScaler
    rows = golden["train_objective"]["scaler.rows"]
    assert rows.shape == (len(SCALER_STEPS), 6) and rows[:, 1].tolist() == [1.0, 1.0, 1.0, 0.0]
    sc = DynamicLossScaler()
    assert (sc.beta, sc.eps, sc.vt, sc.beta_t, sc.scale) == (0.99, 1e-8, 0.0, 1.0, 1.0)
    for k, (loss, training, vt, beta_t, scale, scaled) in enumerate(rows.tolist()):
        assert float(np.float32(loss)) == loss                                   # the fixture's losses are float32 values
        got = sc.scale_loss(torch.tensor(loss, dtype=torch.float32), bool(training))
        assert (sc.vt, sc.beta_t, sc.scale) == (vt, beta_t, scale), (k, sc.state_dict(), vt, beta_t, scale)
        assert float(got) == scaled, (k, float(got), scaled)
        if k == 1:                                                               # a run can resume from the saved state
            sc = DynamicLossScaler(beta=0.5).load_state_dict(sc.state_dict())
    assert rows[3, 2:5].tolist() == rows[2, 2:5].tolist()                        # the eval step leaves the state alone
    plain = DynamicLossScaler()
    plain.update(rows[0, 0])
    assert plain.scale == rows[0, 4]


def test_objective_abi_is_bound_and_exported():
    from sdfa_amd import _lib, objective, score, pca
    hdr = open(os.path.join(ROOT, "include", "sdfa_objective.h")).read()
    declared = set(re.findall(r"\b(sdfa_objective[a-z0-9_]*)\s*\(", hdr))
    assert declared and declared == set(objective.SYMBOLS), declared ^ set(objective.SYMBOLS)
    assert _lib.lib.sdfa_objective_abi_version() == objective.ABI_VERSION == int(re.search(r"#define SDFA_OBJECTIVE_ABI_VERSION\s+(\d+)", hdr).group(1))
    for other in (_lib, pca, score):
        assert not declared & set(other.SYMBOLS), "objective symbols belong to their own header"
    for name, const in (("MAX_K", objective.MAX_K), ("COLS", objective.COLS), ("PAIRS", objective.PAIRS), ("KSTEP", objective.KSTEP),
                        ("LAYOUT_DGRAD", objective.LAYOUT_DGRAD), ("LAYOUT_PLAIN", objective.LAYOUT_PLAIN)):
        assert int(re.search(rf"#define SDFA_OBJECTIVE_{name}\s+(\d+)", hdr).group(1)) == const
    assert objective.MAX_K >= 192 and (objective.LAYOUT_DGRAD, objective.LAYOUT_PLAIN) == (score.LAYOUT_DGRAD, score.LAYOUT_PLAIN)
    assert _lib.lib.sdfa_abi_version() == _lib.ABI_VERSION                       # the main ABI did not move


POINTERS = ("coef", "compT_s", "means_s", "compT_r", "means_r", "truth", "weight", "loss", "rec", "grad", "ws")


def refusals():
    """(name, arguments) that only the host checks can answer."""
    ok = dict(N=6, W=45, Ks=4, Kr=7, layout=0, ws=None, null=None, ws_ptr=None)
    cases = {"odd N": dict(N=5), "N below 2": dict(N=0), "negative N": dict(N=-2), "dgrad width": dict(W=44), "no width": dict(W=0, layout=1),
             "Ks below 1": dict(Ks=0), "Ks above the cap": dict(Ks=193), "Kr below 1": dict(Kr=0), "Kr above the cap": dict(Kr=193),
             "plain K above the cap": dict(layout=1, Ks=193, Kr=0), "unknown layout": dict(layout=2), "short workspace": dict(ws=-1),
             "misaligned workspace": dict(ws_ptr=256 + 64)}
    for p in POINTERS:
        cases["null " + p] = dict(null=p)
    return [(k, {**ok, **v}) for k, v in cases.items()]


def call_refused(lib, a, ptr, real=None):
    """Calls sdfa_objective with `ptr` (a dummy address when there is no device: a refusal never touches it) for every pointer;
    `real` maps pointer names to device addresses."""
    need = lib.sdfa_objective_workspace_bytes(6, 45, 4, 7, 0)
    assert need > 0
    p = {k: ptr for k in POINTERS}
    p.update(real or {})
    if a["ws_ptr"] is not None:
        p["ws"] = real["ws"] + 64 if real else a["ws_ptr"]               # (a real workspace is allocated 64 bytes larger)
    if a["null"]:
        p[a["null"]] = None
    return lib.sdfa_objective(p["coef"], a["N"], a["W"], a["Ks"], a["Kr"], a["layout"], p["compT_s"], p["means_s"], p["compT_r"], p["means_r"],
                              p["truth"], p["weight"], p["loss"], p["rec"], p["grad"], p["ws"], need + (a["ws"] or 0), None)


@pytest.mark.parametrize("name,a", refusals(), ids=[k for k, _ in refusals()])
def test_refusals_are_made_on_the_host(name, a):
    from sdfa_amd import _lib, objective  # noqa: F401
    rc = call_refused(_lib.lib, a, 256)                      # 256: aligned and never to be dereferenced
    assert rc == _lib.EINVAL, name
    assert _lib.lib.sdfa_last_error().decode().startswith("objective:")


def test_plain_needs_no_rotat_basis_and_the_cap_is_accepted():
    """The counterpart of the refusals: what must NOT be refused, asked of the size function (no launch)."""
    from sdfa_amd import _lib, objective
    lib = _lib.lib
    assert lib.sdfa_objective_workspace_bytes(2, 1, 1, 0, 1) > 0                 # one pair, one column, one coefficient
    assert lib.sdfa_objective_workspace_bytes(2, 9, 1, 1, 0) > 0
    assert lib.sdfa_objective_workspace_bytes(100, 89784, objective.MAX_K, objective.MAX_K, 0) > 0
    assert lib.sdfa_objective_workspace_bytes(100, 15069, 59, -5, 1) > 0         # Kr is ignored for plain
    assert lib.sdfa_objective_workspace_bytes(100, 15069, 59, 0, 0) == _lib.EINVAL
    w = [lib.sdfa_objective_workspace_bytes(n, 89784, 85, 180, 0) for n in (2, 100, 2048)]
    assert all(x > 0 and x % 256 == 0 for x in w)
    assert lib.sdfa_objective_workspace_bytes(3, 89784, 85, 180, 0) == _lib.EINVAL


class _HP(dict):
    __getattr__ = dict.__getitem__

    def get(self, k, default=None):
        return self[k] if k in self else default


def _saber(face, loss):
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    hp = _HP(model=_HP(face_data_type=face, prediction_type="face_data"), dataset_anime=_HP(speakers={}, emotions={}))
    if loss is not None:
        hp["loss"] = _HP(loss)
    return SaberSpeechDrivenAnimation(hp)


@pytest.mark.parametrize("face", ["dgrad_3d", "verts_off_3d"])
@pytest.mark.parametrize("dynamic", [True, False, None])
def test_get_loss_returns_the_references_keys(face, dynamic):
    """The device call is stubbed with a differentiable stand-in (the sum of the coefficients times fixed factors): the keys, the
    scales, the scalers' use of self.training and the weights' default are host logic."""
    loss_hp = None if dynamic is None else dict(dynamic_scalar=dynamic, ploss_scale=2, mloss_scale=3, anime_loss_weight=None)
    m = _saber(face, loss_hp)
    seen = {}

    def stub(coef, truth, weight):
        seen["weight"] = weight
        f = torch.tensor([1.0, 2.0, 3.0, 4.0]) if face == "dgrad_3d" else torch.tensor([1.0, 2.0, 0.0, 0.0])
        return coef.sum() * f
    m._train_losses = stub
    coef = torch.full((4, 3), 0.25, requires_grad=True)
    key = "dgrad_3d_coef" if face == "dgrad_3d" else "verts_off_3d_coef"
    batch = dict(face_data=torch.zeros(4, 9), audio_feat=torch.zeros(4, 1), anime_weight=torch.full((4,), 5.0))
    m.train()
    losses, scalars = m.get_loss(dict(prediction={key: coef}), batch)
    assert torch.equal(seen["weight"], torch.ones(4))                            # anime_loss_weight None: ones
    dyn = dynamic is not False                                                   # the reference's default is dynamic
    ps, ms = (2.0, 3.0) if dynamic is not None else (1.0, 1.0)
    if face == "dgrad_3d":
        names = ("ps", "ms", "pr", "mr")
        assert set(scalars) == {"scalar_ps", "scalar_ms", "scalar_pr", "scalar_mr", "scalar_ploss", "scalar_mloss"}
        assert scalars["scalar_ploss"] == scalars["scalar_ps"] + scalars["scalar_pr"] == 3.0 + 9.0
        assert scalars["scalar_mloss"] == scalars["scalar_ms"] + scalars["scalar_mr"] == 6.0 + 12.0
        scalers = ("dyn_p_scale", "dyn_m_scale", "dyn_p_rotat", "dyn_m_rotat")
    else:
        names = ("ploss", "mloss")
        assert scalars == {"scalar_ploss": 3.0, "scalar_mloss": 6.0}
        scalers = ("dyn_p", "dyn_m")
    assert set(losses) == {("dyn_" if dyn else "loss_") + n for n in names}
    assert "dyn_eloss" not in losses and "scalar_eloss" not in scalars            # no evector: ELoss stays absent
    for i, n in enumerate(names):
        raw = 3.0 * (i + 1)
        mult = ps if n[0] == "p" else ms
        if dyn:
            # first training step: scale = sqrt((1 - beta) loss^2 / (1 - beta)) + eps = |loss| + eps
            assert set(m._loss_scalers) == set(scalers)
            assert float(losses["dyn_" + n].detach()) == pytest.approx(raw / (raw + 1e-8) * mult, rel=1e-6)
        else:
            assert float(losses["loss_" + n].detach()) == pytest.approx(raw * mult, rel=1e-6) and not m._loss_scalers
    sum(losses.values()).backward()
    assert coef.grad is not None and coef.grad.shape == coef.shape and (coef.grad != 0).all()
    if dyn:
        before = {k: v.state_dict() for k, v in m._loss_scalers.items()}
        m.eval()
        m.get_loss(dict(prediction={key: coef}), batch)
        assert before == {k: v.state_dict() for k, v in m._loss_scalers.items()}  # eval leaves the scalers alone
    m2 = _saber(face, dict(anime_loss_weight="anime_weight"))
    m2._train_losses = stub
    m2.get_loss(dict(prediction={key: coef}), batch)
    assert torch.equal(seen["weight"], batch["anime_weight"])
