"""torch.ops.sdfa.train_losses (sdfa_amd/ops.py) and SaberSpeechDrivenAnimation.get_loss on the synthetic heads, on the GPU.

torch.autograd.gradcheck does not apply (the operator is float32): instead the operator's backward is compared bitwise with the
saved gradients combined by hand, and the losses and gradients with the torch route in the same process -- the engine's own
expanded rows (engine.expand_coef, what sdfa::regress writes), the criterion restated in torch float32, autograd to the rows,
the rows' gradients carried to the coefficients by a float64 product -- within the kappa of tests/objective_ref64.py.  get_loss
on a train_batch of each head returns scalars that equal the recomputation from the records in float64.  Three Adam steps on a
free-standing Linear feeding the operator are held against the same steps on the torch route: the parameter gradients and the
first step's directions against the model, the loss trajectories within kappa plus a bound on how far Adam can part them.

This module fails to import without sdfa_amd.objective."""
import numpy as np
import pytest
import torch

import objective_ref64 as R
from sdfa_amd import objective as O          # the feature: absent before it
from sdfa_amd import ops, synth

pytestmark = pytest.mark.gpu

B = 3


@pytest.fixture(scope="module")
def heads(synth_sd):
    """{head: (engine, model key, Bases, host bases dict, layout name)}"""
    from sdfa_amd.engine import Engine
    out = {}
    for head in ("dgrad", "offsets"):
        eng = Engine(synth_sd[head], device="cuda:0", max_frames=256)
        key = ops.register_model(None, eng)
        with pytest.raises(KeyError):
            O.bases_of(eng)                                   # an engine pays nothing until it is opted in
        bases = O.attach_bases(eng, synth_sd[head])
        assert O.bases_of(eng) is bases                       # kept once per model
        host = {k: getattr(bases, k).cpu().numpy() for k in ("compT_s", "means_s") + (("compT_r", "means_r") if head == "dgrad" else ())}
        out[head] = (eng, key, bases, host, "dgrad" if head == "dgrad" else "plain")
    return out


def batch_of(bases, host, layout, seed, coef_scale=10.0):
    """Seeded coefficients, truth near another prediction, weights on 0.2 .. 2, on the device and on the host."""
    rs = np.random.RandomState(seed)
    N = 2 * B
    coef = (rs.normal(0, 1, (N, bases.Kc)) * coef_scale).astype(np.float32)
    other = rs.normal(0, 1, (N, bases.Kc)) * coef_scale
    truth = np.zeros((N, bases.W))
    for compT, means, sl, cols, _ in R.parts_of(host, layout, bases.W):
        truth[:, cols] = other[:, sl] @ compT.astype(np.float64).T + means
    truth = (truth + rs.normal(0, 0.01, truth.shape)).astype(np.float32)
    weight = (np.round(rs.uniform(0.2, 2.0, N) * 1024) / 1024).astype(np.float32)
    return coef, truth, weight


def torch_criterion(rows, truth, weight, layout):
    """PLoss / MLoss (criterion.py:7-73) on expanded rows, float32 torch operations: [ps, ms, pr, mr] (plain: [ploss, mloss])."""
    N = rows.shape[0]
    h = weight[N // 2:] + weight[:N // 2]
    out = []
    if layout == "dgrad":
        tri_p, tri_t = rows.view(N, 1, -1, 9), truth.view(N, 1, -1, 9)
        parts = ((tri_p[..., :6], tri_t[..., :6], False), (tri_p[..., 6:], tri_t[..., 6:], True))
    else:
        parts = ((rows.view(N, 1, -1), truth.view(N, 1, -1), False),)
    for p, t, use_exp in parts:
        if use_exp:
            p, t = torch.exp(p), torch.exp(t)

        def reduce(x):
            if layout == "dgrad":
                x = x.sum(-1)
            while x.dim() > 1:
                x = x.mean(-1)
            return x
        out.append((reduce(torch.nn.functional.mse_loss(p, t, reduction="none")) * weight).mean(dim=0))
        mp, mt = p[N // 2:] - p[:N // 2], t[N // 2:] - t[:N // 2]
        out.append((reduce(torch.nn.functional.mse_loss(mp, mt, reduction="none")) * h).mean(dim=0))
    return out


def slots_of(layout):
    return (0, 1, 2, 3) if layout == "dgrad" else (0, 1)


@pytest.mark.parametrize("head", ["dgrad", "offsets"])
def test_backward_is_the_saved_gradients_combined_by_hand(heads, head):
    eng, key, bases, host, layout = heads[head]
    coef, truth, weight = (torch.from_numpy(x).cuda() for x in batch_of(bases, host, layout, 41))
    loss_t, rec_t, grad_t = torch.ops.sdfa.objective(coef, truth, weight, key)
    c = coef.clone().requires_grad_(True)
    loss = torch.ops.sdfa.train_losses(c, truth, weight, key)
    assert loss.shape == (4,) and loss.requires_grad and torch.equal(loss.detach(), loss_t)
    g = torch.tensor([0.75, 1.5, -2.0, 0.3], device="cuda")
    (loss * g).sum().backward()
    kr = bases.Kc - bases.Ks
    cp = torch.cat((g[0].expand(bases.Ks), g[2].expand(kr)))
    cm = torch.cat((g[1].expand(bases.Ks), g[3].expand(kr)))
    by_hand = grad_t[0] * cp + grad_t[1] * cm
    assert torch.equal(c.grad, by_hand)
    assert torch.equal(by_hand, ops.combine_grads(g, grad_t, bases.Ks))
    # one loss at a time reaches only its own basis' columns
    for i in slots_of(layout):
        c.grad = None
        torch.ops.sdfa.train_losses(c, truth, weight, key)[i].backward()
        lo, hi = (0, bases.Ks) if i < 2 else (bases.Ks, bases.Kc)
        assert torch.equal(c.grad[:, lo:hi], grad_t[i & 1][:, lo:hi]) and c.grad[:, lo:hi].abs().max() > 0
        rest = torch.ones(bases.Kc, dtype=torch.bool, device="cuda")
        rest[lo:hi] = False
        assert not c.grad[:, rest].any()
    # the fake-tensor function: shapes and dtypes without a launch
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        f = [mode.from_tensor(t) for t in (coef, truth, weight)]
        fl, fr, fg = torch.ops.sdfa.objective(*f, key)
        assert tuple(fl.shape) == (4,) and fr.dtype == torch.float64 and tuple(fr.shape) == (2 * B, 4) and tuple(fg.shape) == (2, 2 * B, bases.Kc)
        assert tuple(torch.ops.sdfa.train_losses(*f, key).shape) == (4,)


@pytest.mark.parametrize("head", ["dgrad", "offsets"])
def test_against_the_torch_route_within_kappa(heads, head):
    """Both routes against the float64 model, each within kappa alone.  The largest ratios are printed (the torch route's also
    over kappa plus objective_ref64.ref32_extra_*, the float32 reductions only it makes: for comparison, part of no bound)."""
    eng, key, bases, host, layout = heads[head]
    coef_h, truth_h, weight_h = batch_of(bases, host, layout, 42)
    coef, truth, weight = (torch.from_numpy(x).cuda() for x in (coef_h, truth_h, weight_h))
    m = R.model(coef_h, host, truth_h, weight_h, layout)
    loss, rec, grad = torch.ops.sdfa.objective(coef, truth, weight, key)
    rows = eng.expand_coef(coef).detach().requires_grad_(True)
    terms = torch_criterion(rows, truth, weight, layout)
    A = {s: torch.from_numpy(host["compT_" + s]).cuda().double() for s in (("s", "r") if layout == "dgrad" else ("s",))}
    worst_op, worst_torch, worst_torch_k = 0.0, 0.0, 0.0
    for i, s in zip(range(len(terms)), slots_of(layout)):
        worst_op = max(worst_op, abs(float(loss[s]) - m["loss"][s]) / m["k_loss"][s])
        err = abs(float(terms[i].detach()) - m["loss"][s])
        worst_torch = max(worst_torch, err / (m["k_loss"][s] + m["ref32_extra_loss"][s]))
        worst_torch_k = max(worst_torch_k, err / m["k_loss"][s])
        (grows,) = torch.autograd.grad(terms[i], rows, retain_graph=True)
        grows = grows.double()
        if layout == "dgrad":
            tri = grows.view(2 * B, -1, 9)
            part, lo, hi = (tri[..., :6].reshape(2 * B, -1), 0, bases.Ks) if s < 2 else (tri[..., 6:].reshape(2 * B, -1), bases.Ks, bases.Kc)
            gt = (part @ A["s" if s < 2 else "r"]).cpu().numpy()
        else:
            lo, hi = 0, bases.Kc
            gt = (grows @ A["s"]).cpu().numpy()
        want, kap, ext = m["grad"][s & 1][:, lo:hi], m["k_grad"][s & 1][:, lo:hi], m["ref32_extra_grad"][s & 1][:, lo:hi]
        worst_op = max(worst_op, float((np.abs(grad[s & 1][:, lo:hi].cpu().numpy() - want) / kap).max()))
        worst_torch = max(worst_torch, float((np.abs(gt - want) / (kap + ext)).max()))
        worst_torch_k = max(worst_torch_k, float((np.abs(gt - want) / kap).max()))
    print(f"{head}: operator / kappa {worst_op:.4f}; torch route / kappa {worst_torch_k:.4f}, / (kappa + float32 reductions) {worst_torch:.4f}")
    assert worst_op <= 1 and worst_torch_k <= 1


def _train_set(width, sr=16000):
    from speech_anime import hparams as H
    from speech_anime.datasets.sliding_window import SOURCES, TrainSet
    rs = np.random.RandomState(9)
    clips, tracks = [], []
    for L, seed, kind, spk, start_ts, minfi, maxfi in ((9600, 70, "speechlike", "m0", 37.5, 3, 40), (7200, 74, "uniform", "f1", 0.0, 0, 30)):
        c = dict(sr=sr, speaker_id=H.DEFAULTS["dataset_anime"]["speakers"][spk], start_ts=start_ts, anime_minfi=minfi, anime_maxfi=maxfi)
        for si, s in enumerate(SOURCES):
            c[s] = synth.make_pcm(seed + si, L // 2 if s.endswith("_8k") else L, kind)
        clips.append(c)
        n = maxfi - minfi + 1
        track = (np.cumsum(rs.normal(0, 0.01, (n, width)), axis=0) + rs.normal(0, 0.05, (1, width))).astype(np.float32)
        tracks.append((track, rs.uniform(0.0, 0.02, n).astype(np.float32)))
    return TrainSet(clips, tracks, sr)


@pytest.mark.parametrize("head,dynamic", [("dgrad", True), ("offsets", False)])
def test_get_loss_on_a_train_batch(synth_sd, head, dynamic):
    from speech_anime import hparams as H
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    hp = H.configure({"custom_hparams": head})
    hp.audio.set_key("sample_rate", 16000)
    hp.set_key("loss", dict(ploss_scale=1, mloss_scale=2, dynamic_scalar=dynamic, anime_loss_weight="anime_weight"))
    model = SaberSpeechDrivenAnimation(hp).load_state_dict(synth_sd[head]).enable_training_objective(synth_sd[head])
    eng, key = model._model._engine, model._model._key
    ts = _train_set(eng.out_dim)
    torch.cuda.manual_seed(20)                                # the batch's white noise is torch.randn on the device: the same batch in every process
    batch = DSW.train_batch(ts, None, [0, 11, 47], np.random.RandomState(3), hparams=hp)
    z, _ = torch.ops.sdfa.encoder(batch["audio_feat"], key)
    coef = torch.ops.sdfa.regress_coef(z, batch["speaker_id"], key).clone().requires_grad_(True)
    name = "dgrad_3d_coef" if head == "dgrad" else "verts_off_3d_coef"
    model.train()
    losses, scalars = model.get_loss(dict(prediction={name: coef}), batch)
    bases = O.bases_of(eng)
    _, rec, grad = torch.ops.sdfa.objective(coef.detach(), batch["face_data"], batch["anime_weight"], key)
    want = O.scalars_of(rec, batch["anime_weight"], bases.n)
    if head == "dgrad":
        assert set(losses) == ({"dyn_ps", "dyn_ms", "dyn_pr", "dyn_mr"} if dynamic else {"loss_ps", "loss_ms", "loss_pr", "loss_mr"})
        for k in ("ps", "ms", "pr", "mr"):
            assert scalars["scalar_" + k] == pytest.approx(want[k], rel=1e-6) and want[k] > 0
        assert scalars["scalar_ploss"] == scalars["scalar_ps"] + scalars["scalar_pr"] and scalars["scalar_mloss"] == scalars["scalar_ms"] + scalars["scalar_mr"]
    else:
        assert set(losses) == ({"dyn_ploss", "dyn_mloss"} if dynamic else {"loss_ploss", "loss_mloss"})
        assert scalars["scalar_ploss"] == pytest.approx(want["ps"], rel=1e-6) and scalars["scalar_mloss"] == pytest.approx(want["ms"], rel=1e-6)
        assert want["pr"] == want["mr"] == 0.0 and want["ps"] > 0
    for v in losses.values():
        assert v.is_cuda and v.dim() == 0 and v.requires_grad
    sum(losses.values()).backward()
    # the objective's gradient is the two terms over their scales (first training step: scale = |loss| + eps), times the hparams' factors
    vals = [want[k] for k in O.LOSS_NAMES]
    if dynamic:
        f = [1.0 / (abs(float(np.float32(v))) + 1e-8) if v else 0.0 for v in vals]
    else:
        f = [1.0] * 4
    gl = torch.tensor([f[0] * 1.0, f[1] * 2.0, f[2] * 1.0, f[3] * 2.0], dtype=torch.float32, device="cuda")
    expect = ops.combine_grads(gl, grad, bases.Ks)
    assert torch.allclose(coef.grad, expect, rtol=1e-5, atol=0) and coef.grad.abs().max() > 0


def adam_ratio(t, b1=0.9, b2=0.999):
    """Largest |m^_t| / sqrt(v^_t) Adam can form at step t, whatever the gradients: by Cauchy-Schwarz on
    m_t = (1 - b1) sum_i b1^(t-i) g_i against v_t = (1 - b2) sum_i b2^(t-i) g_i^2, with both bias corrections.  1 at t = 1."""
    s = sum((b1 * b1 / b2) ** j for j in range(t))
    return (1 - b1) / (1 - b1 ** t) * np.sqrt(s) * np.sqrt((1 - b2 ** t) / (1 - b2))


def drift_bound(res_a, res_b, reach, weight_h, n):
    """How far the four float64 losses of two coefficient sets can lie apart when row r's coefficients differ by at most
    reach[r] per element -- a quantity known before the run.  The predicted arguments then differ by at most
    rho[r][col] = reach[r] sum_k |compT[col][k]|, the e() values by rho (scale) or max(e_a, e_b) rho (rotat: the mean value
    theorem), a motion residual by the sum over its two rows, and q_a^2 - q_b^2 = (q_a - q_b)(q_a + q_b) exactly."""
    w, h = np.asarray(weight_h, np.float64), R.half_weights(weight_h)
    N = w.shape[0]
    Bh = N // 2
    out = np.zeros(4)
    for pi, ((ea, da, ma, absA), (eb, db, mb, _)) in enumerate(zip(res_a, res_b)):
        rho = reach[:, None] * absA.sum(1)[None, :]
        de = rho * np.maximum(ea, eb) if pi == 1 else rho
        out[2 * pi] = (w * (de * (np.abs(da) + np.abs(db))).sum(1)).sum() / (N * n)
        out[2 * pi + 1] = (h * ((de[Bh:] + de[:Bh]) * (np.abs(ma) + np.abs(mb))).sum(1)).sum() / (Bh * n)
    return out


def test_three_adam_steps_follow_the_torch_route(heads):
    """A free-standing Linear(256, Kc) feeds the operator; a copy feeds the torch route (F.linear with the basis, view, exp,
    mse_loss, backward()); both take three Adam steps (lr = 1e-4) from the same parameters.

    The gradient as Adam consumes it (first step, where both routes stand at the same coefficients): each route's parameter
    gradient d objective / d weight = gcoef^T x lies within its propagated bound of the float64 model's -- kappa of the two
    gradient terms, the float32 addition of the terms and the (N + 2) roundings of the float32 product with x -- and every
    parameter whose model gradient exceeds that bound moves against its sign, in both routes (Adam's first step is
    -lr g / (|g| + eps)).  A gradient wrong in sign, scale or column fails here.

    The trajectory: Adam normalises each element, so where a gradient element is smaller than its error the routes may step in
    opposite directions; no kappa of the losses bounds that.  What is known in advance is how far Adam can move a parameter:
    lr adam_ratio(t) at step t.  After s steps two routes' parameters differ by at most 2 lr sum_t adam_ratio(t) (plus the
    float32 rounding of the updates), row r's coefficients by that times (|x_r|_1 + 1), and drift_bound turns this reach into
    a bound on the distance of the float64 losses.  Asserted at every step: each route within kappa of the model at its own
    coefficients; the model's drift between the two coefficient sets within drift_bound; |L_op - L_torch| within the two
    kappas plus drift_bound.  The objective after the third step is lower than before the first, in both routes."""
    eng, key, bases, host, layout = heads["dgrad"]
    _, truth_h, weight_h = batch_of(bases, host, layout, 43)
    truth, weight = torch.from_numpy(truth_h).cuda(), torch.from_numpy(weight_h).cuda()
    torch.manual_seed(0)
    x = torch.randn(2 * B, 256, device="cuda")
    lin_op = torch.nn.Linear(256, bases.Kc).cuda()
    with torch.no_grad():
        lin_op.weight.mul_(5.0)                               # coefficients of the heads' size
    lin_t = torch.nn.Linear(256, bases.Kc).cuda()
    lin_t.load_state_dict(lin_op.state_dict())
    lr = 1e-4
    opt_op, opt_t = torch.optim.Adam(lin_op.parameters(), lr=lr), torch.optim.Adam(lin_t.parameters(), lr=lr)
    As, ms_ = torch.from_numpy(host["compT_s"]).cuda(), torch.from_numpy(host["means_s"]).cuda()
    Ar, mr_ = torch.from_numpy(host["compT_r"]).cuda(), torch.from_numpy(host["means_r"]).cuda()
    x64 = x.cpu().numpy().astype(np.float64)
    theta_max = float(max(lin_op.weight.detach().abs().max(), lin_op.bias.detach().abs().max()))

    def torch_route(coef):
        N = coef.shape[0]
        s = torch.nn.functional.linear(coef[:, :bases.Ks], As, ms_).view(N, -1, 6)
        r = torch.nn.functional.linear(coef[:, bases.Ks:], Ar, mr_).view(N, -1, 3)
        return torch.stack(torch_criterion(torch.cat((s, r), dim=-1).view(N, -1), truth, weight, layout))

    traj = []
    for step in range(4):                                     # three optimiser steps; the fourth pass only evaluates
        c_op, c_t = lin_op(x), lin_t(x)
        l_op, l_t = torch.ops.sdfa.train_losses(c_op, truth, weight, key), torch_route(c_t)
        ch_op, ch_t = c_op.detach().cpu().numpy(), c_t.detach().cpu().numpy()
        m_op, m_t = R.model(ch_op, host, truth_h, weight_h, layout), R.model(ch_t, host, truth_h, weight_h, layout)
        lo, lt = l_op.detach().cpu().numpy().astype(np.float64), l_t.detach().cpu().numpy().astype(np.float64)
        r_op = float((np.abs(lo - m_op["loss"]) / m_op["k_loss"]).max())
        r_t = float((np.abs(lt - m_t["loss"]) / m_t["k_loss"]).max())
        moved = 2 * lr * sum(adam_ratio(t) for t in range(1, step + 1)) + 2 * step * R.U * (theta_max + step * 2 * lr)
        reach = moved * (np.abs(x64).sum(1) + 1)
        bound = drift_bound(R.residuals64(ch_op, host, truth_h, layout), R.residuals64(ch_t, host, truth_h, layout), reach, weight_h, bases.n)
        drift = np.abs(m_op["loss"] - m_t["loss"])
        print(f"step {step}: operator / kappa {r_op:.4f}, torch route / kappa {r_t:.4f}, objective {lo.sum():.9g} vs {lt.sum():.9g}, "
              f"model drift {drift.max():.3g} of at most {bound.max():.3g}, largest drift / bound {(drift[bound > 0] / bound[bound > 0]).max() if step else 0.0:.3g}")
        assert r_op <= 1 and r_t <= 1
        assert (drift <= bound).all(), (step, drift, bound)
        assert (np.abs(lo - lt) <= m_op["k_loss"] + m_t["k_loss"] + bound).all()
        traj.append((lo.sum(), lt.sum()))
        if step < 3:
            before = [(lin.weight.detach().clone(), lin.bias.detach().clone()) for lin in (lin_op, lin_t)]
            for opt, l in ((opt_op, l_op), (opt_t, l_t)):
                opt.zero_grad()
                l.sum().backward()
            if step == 0:                                     # both routes at the same coefficients: m_op is the model of both
                assert np.array_equal(ch_op, ch_t)
                g0, g1 = m_op["grad"][0], m_op["grad"][1]
                gc, dgc = g0 + g1, m_op["k_grad"][0] + m_op["k_grad"][1] + 2 * R.U * (np.abs(g0) + np.abs(g1))
                gw = gc.T @ x64                                                              # [Kc][256]
                dgw = dgc.T @ np.abs(x64) + (2 * B + 2) * R.U * (np.abs(gc).T @ np.abs(x64))
                gb, dgb = gc.sum(0), dgc.sum(0) + (2 * B + 2) * R.U * np.abs(gc).sum(0)
                for name, lin in (("operator", lin_op), ("torch", lin_t)):
                    rw = float((np.abs(lin.weight.grad.cpu().numpy() - gw) / dgw).max())
                    rb = float((np.abs(lin.bias.grad.cpu().numpy() - gb) / dgb).max())
                    print(f"step 0, {name}: |parameter gradient - model| / bound: weight {rw:.4f}, bias {rb:.4f}")
                    assert rw <= 1 and rb <= 1, (name, rw, rb)
            opt_op.step()
            opt_t.step()
            if step == 0:
                sure = np.abs(gw) > dgw
                assert sure.mean() > 0.5, sure.mean()                                        # not vacuous: most parameters have a determined sign
                for (w0, _), lin in zip(before, (lin_op, lin_t)):
                    dw = (lin.weight.detach() - w0).cpu().numpy()
                    assert (np.sign(dw[sure]) == -np.sign(gw[sure])).all()
    assert traj[3][0] < traj[0][0] and traj[3][1] < traj[0][1]
