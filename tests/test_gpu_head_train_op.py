"""torch.ops.sdfa.head_train (sdfa_amd/ops.py) and the head-training surface of SaberSpeechDrivenAnimation -- train_step, fit_head,
head_state_dict, commit_head -- on the synthetic offsets head, on the GPU.

The operator under loss.backward() leaves the gradient bits of the direct sdfa_headtrain calls.  One train_step + get_loss +
optimizer_step on the two-clip synthetic TrainSet of tests/test_gpu_train_losses.py gives the parameters of the float64 model
(tests/headtrain_ref64.py, fed the z and the d loss / d coef the device produced) within kappa.  commit_head() then makes an
inference engine whose regress_coef agrees with the trainer's forward within the forward's kappa.  Twenty steps of fit_head on
a fixed batch lower scalar_ploss.  A trainer restored from state_dict() continues bit for bit.

This module fails to import without sdfa_amd.headtrain."""
import numpy as np
import pytest
import torch

import headtrain_ref64 as R
from sdfa_amd import headtrain as HT          # the feature: absent before it
from test_gpu_train_losses import _train_set

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _device_rng_left_as_found():
    """train_batch's device noise draws from torch's global CUDA generator: this module hands it back as it found it, so the
    modules that run after it see the stream they saw before this one existed."""
    state = torch.cuda.get_rng_state()
    yield
    torch.cuda.set_rng_state(state)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_operator_backward_leaves_the_direct_calls_gradients():
    c = R.case("dgrad", 3, 77, (0, 1, 2, 3, 4, 6, 7))
    z, sid, dcoef = torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["sid"]).cuda(), torch.from_numpy(c["dcoef"]).cuda()
    a, b = HT.HeadTrainer(c["params"], "dgrad"), HT.HeadTrainer(c["params"], "dgrad")
    coef_a = a.forward(z, sid)
    dz_a = a.backward(dcoef)
    key = HT.register_trainer(b)
    zz = z.clone().requires_grad_(True)
    coef_b = torch.ops.sdfa.head_train(zz, sid, key)
    assert coef_b.requires_grad and torch.equal(coef_a, coef_b.detach())
    (coef_b * dcoef).sum().backward()
    assert torch.equal(zz.grad, dz_a)
    ga, gb = a.grads(), b.grads()
    for n in ga:
        assert (bits(ga[n]) == bits(gb[n])).all() and np.abs(ga[n]).max() > 0, n
    with pytest.raises(KeyError):
        torch.ops.sdfa.head_train(zz, sid, "no such trainer")
    fake = torch.library.opcheck(torch.ops.sdfa.head_train.default, (z, sid, key), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake


@pytest.fixture(scope="module")
def tuned(synth_sd):
    """An offsets model after one train_step + optimizer_step on a train_batch, with everything the checks need."""
    from speech_anime import hparams as H
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    hp = H.configure({"custom_hparams": "offsets"})
    hp.audio.set_key("sample_rate", 16000)
    hp.set_key("loss", dict(ploss_scale=1, mloss_scale=1, dynamic_scalar=True, anime_loss_weight="anime_weight"))
    sd = synth_sd["offsets"]
    model = SaberSpeechDrivenAnimation(hp).load_state_dict(sd).enable_head_training(sd)
    ts = _train_set(model._model._engine.out_dim)
    batch = DSW.train_batch(ts, None, [0, 11, 47], np.random.RandomState(3), hparams=hp)
    before = model._head_trainer.parameters()
    pred, losses, scalars = model.train_step(batch, 0)
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    model.optimizer_step()
    return dict(model=model, hp=hp, ts=ts, batch=batch, before=before, coef=coef.detach(), dcoef=coef.grad.detach().clone(),
                z=pred["condition"].detach().reshape(-1, 512), scalars=scalars, losses=losses)


def test_train_step_and_one_adam_step_within_kappa(tuned):
    m = tuned["model"]
    assert set(tuned["losses"]) == {"dyn_ploss", "dyn_mloss"} and tuned["scalars"]["scalar_ploss"] > 0
    assert m.training and m._head_trainer.step_count == 1
    z, sid = tuned["z"].cpu().numpy(), tuned["batch"]["speaker_id"].cpu().numpy()
    r = R.run("offsets", tuned["before"], z, sid, tuned["dcoef"].cpu().numpy())
    d = np.abs(tuned["coef"].cpu().numpy() - r["coef"])
    assert (d <= r["k_coef"]).all()
    got = m._head_trainer.parameters()
    worst = float((d / r["k_coef"]).max())
    for n, g in r["grads"].items():
        p1, _, _, kp, _, _ = R.adam(tuned["before"][n], g, 0.0 * g, 0.0 * g, 1, eg=r["k_grads"][n])
        d = np.abs(got[n].astype(np.float64) - p1.reshape(got[n].shape))
        kp = kp.reshape(got[n].shape)
        assert (d <= kp).all(), (n, float((d / np.maximum(kp, 1e-300)).max()))
        worst = max(worst, float((d[kp > 0] / kp[kp > 0]).max()))
        assert (got[n] != tuned["before"][n]).mean() > 0.5, n
    print(f"\ntrain_step + optimizer_step: largest |gpu - ref64| / kappa {worst:.4f}")
    names = set(m.head_state_dict())
    assert names == {"_model." + n for n in HT.tensor_shapes("offsets")}


def test_commit_head_feeds_the_tuned_head_to_inference(tuned):
    m = tuned["model"]
    old_engine = m._model._engine
    z, sid = tuned["z"], tuned["batch"]["speaker_id"]
    coef_old = torch.ops.sdfa.regress_coef(z, sid, m._model._key)
    m.commit_head()
    assert m._model._engine is not old_engine
    coef_new = torch.ops.sdfa.regress_coef(z, sid, m._model._key)
    coef_tr = m._head_trainer.forward(z, sid)
    r = R.run("offsets", m._head_trainer.parameters(), z.cpu().numpy(), sid.cpu().numpy())
    for what, got in (("engine", coef_new), ("trainer", coef_tr)):
        d = np.abs(got.cpu().numpy() - r["coef"])
        assert (d <= r["k_coef"]).all(), (what, float((d / r["k_coef"]).max()))
    d = np.abs((coef_new - coef_tr).cpu().numpy())
    assert (d <= r["k_coef"]).all()
    moved = np.abs((coef_new - coef_old).cpu().numpy())
    assert (moved > 100 * r["k_coef"]).any()                  # the engine before the commit is the untuned head
    print(f"\ncommit_head: engine vs trainer {float((d / r['k_coef']).max()):.4f} x kappa; the step moved coef by up to {float((moved / r['k_coef']).max()):.3g} x kappa")
    # generate_animation runs on the new engine
    from sdfa_amd import synth
    ts_list, animes, _ = m.generate_animation(synth.make_pcm(3, 2 * 16000), "m0", 0, 0)
    assert len(ts_list) == animes.shape[0] > 0 and np.isfinite(animes).all()


def test_fit_head_on_a_fixed_batch_lowers_the_loss(tuned):
    m = tuned["model"]
    hist = m.fit_head(tuned["ts"], 20, np.random.RandomState(1), fixed_batch=tuned["batch"])
    assert len(hist) == 20 and m._head_trainer.step_count == 21
    first, last = hist[0]["scalar_ploss"], hist[-1]["scalar_ploss"]
    print(f"\nfit_head, 20 steps on one batch: scalar_ploss {first:.6g} -> {last:.6g}")
    assert last < first
    # and over fresh batches it runs
    more = m.fit_head(tuned["ts"], 2, np.random.RandomState(2), batch_size=4)
    assert len(more) == 2 and all(np.isfinite(s["scalar_ploss"]) for s in more)


def test_state_dict_resumes_bit_for_bit():
    c = R.case("offsets", 3, 78, (0, 1, 2, 3, 4, 6, 7))
    z, sid, dcoef = torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["sid"]).cuda(), torch.from_numpy(c["dcoef"]).cuda()

    def step(tr):
        tr.forward(z, sid)
        tr.backward(dcoef, want_dz=False)
        tr.step()

    a = HT.HeadTrainer(c["params"], "offsets", lr=3e-4)
    step(a)
    step(a)
    state = a.state_dict()
    b = HT.HeadTrainer(c["params"], "offsets").load_state_dict(state)
    assert b.step_count == 2 and b.lr == 3e-4
    step(a)
    step(b)
    pa, pb = a.parameters(), b.parameters()
    (ma, va), (mb, vb) = a.moments(), b.moments()
    for n in pa:
        assert (bits(pa[n]) == bits(pb[n])).all() and (bits(ma[n]) == bits(mb[n])).all() and (bits(va[n]) == bits(vb[n])).all(), n
        assert (bits(pa[n]) != bits(c["params"][n])).any()
