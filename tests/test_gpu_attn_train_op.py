"""torch.ops.sdfa.attn_train / encoder_memory (sdfa_amd/ops.py) and attention training in SaberSpeechDrivenAnimation --
enable_head_training(attention=True), train_step, fit_head, head_state_dict, commit_head -- on the synthetic offsets model, on
the GPU.

The operator under loss.backward() leaves the gradient bits of the direct sdfa_attntrain calls; a gradient for align is refused
by name.  One train_step + get_loss + optimizer_step on the two-clip synthetic TrainSet of tests/test_gpu_train_losses.py lies
within 1 x kappa of the restated chain: the attention model (tests/attntrain_ref64.py) on the device's H gives z; the head model
(tests/headtrain_ref64.py) on that z and the objective's d loss / d coef gives dz with its kappa; the attention model's backward
takes that dz and its kappa and gives the gradients; Adam gives the parameters.  (d loss / d coef is the device's, as in
tests/test_gpu_head_train_op.py: the objective has its own float64 check in tests/test_gpu_train_losses.py.)  commit_head()
then makes an inference engine whose z agrees with the trainer's forward within kappa.  Twenty steps of fit_head on a fixed
batch with attention enabled lower scalar_ploss.  A trainer restored from state_dict() continues bit for bit.  With
attention=False train_step returns the bits of the HeadTrainer driven directly.

This module fails to import without sdfa_amd.attntrain."""
import numpy as np
import pytest
import torch

import attntrain_ref64 as R
import headtrain_ref64 as RH
from sdfa_amd import attntrain as AT          # the feature: absent before it
from sdfa_amd import headtrain as HT
from test_gpu_train_losses import _train_set

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _device_rng_left_as_found():
    """train_batch's device noise draws from torch's global CUDA generator: this module hands it back as it found it."""
    state = torch.cuda.get_rng_state()
    yield
    torch.cuda.set_rng_state(state)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_operator_backward_leaves_the_direct_calls_gradients():
    c = R.case(5, 77, "peaked")
    H, dz = torch.from_numpy(c["H"]).cuda(), torch.from_numpy(c["dz"]).cuda()
    a, b, n = AT.AttnTrainer(c["params"]), AT.AttnTrainer(c["params"]), AT.AttnTrainer(c["params"], want_dH=False)
    z_a, align_a = a.forward(H)
    dH_a = a.backward(dz)
    for tr in (b, n):
        key = AT.register_trainer(tr)
        HH = H.clone().requires_grad_(True)
        z_b, align_b = torch.ops.sdfa.attn_train(HH, key)
        assert z_b.requires_grad and torch.equal(z_a, z_b.detach()) and torch.equal(align_a, align_b.detach())
        (z_b * dz).sum().backward()
        if tr is b:
            assert torch.equal(HH.grad, dH_a)
        else:
            assert HH.grad is None                           # made with want_dH = False: the dH tiles are skipped
        ga, gb = a.grads(), tr.grads()
        for name in ga:
            assert (bits(ga[name]) == bits(gb[name])).all() and np.abs(ga[name]).max() > 0, name
    HH = H.clone().requires_grad_(True)
    z_b, align_b = torch.ops.sdfa.attn_train(HH, key)
    with pytest.raises(NotImplementedError, match="align is not differentiable"):
        (z_b.sum() + align_b[:, 0].sum()).backward()
    with pytest.raises(KeyError):
        torch.ops.sdfa.attn_train(HH, "no such trainer")
    fake = torch.library.opcheck(torch.ops.sdfa.attn_train.default, (H, key), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake


def _model(synth_sd, attention):
    from speech_anime import hparams as Hp
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    hp = Hp.configure({"custom_hparams": "offsets"})
    hp.audio.set_key("sample_rate", 16000)
    hp.set_key("loss", dict(ploss_scale=1, mloss_scale=1, dynamic_scalar=True, anime_loss_weight="anime_weight"))
    sd = synth_sd["offsets"]
    return hp, SaberSpeechDrivenAnimation(hp).load_state_dict(sd).enable_head_training(sd, attention=attention)


def _batch(model, hp):
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    ts = _train_set(model._model._engine.out_dim)
    return ts, DSW.train_batch(ts, None, [0, 11, 47], np.random.RandomState(3), hparams=hp)


@pytest.fixture(scope="module")
def tuned(synth_sd):
    """An offsets model after one train_step + optimizer_step with attention enabled, with everything the checks need."""
    hp, model = _model(synth_sd, True)
    ts, batch = _batch(model, hp)
    before_head, before_attn = model._head_trainer.parameters(), model._attn_trainer.parameters()
    H, z_enc, align_enc = torch.ops.sdfa.encoder_memory(batch["audio_feat"].contiguous(), model._model._key)
    pred, losses, scalars = model.train_step(batch, 0)
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    grads_attn = model._attn_trainer.grads()
    model.optimizer_step()
    return dict(model=model, hp=hp, ts=ts, batch=batch, before_head=before_head, before_attn=before_attn, H=H, z_enc=z_enc,
                align_enc=align_enc, coef=coef.detach(), dcoef=coef.grad.detach().clone(), pred=pred, scalars=scalars, losses=losses,
                grads_attn=grads_attn)


def test_train_step_and_one_adam_step_within_kappa_of_the_restated_chain(tuned):
    m = tuned["model"]
    assert set(tuned["losses"]) == {"dyn_ploss", "dyn_mloss"} and tuned["scalars"]["scalar_ploss"] > 0
    assert m.training and m._head_trainer.step_count == 1 and m._attn_trainer.step_count == 1
    H = tuned["H"].cpu().numpy()
    sid = tuned["batch"]["speaker_id"].cpu().numpy()
    worst = {}

    def within(what, got, val, kap):
        d = np.abs(np.asarray(got, np.float64).reshape(val.shape) - val)
        r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
        worst[what] = max(worst.get(what, 0.0), r)
        assert (d <= kap).all(), (what, r)

    fwd = R.run(tuned["before_attn"], H)
    z_dev = tuned["pred"]["condition"].detach().reshape(-1, 512).cpu().numpy()
    within("z", z_dev, fwd["z"], fwd["k_z"])
    within("align", tuned["pred"]["align_dict"]["audio_encoder10"].reshape(-1, 64).cpu().numpy(), fwd["align"], fwd["k_align"])
    # with untouched parameters the trained layer is the inference layer: other kernels, the same function
    within("z of the inference kernels", tuned["z_enc"].cpu().numpy(), fwd["z"], fwd["k_z"])
    head = RH.run("offsets", tuned["before_head"], z_dev, sid, tuned["dcoef"].cpu().numpy())
    within("coef", tuned["coef"].cpu().numpy(), head["coef"], head["k_coef"])
    r = R.run(tuned["before_attn"], H, head["dz"], ddz=head["k_dz"])
    got = m._attn_trainer.parameters()
    for n, g in r["grads"].items():
        within("grad", tuned["grads_attn"][n], g, r["k_grads"][n])
        p1, _, _, kp, _, _ = R.adam(tuned["before_attn"][n], g, 0.0 * g, 0.0 * g, 1, eg=r["k_grads"][n])
        within("param", got[n], p1, kp)
        assert (got[n] != tuned["before_attn"][n]).mean() > 0.5, n
    got = m._head_trainer.parameters()
    for n, g in head["grads"].items():
        p1, _, _, kp, _, _ = RH.adam(tuned["before_head"][n], g, 0.0 * g, 0.0 * g, 1, eg=head["k_grads"][n])
        within("head param", got[n], p1.reshape(got[n].shape), kp.reshape(got[n].shape))
    print("\ntrain_step(attention) + optimizer_step: largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert set(m.head_state_dict()) == {"_model." + n for n in list(HT.tensor_shapes("offsets")) + list(AT.tensor_shapes())}


def test_commit_head_feeds_the_tuned_attention_to_inference(tuned):
    m = tuned["model"]
    old_engine = m._model._engine
    feat = tuned["batch"]["audio_feat"].contiguous()
    z_old, _ = torch.ops.sdfa.encoder(feat, m._model._key)
    m.commit_head()
    assert m._model._engine is not old_engine
    z_new, align_new = torch.ops.sdfa.encoder(feat, m._model._key)
    z_tr, align_tr = m._attn_trainer.forward(tuned["H"])
    r = R.run(m._attn_trainer.parameters(), tuned["H"].cpu().numpy())
    for what, got in (("engine", z_new), ("trainer", z_tr)):
        d = np.abs(got.cpu().numpy() - r["z"])
        assert (d <= r["k_z"]).all(), (what, float((d / r["k_z"]).max()))
    d = np.abs((z_new - z_tr).cpu().numpy())
    assert (d <= r["k_z"]).all()
    moved = np.abs((z_new - z_old).cpu().numpy())
    assert (moved > r["k_z"]).any()                           # the engine before the commit is the untuned layer
    print(f"\ncommit_head: engine vs trainer z {float((d / r['k_z']).max()):.4f} x kappa; the step moved z by up to {float((moved / r['k_z']).max()):.3g} x kappa")
    from sdfa_amd import synth
    ts_list, animes, _ = m.generate_animation(synth.make_pcm(3, 2 * 16000), "m0", 0, 0)
    assert len(ts_list) == animes.shape[0] > 0 and np.isfinite(animes).all()


def test_fit_head_with_attention_on_a_fixed_batch_lowers_the_loss(tuned):
    m = tuned["model"]
    hist = m.fit_head(tuned["ts"], 20, np.random.RandomState(1), fixed_batch=tuned["batch"])
    assert len(hist) == 20 and m._head_trainer.step_count == 21 and m._attn_trainer.step_count == 21
    first, last = hist[0]["scalar_ploss"], hist[-1]["scalar_ploss"]
    print(f"\nfit_head with attention, 20 steps on one batch: scalar_ploss {first:.6g} -> {last:.6g}")
    assert last < first
    m._attn_trainer.step()                                    # out of step: refused
    with pytest.raises(RuntimeError, match="step together"):
        m.optimizer_step()


def test_state_dict_resumes_bit_for_bit():
    c = R.case(3, 78, "flat")
    H, dz = torch.from_numpy(c["H"]).cuda(), torch.from_numpy(c["dz"]).cuda()

    def step(tr):
        tr.forward(H)
        tr.backward(dz, want_dH=False)
        tr.step()

    a = AT.AttnTrainer(c["params"], lr=3e-4)
    step(a)
    step(a)
    state = a.state_dict()
    b = AT.AttnTrainer(c["params"]).load_state_dict(state)
    assert b.step_count == 2 and b.lr == 3e-4
    step(a)
    step(b)
    pa, pb = a.parameters(), b.parameters()
    (ma, va), (mb, vb) = a.moments(), b.moments()
    for n in pa:
        assert (bits(pa[n]) == bits(pb[n])).all() and (bits(ma[n]) == bits(mb[n])).all() and (bits(va[n]) == bits(vb[n])).all(), n
        assert (bits(pa[n]) != bits(c["params"][n])).any()


def test_without_attention_train_step_is_the_head_trainer_driven_directly(synth_sd):
    hp, model = _model(synth_sd, False)
    assert model._attn_trainer is None
    ts, batch = _batch(model, hp)
    pred, losses, scalars = model.train_step(batch, 0)
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    z, align = torch.ops.sdfa.encoder(batch["audio_feat"].contiguous(), model._model._key)
    direct = HT.HeadTrainer(synth_sd["offsets"], "offsets")
    coef_d = direct.forward(z, batch["speaker_id"])
    direct.backward(coef.grad.detach(), want_dz=False)
    assert torch.equal(coef.detach(), coef_d)
    assert torch.equal(pred["condition"].detach().reshape(-1, 512), z) and torch.equal(pred["align_dict"]["audio_encoder10"].reshape(-1, 64), align)
    ga, gb = model._head_trainer.grads(), direct.grads()
    for n in ga:
        assert (bits(ga[n]) == bits(gb[n])).all(), n
    assert set(model.head_state_dict()) == {"_model." + n for n in HT.tensor_shapes("offsets")}
