"""torch.ops.sdfa.lstm_train / encoder_layer0 (sdfa_amd/ops.py) and training the BiLSTM's top layer in SaberSpeechDrivenAnimation
-- enable_head_training(attention=True, bilstm_top=True), train_step, fit_head, head_state_dict, commit_head -- on the synthetic
offsets model, on the GPU.

sdfa_encoder_layer0: an LstmTrainer(layer=1) holding the checkpoint's weights maps its X1 to sdfa_encoder_memory's H within kappa
(other kernels, the same function), at 72 frames and at 200 frames on an engine whose workspace holds one 128-frame chunk; X1 has
the same bits with the option encoder_dedup_off.

One train_step + get_loss + optimizer_step on the two-clip synthetic TrainSet of tests/test_gpu_train_losses.py lies within
1 x kappa of the restated chain.  Forward, each stage on the float32 input the device gave it: the BiLSTM model
(tests/lstmtrain_ref64.py) on the device's X1 gives H; the attention model (tests/attntrain_ref64.py) on the device's H gives z;
the head model (tests/headtrain_ref64.py) on the device's z gives the coefficients.  Backward, each stage's gradient and kappa
fed on: the head model on the objective's d loss / d coef gives dz with its kappa; the attention model's backward takes that dz
and its kappa and gives its gradients and dH with its kappa; the BiLSTM model's backward takes that dH and its kappa and gives
the layer's gradients; Adam gives the parameters.  (d loss / d coef is the device's, as in tests/test_gpu_head_train_op.py: the
objective has its own float64 check in tests/test_gpu_train_losses.py.)  commit_head() then makes an inference engine whose H
agrees with the trainer's forward within kappa, while the step moved H by many kappa.  Twenty steps of fit_head on a fixed batch lower scalar_ploss.  A trainer
restored from state_dict() continues bit for bit.  With bilstm_dropout = 0.1 and a seeded generator the step equals one fed the
explicitly masked X1, bit for bit.  With bilstm_top=False train_step gives the bits of attention + head training.

Measured on an MI355X: layer 1 on sdfa_encoder_layer0's X1 against the encoder's H 0.0145 x kappa (72 frames) and 0.0115 (200);
train_step + optimizer_step 0.098 x kappa at most (a head parameter; H 0.0101, an attention gradient 0.0010, the BiLSTM gradients
below 5e-5 of a kappa that carries the attention layer's whole k_dH linearly over the 192 rows); commit_head: engine against trainer
0.004 x kappa, the step having moved H by 446 x kappa; fit_head: scalar_ploss 0.00506 -> 0.00421.  The module takes 8 s.

This module fails to import without sdfa_amd.lstmtrain."""
import numpy as np
import pytest
import torch

import attntrain_ref64 as RA
import headtrain_ref64 as RH
import lstmtrain_ref64 as R
from sdfa_amd import attntrain as AT
from sdfa_amd import headtrain as HT
from sdfa_amd import lstmtrain as LT          # the feature: absent before it
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


def within(worst, what, got, val, kap):
    d = np.abs(np.asarray(got, np.float64).reshape(val.shape) - val)
    assert np.isfinite(d).all(), what
    r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
    worst[what] = max(worst.get(what, 0.0), r)
    assert (d <= kap).all(), (what, r)


# ---------------------------------------------------------------------------------------------------- sdfa_encoder_layer0
@pytest.mark.parametrize("n_frames", [72, 200], ids=["one-chunk", "across-chunks"])
def test_encoder_layer0_feeds_layer1_to_the_encoders_memory(synth_sd, n_frames):
    from sdfa_amd import _lib, ops, synth
    from sdfa_amd.engine import Engine
    sd = synth_sd["offsets"]
    eng = Engine(sd, device="cuda:0", max_frames=128)        # a workspace of one 128-frame chunk: 200 frames take two
    pcm = synth.make_pcm(1, 16000 * n_frames // 60)
    feat, _, _ = eng.mel_frontend([pcm], 16000)
    feat = feat[:n_frames].contiguous()
    assert feat.shape[0] == n_frames
    H, _, _ = eng.encoder_memory(feat, want_z=False, want_align=False)
    X1 = eng.encoder_layer0(feat)
    assert X1.shape == (n_frames, 64, 512) and float(X1.abs().max()) <= 1.0 and float(X1.abs().mean()) > 1e-3
    assert torch.equal(torch.ops.sdfa.encoder_layer0(feat, ops.register_model(None, eng)), X1)
    tr = LT.LstmTrainer(sd, layer=1)
    Y = tr.forward(X1)
    r = R.run(1, tr.parameters(), X1.cpu().numpy())
    worst = {}
    within(worst, "trainer's H", Y.cpu().numpy(), r["Y"], r["k_Y"])
    within(worst, "engine's H", H.cpu().numpy(), r["Y"], r["k_Y"])
    print(f"\n{n_frames} frames: layer 1 on sdfa_encoder_layer0's X1, largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    # the every-column path gives the same bits
    _lib.set_option("encoder_dedup_off", 1)
    try:
        X1_off = eng.encoder_layer0(feat)
    finally:
        _lib.set_option("encoder_dedup_off", 0)
    assert torch.equal(X1_off, X1)
    assert tr.lstm_state_dict().keys() == {"_model." + n for n in LT.tensor_shapes(1)}


# ---------------------------------------------------------------------------------------------------- the model
def _model(synth_sd, **kw):
    from speech_anime import hparams as Hp
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    hp = Hp.configure({"custom_hparams": "offsets"})
    hp.audio.set_key("sample_rate", 16000)
    hp.set_key("loss", dict(ploss_scale=1, mloss_scale=1, dynamic_scalar=True, anime_loss_weight="anime_weight"))
    sd = synth_sd["offsets"]
    return hp, SaberSpeechDrivenAnimation(hp).load_state_dict(sd).enable_head_training(sd, **kw)


def _batch(model, hp):
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    ts = _train_set(model._model._engine.out_dim)
    return ts, DSW.train_batch(ts, None, [0, 11, 47], np.random.RandomState(3), hparams=hp)


def test_enabling_refusals(synth_sd):
    with pytest.raises(NotImplementedError, match="bilstm_top=True needs attention=True"):
        _model(synth_sd, bilstm_top=True)
    with pytest.raises(NotImplementedError, match="bilstm_dropout needs bilstm_top=True"):
        _model(synth_sd, attention=True, bilstm_dropout=0.1)
    with pytest.raises(ValueError, match="bilstm_dropout"):
        _model(synth_sd, attention=True, bilstm_top=True, bilstm_dropout=1.0)


@pytest.fixture(scope="module")
def tuned(synth_sd):
    """An offsets model after one train_step + optimizer_step with the BiLSTM's top layer enabled, with everything the checks need."""
    hp, model = _model(synth_sd, attention=True, bilstm_top=True)
    assert model._attn_trainer.want_dH and not model._lstm_trainer.want_dX and model._lstm_trainer.layer == 1
    ts, batch = _batch(model, hp)
    before = dict(head=model._head_trainer.parameters(), attn=model._attn_trainer.parameters(), lstm=model._lstm_trainer.parameters())
    feat = batch["audio_feat"].contiguous()
    X1 = torch.ops.sdfa.encoder_layer0(feat, model._model._key)
    H_enc, _, _ = torch.ops.sdfa.encoder_memory(feat, model._model._key)
    pred, losses, scalars = model.train_step(batch, 0)
    H_tr = model._lstm_trainer._Y.detach().clone()
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    grads = dict(attn=model._attn_trainer.grads(), lstm=model._lstm_trainer.grads())
    model.optimizer_step()
    return dict(model=model, hp=hp, ts=ts, batch=batch, before=before, X1=X1, H_enc=H_enc, H_tr=H_tr, coef=coef.detach(),
                dcoef=coef.grad.detach().clone(), pred=pred, scalars=scalars, losses=losses, grads=grads)


def test_train_step_and_one_adam_step_within_kappa_of_the_restated_chain(tuned):
    m = tuned["model"]
    assert set(tuned["losses"]) == {"dyn_ploss", "dyn_mloss"} and tuned["scalars"]["scalar_ploss"] > 0
    assert m.training and m._head_trainer.step_count == m._attn_trainer.step_count == m._lstm_trainer.step_count == 1
    X1 = tuned["X1"].cpu().numpy()
    sid = tuned["batch"]["speaker_id"].cpu().numpy()
    worst = {}
    lf = R.run(1, tuned["before"]["lstm"], X1)
    within(worst, "H", tuned["H_tr"].cpu().numpy(), lf["Y"], lf["k_Y"])
    # with untouched parameters the trained layer is the inference layer: other kernels, the same function
    within(worst, "H of the inference kernels", tuned["H_enc"].cpu().numpy(), lf["Y"], lf["k_Y"])
    # each later stage's forward is judged on the float32 input the device gave it, as tests/test_gpu_attn_train_op.py does
    H_dev = tuned["H_tr"].cpu().numpy()
    af = RA.run(tuned["before"]["attn"], H_dev)
    z_dev = tuned["pred"]["condition"].detach().reshape(-1, 512).cpu().numpy()
    within(worst, "z", z_dev, af["z"], af["k_z"])
    head = RH.run("offsets", tuned["before"]["head"], z_dev, sid, tuned["dcoef"].cpu().numpy())
    within(worst, "coef", tuned["coef"].cpu().numpy(), head["coef"], head["k_coef"])
    # the attention backward on the device's H (an exact float32 input of the device's attention layer), dz and its kappa fed on
    ab = RA.run(tuned["before"]["attn"], H_dev, head["dz"], ddz=head["k_dz"])
    for n, g in ab["grads"].items():
        within(worst, "attention grad", tuned["grads"]["attn"][n], g, ab["k_grads"][n])
    lb = R.run(1, tuned["before"]["lstm"], X1, ab["dH"], kdY=ab["k_dH"], want_dX=False)
    got = m._lstm_trainer.parameters()
    for n, g in lb["grads"].items():
        within(worst, "BiLSTM grad", tuned["grads"]["lstm"][n], g, lb["k_grads"][n])
        assert np.abs(g).max() > 0
        p1, _, _, kp, _, _ = R.adam(tuned["before"]["lstm"][n], g, 0.0 * g, 0.0 * g, 1, eg=lb["k_grads"][n])
        within(worst, "BiLSTM param", got[n], p1, kp)
        assert (got[n] != tuned["before"]["lstm"][n]).mean() > 0.5, n
    got = m._attn_trainer.parameters()
    for n, g in ab["grads"].items():
        p1, _, _, kp, _, _ = RA.adam(tuned["before"]["attn"][n], g, 0.0 * g, 0.0 * g, 1, eg=ab["k_grads"][n])
        within(worst, "attention param", got[n], p1, kp)
    got = m._head_trainer.parameters()
    for n, g in head["grads"].items():
        p1, _, _, kp, _, _ = RH.adam(tuned["before"]["head"][n], g, 0.0 * g, 0.0 * g, 1, eg=head["k_grads"][n])
        within(worst, "head param", got[n], p1.reshape(got[n].shape), kp.reshape(got[n].shape))
    print("\ntrain_step(bilstm_top) + optimizer_step: largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert set(m.head_state_dict()) == {"_model." + n for n in list(HT.tensor_shapes("offsets")) + list(AT.tensor_shapes()) + list(LT.tensor_shapes(1))}


def test_commit_head_feeds_the_tuned_layer_to_inference(tuned):
    m = tuned["model"]
    old_engine = m._model._engine
    feat = tuned["batch"]["audio_feat"].contiguous()
    m.commit_head()
    assert m._model._engine is not old_engine
    H_new, _, _ = torch.ops.sdfa.encoder_memory(feat, m._model._key)
    assert torch.equal(torch.ops.sdfa.encoder_layer0(feat, m._model._key), tuned["X1"])      # layer 0 is frozen
    H_tr = m._lstm_trainer.forward(tuned["X1"])
    r = R.run(1, m._lstm_trainer.parameters(), tuned["X1"].cpu().numpy())
    for what, got in (("engine", H_new), ("trainer", H_tr)):
        d = np.abs(got.cpu().numpy() - r["Y"])
        assert (d <= r["k_Y"]).all(), (what, float((d / r["k_Y"]).max()))
    d = np.abs((H_new - H_tr).cpu().numpy())
    assert (d <= r["k_Y"]).all()
    moved = np.abs((H_new - tuned["H_enc"]).cpu().numpy())
    assert (moved > 10 * r["k_Y"]).any()                      # the engine before the commit is the untuned layer
    print(f"\ncommit_head: engine vs trainer H {float((d / r['k_Y']).max()):.4f} x kappa; the step moved H by up to {float((moved / r['k_Y']).max()):.3g} x kappa")
    from sdfa_amd import synth
    ts_list, animes, _ = m.generate_animation(synth.make_pcm(3, 2 * 16000), "m0", 0, 0)
    assert len(ts_list) == animes.shape[0] > 0 and np.isfinite(animes).all()


def test_fit_head_with_the_top_layer_on_a_fixed_batch_lowers_the_loss(tuned):
    m = tuned["model"]
    hist = m.fit_head(tuned["ts"], 20, np.random.RandomState(1), fixed_batch=tuned["batch"])
    assert len(hist) == 20 and m._head_trainer.step_count == m._attn_trainer.step_count == m._lstm_trainer.step_count == 21
    first, last = hist[0]["scalar_ploss"], hist[-1]["scalar_ploss"]
    print(f"\nfit_head with the BiLSTM's top layer, 20 steps on one batch: scalar_ploss {first:.6g} -> {last:.6g}")
    assert last < first
    m._lstm_trainer.step()                                    # out of step: refused
    with pytest.raises(RuntimeError, match="BiLSTM trainer at step 22"):
        m.optimizer_step()


def test_state_dict_resumes_bit_for_bit():
    c = R.case(1, 3, 78, "carry")
    X, dY = torch.from_numpy(c["X"]).cuda(), torch.from_numpy(c["dY"]).cuda()

    def step(tr):
        tr.forward(X)
        tr.backward(dY, want_dX=False)
        tr.step()

    a = LT.LstmTrainer(c["params"], layer=1, lr=3e-4)
    step(a)
    step(a)
    state = a.state_dict()
    b = LT.LstmTrainer(c["params"], layer=1).load_state_dict(state)
    assert b.step_count == 2 and b.lr == 3e-4
    step(a)
    step(b)
    pa, pb = a.parameters(), b.parameters()
    (ma, va), (mb, vb) = a.moments(), b.moments()
    for n in pa:
        assert (bits(pa[n]) == bits(pb[n])).all() and (bits(ma[n]) == bits(mb[n])).all() and (bits(va[n]) == bits(vb[n])).all(), n
        assert (bits(pa[n]) != bits(c["params"][n])).any()
    with pytest.raises(AssertionError):
        LT.LstmTrainer(R.case(0, 1, 1)["params"], layer=0).load_state_dict(state)     # another layer's state
    fake = torch.library.opcheck(torch.ops.sdfa.lstm_train.default, (X, LT.register_trainer(a)), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake
    with pytest.raises(KeyError):
        torch.ops.sdfa.lstm_train(X, "no such trainer")


def _one_step(model, batch):
    pred, losses, _ = model.train_step(batch, 0)
    sum(losses.values()).backward()
    return pred, dict(head=model._head_trainer.grads(), attn=model._attn_trainer.grads(),
                      lstm=model._lstm_trainer.grads() if model._lstm_trainer is not None else {})


def test_dropout_with_a_seeded_generator_is_the_explicitly_masked_step(synth_sd):
    p = 0.1
    hp, model = _model(synth_sd, attention=True, bilstm_top=True, bilstm_dropout=p)
    ts, batch = _batch(model, hp)
    model._train_generator = torch.Generator(device="cuda").manual_seed(1234)
    pred, grads = _one_step(model, batch)
    # the same draw, applied by hand, through the trainers driven directly
    X1 = torch.ops.sdfa.encoder_layer0(batch["audio_feat"].contiguous(), model._model._key)
    keep = torch.empty_like(X1).bernoulli_(1.0 - p, generator=torch.Generator(device="cuda").manual_seed(1234))
    assert 0.85 < float(keep.mean()) < 0.95
    masked = X1 * (keep / (1.0 - p))
    assert torch.equal(model._lstm_trainer._X, masked)
    hp2, plain = _model(synth_sd, attention=True, bilstm_top=True)
    H = plain._lstm_trainer.forward(masked)
    z, align = plain._attn_trainer.forward(H)
    assert torch.equal(z, pred["condition"].detach().reshape(-1, 512)) and torch.equal(align, pred["align_dict"]["audio_encoder10"].reshape(-1, 64))
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef_d = plain._head_trainer.forward(z, batch["speaker_id"])
    assert torch.equal(coef_d, coef.detach())
    # the gradients: the same objective on the same coefficients, so the unmasked model's step on `masked` has the same bits
    Xr = masked.clone().requires_grad_(True)
    zz, _ = torch.ops.sdfa.attn_train(torch.ops.sdfa.lstm_train(Xr, plain._lstm_trainer_key), plain._attn_trainer_key)
    cc = torch.ops.sdfa.head_train(zz, batch["speaker_id"], plain._head_trainer_key)
    name = "verts_off_3d_coef"
    plain.train()                                             # as train_step does: the dynamic loss scalers update in training mode
    losses, _ = plain.get_loss(dict(prediction={name: cc}, condition=zz.view(-1, 1, 512), align_dict={}, latent_dict={}), batch)
    sum(losses.values()).backward()
    for kind, tr in (("head", plain._head_trainer), ("attn", plain._attn_trainer), ("lstm", plain._lstm_trainer)):
        g = tr.grads()
        for n in g:
            assert (bits(g[n]) == bits(grads[kind][n])).all(), (kind, n)
    # another seed draws another mask; p = 0 draws none
    model._train_generator.manual_seed(99)
    model.train_step(batch, 1)
    assert not torch.equal(model._lstm_trainer._X, masked)
    plain.train_step(batch, 0)
    assert torch.equal(plain._lstm_trainer._X, X1) and getattr(plain, "_train_generator", None) is None


def test_without_bilstm_top_train_step_is_attention_plus_head(synth_sd):
    hp, model = _model(synth_sd, attention=True)
    assert model._lstm_trainer is None and not model._attn_trainer.want_dH
    ts, batch = _batch(model, hp)
    pred, losses, scalars = model.train_step(batch, 0)
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    H, _, _ = torch.ops.sdfa.encoder_memory(batch["audio_feat"].contiguous(), model._model._key)
    at = AT.AttnTrainer(synth_sd["offsets"], want_dH=False)
    z, align = at.forward(H)
    direct = HT.HeadTrainer(synth_sd["offsets"], "offsets")
    coef_d = direct.forward(z, batch["speaker_id"])
    at.backward(direct.backward(coef.grad.detach(), want_dz=True), want_dH=False)
    assert torch.equal(coef.detach(), coef_d)
    assert torch.equal(pred["condition"].detach().reshape(-1, 512), z) and torch.equal(pred["align_dict"]["audio_encoder10"].reshape(-1, 64), align)
    for a, b in ((model._head_trainer, direct), (model._attn_trainer, at)):
        ga, gb = a.grads(), b.grads()
        for n in ga:
            assert (bits(ga[n]) == bits(gb[n])).all(), n
    assert set(model.head_state_dict()) == {"_model." + n for n in list(HT.tensor_shapes("offsets")) + list(AT.tensor_shapes())}
    model.optimizer_step()
    assert model._head_trainer.step_count == model._attn_trainer.step_count == 1
