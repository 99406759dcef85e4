"""sdfa_encoder_conv (include/sdfa_freqtrain.h, torch.ops.sdfa.encoder_conv), torch.ops.sdfa.freq_train and training the frequency
LSTM in SaberSpeechDrivenAnimation -- enable_head_training(attention=True, bilstm_top=True, bilstm_bottom=True, freq_lstm=True),
train_step, fit_head, head_state_dict, commit_head, training_state_dict / load_training_state_dict -- on the synthetic offsets
model, on the GPU.

sdfa_encoder_conv at 72 frames and at 200 frames on an engine whose workspace holds one 128-frame chunk: C [N][64][32][64] is finite
and every row is written, the operator equals the method, the option encoder_dedup_off gives the same bits (on the default path the
conv stack holds a chunk's distinct columns only and the copy goes through the share map), C is bit for bit the debug tap of X3
transposed, a FreqTrainer holding the checkpoint's weights maps C to X0 within 1 x kappa of tests/freqtrain_ref64.py on that C, the
engine's own sdfa_encoder_x0 lies within the same kappa (other kernels, the same function; the float64 model is run on the first
and the last eight frames, 1,024 columns, which keeps the test at a few seconds and reaches into the second chunk), and sdfa_encoder_x0,
sdfa_encoder_layer0 and sdfa_encoder_memory give after it the bits they gave before it.

The operator: its backward leaves the bits of the direct calls, and returns no gradient for C (a null d_dC) unless the trainer
wants dC.

One train_step(freq_lstm=True) + the summed losses' backward + optimizer_step on the three-window synthetic batch of
tests/test_gpu_lstm_train_op.py within 1 x kappa of the chain freqtrain_ref64 -> bilstm2_ref64 -> attention ref64 -> head ref64 ->
Adam, built as tests/test_gpu_bilstm_train.py builds its chain: each stage's forward on the float32 input the device gave it, each
stage's gradient and kappa fed on backwards.  commit_head() makes an engine whose X0 agrees with the trainer's within kappa while
the step moved it by many kappa.  A few fit_head steps on one batch lower scalar_ploss.  training_state_dict() taken after two steps
and loaded into a freshly enabled model continues for two more with the bits of the uninterrupted run.  The refusals by name.

Measured on an MI355X (largest |gpu - ref64| / kappa): the frequency LSTM on sdfa_encoder_conv's C 0.0057 (trainer) and 0.0058
(engine) at 72 frames, 0.0062 and 0.0059 at 200; train_step + optimizer_step 0.098 at most (a head parameter; X0 0.0070, Y0 0.0145,
H 0.0053, the BiLSTM's and the frequency LSTM's gradients and parameters below 6e-5); commit_head: engine against model 0.0052, the
step having moved X0 by 126 x kappa; fit_head: scalar_ploss 0.004753 -> 0.004258 in 10 steps.  The module takes 11 s.

This module fails to import without sdfa_amd.freqtrain and tests/freqtrain_ref64.py."""
import numpy as np
import pytest
import torch

import attntrain_ref64 as RA
import bilstm2_ref64 as B
import freqtrain_ref64 as RF
import headtrain_ref64 as RH
import lstmtrain_ref64 as R
from sdfa_amd import attntrain as AT
from sdfa_amd import freqtrain as FT        # the feature: absent before it
from sdfa_amd import headtrain as HT
from sdfa_amd import lstmtrain as LT
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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def within(worst, what, got, val, kap):
    d = np.abs(np.asarray(got, np.float64).reshape(val.shape) - val)
    assert np.isfinite(d).all(), what
    r = float((d[kap > 0] / kap[kap > 0]).max(initial=0.0))
    worst[what] = max(worst.get(what, 0.0), r)
    assert (d <= kap).all(), (what, r)


def cols(Cdev):
    """device C [N][64][32][64] -> the float64 model's [R][32][64]"""
    return Cdev.detach().cpu().numpy().reshape(-1, RF.NS, RF.NI)


# ---------------------------------------------------------------------------------------------------- sdfa_encoder_conv
@pytest.mark.parametrize("n_frames", [72, 200], ids=["one-partial-chunk", "two-chunks"])
def test_encoder_conv_is_the_input_of_the_frequency_lstm(synth_sd, n_frames):
    from sdfa_amd import _lib, ops, synth
    from sdfa_amd.engine import Engine
    assert FT.ABI_VERSION == _lib.lib.sdfa_freqtrain_abi_version()
    sd = synth_sd["offsets"]
    eng = Engine(sd, device="cuda:0", max_frames=128)        # a workspace of one 128-frame chunk: 200 frames take two
    pcm = synth.make_pcm(1, 16000 * n_frames // 60)
    feat, _, _ = eng.mel_frontend([pcm], 16000)
    feat = feat[:n_frames].contiguous()
    assert feat.shape[0] == n_frames
    X0_before = eng.encoder_x0(feat)
    X1_before = eng.encoder_layer0(feat)
    H_before, z_before, align_before = eng.encoder_memory(feat)
    Cx = eng.encoder_conv(feat)
    assert Cx.shape == (n_frames, FT.COLUMNS, FT.STEPS, FT.IN) and Cx.dtype == torch.float32 and Cx.is_contiguous()
    assert bool(torch.isfinite(Cx).all()) and float(Cx.abs().mean()) > 1e-4
    assert (Cx.abs().amax(dim=(2, 3)) > 0).all()             # every row (n, t) was written, the second chunk's too
    key = ops.register_model(None, eng)
    assert torch.equal(torch.ops.sdfa.encoder_conv(feat, key), Cx)
    fake = torch.library.opcheck(torch.ops.sdfa.encoder_conv.default, (feat, key), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake
    # the every-column path gives the same bits: on the default path the copy went through the share map
    last = n_frames - (n_frames - 1) // 128 * 128            # frames of the last chunk
    distinct = eng.distinct_columns(last)
    assert 0 < distinct < 64 * last, (distinct, last)         # X3 did hold fewer columns than the chunk has
    _lib.set_option("encoder_dedup_off", 1)
    try:
        C_off = eng.encoder_conv(feat)
    finally:
        _lib.set_option("encoder_dedup_off", 0)
    assert torch.equal(C_off, Cx)
    # the debug tap of X3 is the reference's (n, 64 ch, 32 f, 64 t): C is its transpose, bit for bit
    dbg = Engine(sd, device="cuda:0", max_frames=128, debug_keep=True)
    for f0 in range(0, n_frames, 128):
        part = feat[f0:f0 + 128].contiguous()
        dbg.encoder(part)
        X3 = dbg.tap(1, part.shape[0])
        assert torch.equal(X3.permute(0, 3, 2, 1).contiguous(), Cx[f0:f0 + 128])
    # the frequency LSTM with the checkpoint's weights, the training kernels and the inference kernels, on this C
    tr = FT.FreqTrainer(sd)
    rows = list(range(8)) + list(range(n_frames - 8, n_frames))      # the float64 model on the first and the last 8 frames (the last chunk's)
    X0 = tr.forward(Cx)
    r = RF.run(tr.parameters(), cols(Cx[rows]))
    worst = {}
    within(worst, "trainer's X0", X0[rows].cpu().numpy(), r["X0"], r["k_X0"])
    within(worst, "engine's X0", X0_before[rows].cpu().numpy(), r["X0"], r["k_X0"])
    assert bool(torch.isfinite(X0).all())
    print(f"\n{n_frames} frames: the frequency LSTM on sdfa_encoder_conv's C, largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    # the other entry points launch what they launched: the same bits after the conv exit used the workspace
    assert torch.equal(eng.encoder_x0(feat), X0_before)
    assert torch.equal(eng.encoder_layer0(feat), X1_before)
    H_after, z_after, align_after = eng.encoder_memory(feat)
    assert torch.equal(H_after, H_before) and torch.equal(z_after, z_before) and torch.equal(align_after, align_before)
    # the refusals of sdfa_encoder_x0, with real buffers
    ws = eng.workspace(n_frames)
    cp, fp, wp = Cx.data_ptr(), feat.data_ptr(), ws.data_ptr()
    call = _lib.lib.sdfa_encoder_conv
    assert call(eng._m, fp, n_frames, None, wp, ws.numel(), None) == _lib.EINVAL
    assert call(eng._m, fp, n_frames, cp + 4, wp, ws.numel(), None) == _lib.EINVAL and b"16-byte aligned" in _lib.lib.sdfa_last_error()
    assert call(eng._m, None, n_frames, cp, wp, ws.numel(), None) == _lib.EINVAL
    assert call(eng._m, fp, -1, cp, wp, ws.numel(), None) == _lib.EINVAL
    assert call(eng._m, fp, n_frames, cp, wp, 4096, None) == _lib.ENOSPACE
    assert call(eng._m, fp, 0, cp, wp, ws.numel(), None) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(eng.encoder_conv(feat), Cx)


# ---------------------------------------------------------------------------------------------------- the operator
def test_operator_backward_is_the_direct_calls():
    from sdfa_amd import ops  # noqa: F401  (registers torch.ops.sdfa.freq_train)
    N = 2
    c = RF.case(RF.COLS * N, 77, "carry")
    C4, dX3 = dev(c["C"].reshape(N, RF.COLS, RF.NS, RF.NI)), dev(c["dX0"].reshape(N, RF.COLS, RF.NO))
    direct = FT.FreqTrainer(c["params"])
    X0d = direct.forward(C4)
    dCd = direct.backward(dX3, want_dC=True)
    for want in (False, True):
        tr = FT.FreqTrainer(c["params"], want_dC=want)
        Cr = C4.clone().requires_grad_(True)
        X0 = torch.ops.sdfa.freq_train(Cr, FT.register_trainer(tr))
        assert torch.equal(X0.detach(), X0d)
        (X0 * dX3).sum().backward()
        assert (Cr.grad is None) if not want else torch.equal(Cr.grad, dCd)       # a null d_dC unless the trainer wants dC
        ga, gb = tr.grads(), direct.grads()
        for n in ga:
            assert (bits(ga[n]) == bits(gb[n])).all(), n
    fake = torch.library.opcheck(torch.ops.sdfa.freq_train.default, (C4, FT.register_trainer(direct)), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake
    with pytest.raises(KeyError, match="no frequency LSTM trainer registered"):
        FT.trainer_of("sdfa-freq-trainer-none")


# ---------------------------------------------------------------------------------------------------- the model
FLAGS = dict(attention=True, bilstm_top=True, bilstm_bottom=True, freq_lstm=True)


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


def _trainers(model):
    return dict(head=model._head_trainer, attn=model._attn_trainer, lstm=model._lstm_trainer, lstm0=model._lstm0_trainer, freq=model._freq_trainer)


def test_refusals_by_name(synth_sd):
    msg = "head training: freq_lstm=True needs bilstm_bottom=True: the frequency LSTM is trained through the bottom layer's dX"
    with pytest.raises(NotImplementedError, match=msg):
        _model(synth_sd, attention=True, bilstm_top=True, freq_lstm=True)
    with pytest.raises(NotImplementedError, match=msg):
        _model(synth_sd, freq_lstm=True)
    hp, with_freq = _model(synth_sd, **FLAGS)
    state = with_freq.training_state_dict()
    assert state["flags"] == dict(FLAGS, bilstm_dropout=0.0)
    assert set(state["trainers"]) == {"head", "attention", "bilstm_top", "bilstm_bottom", "freq_lstm"}
    hp, without = _model(synth_sd, attention=True, bilstm_top=True, bilstm_bottom=True)
    assert without._freq_trainer is None and not without._lstm0_trainer.want_dX and with_freq._lstm0_trainer.want_dX
    assert "freq_lstm" not in without.training_state_dict()["flags"]          # the flags of a model without it are what they were
    with pytest.raises(ValueError, match=r"training state: taken with freq_lstm=True \(this model: freq_lstm=False\)"):
        without.load_training_state_dict(state)
    with pytest.raises(ValueError, match=r"taken with freq_lstm=False \(this model: freq_lstm=True\)"):
        with_freq.load_training_state_dict(without.training_state_dict())


@pytest.fixture(scope="module")
def tuned(synth_sd):
    """An offsets model after one train_step + optimizer_step with the frequency LSTM enabled, with everything the checks need."""
    hp, model = _model(synth_sd, **FLAGS)
    assert model._lstm0_trainer.want_dX and not model._freq_trainer.want_dC
    ts, batch = _batch(model, hp)
    before = {k: t.parameters() for k, t in _trainers(model).items()}
    feat = batch["audio_feat"].contiguous()
    C_enc = torch.ops.sdfa.encoder_conv(feat, model._model._key)
    X0_enc = torch.ops.sdfa.encoder_x0(feat, model._model._key)
    pred, losses, scalars = model.train_step(batch, 0)
    assert torch.equal(model._freq_trainer._C, C_enc)
    X0_tr = model._lstm0_trainer._X.detach().clone()
    Y0_tr = model._lstm0_trainer._Y.detach().clone()
    H_tr = model._lstm_trainer._Y.detach().clone()
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    grads = {k: t.grads() for k, t in _trainers(model).items() if k != "head"}
    model.optimizer_step()
    return dict(model=model, hp=hp, ts=ts, batch=batch, before=before, C=C_enc, X0_enc=X0_enc, X0_tr=X0_tr, Y0_tr=Y0_tr, H_tr=H_tr,
                coef=coef.detach(), dcoef=coef.grad.detach().clone(), pred=pred, scalars=scalars, losses=losses, grads=grads)


def test_train_step_and_one_adam_step_within_kappa_of_the_restated_chain(tuned):
    m = tuned["model"]
    assert set(tuned["losses"]) == {"dyn_ploss", "dyn_mloss"} and tuned["scalars"]["scalar_ploss"] > 0
    assert m.training and [t.step_count for t in _trainers(m).values()] == [1, 1, 1, 1, 1]
    Cn = cols(tuned["C"])
    X0 = tuned["X0_tr"].cpu().numpy()
    ones = np.ones(X0.shape[:2] + (R.NY,), np.float32)
    sid = tuned["batch"]["speaker_id"].cpu().numpy()
    both = {**tuned["before"]["lstm0"], **tuned["before"]["lstm"]}
    worst = {}
    ff = RF.run(tuned["before"]["freq"], Cn)
    within(worst, "X0", X0, ff["X0"], ff["k_X0"])
    within(worst, "X0 of the inference kernels", tuned["X0_enc"].cpu().numpy(), ff["X0"], ff["k_X0"])
    # each later stage's forward is judged on the float32 input the device gave it, as tests/test_gpu_bilstm_train.py does
    lf = B.run(both, X0, ones)
    within(worst, "Y0", tuned["Y0_tr"].cpu().numpy(), lf["Y0"], lf["k_Y0"])
    within(worst, "H", tuned["H_tr"].cpu().numpy(), lf["H"], lf["k_H"])
    H_dev = tuned["H_tr"].cpu().numpy()
    af = RA.run(tuned["before"]["attn"], H_dev)
    z_dev = tuned["pred"]["condition"].detach().reshape(-1, 512).cpu().numpy()
    within(worst, "z", z_dev, af["z"], af["k_z"])
    head = RH.run("offsets", tuned["before"]["head"], z_dev, sid, tuned["dcoef"].cpu().numpy())
    within(worst, "coef", tuned["coef"].cpu().numpy(), head["coef"], head["k_coef"])
    ab = RA.run(tuned["before"]["attn"], H_dev, head["dz"], ddz=head["k_dz"])
    for n, g in ab["grads"].items():
        within(worst, "attention grad", tuned["grads"]["attn"][n], g, ab["k_grads"][n])
    lb = B.run(both, X0, ones, ab["dH"], kdH=ab["k_dH"])
    for kind, layer in (("lstm0", 0), ("lstm", 1)):
        got = _trainers(m)[kind].parameters()
        for n in R.names(layer):
            g = lb["grads"][n]
            within(worst, f"BiLSTM l{layer} grad", tuned["grads"][kind][n], g, lb["k_grads"][n])
            p1, _, _, kp, _, _ = R.adam(tuned["before"][kind][n], g, 0.0 * g, 0.0 * g, 1, eg=lb["k_grads"][n])
            within(worst, f"BiLSTM l{layer} param", got[n], p1, kp)
            assert (got[n] != tuned["before"][kind][n]).mean() > 0.5, n
    # layer 0's dX0, which bilstm2_ref64 does not form, then the frequency LSTM's backward on it
    l0 = R.run(0, tuned["before"]["lstm0"], X0, lb["dY0"], kdY=lb["k_dY0"], want_dX=True)
    fb = RF.run(tuned["before"]["freq"], Cn, l0["dX"].reshape(-1, RF.NO), kdX0=l0["k_dX"].reshape(-1, RF.NO), want_dC=False)
    got = m._freq_trainer.parameters()
    assert set(got) == set(RF.names()) == set(fb["grads"])
    for n in RF.names():
        g = fb["grads"][n]
        kind = n.rsplit(".6.", 1)[1].split(".")[0]
        within(worst, f"frequency {kind} grad", tuned["grads"]["freq"][n], g, fb["k_grads"][n])
        assert np.abs(g).max() > 0
        p1, _, _, kp, _, _ = RF.adam(tuned["before"]["freq"][n], g, 0.0 * g, 0.0 * g, 1, eg=fb["k_grads"][n])
        within(worst, f"frequency {kind} param", got[n], p1, kp)
        assert (got[n] != tuned["before"]["freq"][n]).mean() > 0.5, n          # every tensor of the module has moved
    got = m._attn_trainer.parameters()
    for n, g in ab["grads"].items():
        p1, _, _, kp, _, _ = RA.adam(tuned["before"]["attn"][n], g, 0.0 * g, 0.0 * g, 1, eg=ab["k_grads"][n])
        within(worst, "attention param", got[n], p1, kp)
        assert (got[n] != tuned["before"]["attn"][n]).any(), n
    got = m._head_trainer.parameters()
    for n, g in head["grads"].items():
        p1, _, _, kp, _, _ = RH.adam(tuned["before"]["head"][n], g, 0.0 * g, 0.0 * g, 1, eg=head["k_grads"][n])
        within(worst, "head param", got[n], p1.reshape(got[n].shape), kp.reshape(got[n].shape))
        assert (got[n] != tuned["before"]["head"][n]).any(), n
    print("\ntrain_step(freq_lstm) + optimizer_step: largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert set(m.head_state_dict()) == {"_model." + n for n in list(HT.tensor_shapes("offsets")) + list(AT.tensor_shapes()) + list(LT.tensor_shapes(1))
                                        + list(LT.tensor_shapes(0)) + list(FT.tensor_shapes())}


def test_commit_head_feeds_the_tuned_frequency_lstm_to_inference(tuned):
    m = tuned["model"]
    old_engine = m._model._engine
    feat = tuned["batch"]["audio_feat"].contiguous()
    m.commit_head()
    assert m._model._engine is not old_engine
    assert torch.equal(torch.ops.sdfa.encoder_conv(feat, m._model._key), tuned["C"])          # the conv stack is frozen
    X0_new = torch.ops.sdfa.encoder_x0(feat, m._model._key)
    X0_tr = m._freq_trainer.forward(tuned["C"])
    r = RF.run(m._freq_trainer.parameters(), cols(tuned["C"]))
    worst = {}
    within(worst, "engine's X0", X0_new.cpu().numpy(), r["X0"], r["k_X0"])
    within(worst, "trainer's X0", X0_tr.cpu().numpy(), r["X0"], r["k_X0"])
    kap = r["k_X0"].reshape(X0_new.shape)
    assert (np.abs((X0_new - X0_tr).cpu().numpy()) <= kap).all()
    moved = np.abs((X0_new - tuned["X0_enc"]).cpu().numpy())
    assert (moved > 10 * kap).any()                          # the engine before the commit holds the untuned module
    worst["moved X0"] = float((moved / kap).max())
    print("\ncommit_head with the frequency LSTM: |gpu - ref64| / kappa and what the step moved: " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items()))
    from sdfa_amd import synth
    ts_list, animes, _ = m.generate_animation(synth.make_pcm(3, 2 * 16000), "m0", 0, 0)
    assert len(ts_list) == animes.shape[0] > 0 and np.isfinite(animes).all()


def test_fit_head_with_the_frequency_lstm_on_a_fixed_batch_lowers_the_loss(tuned):
    m = tuned["model"]
    hist = m.fit_head(tuned["ts"], 10, np.random.RandomState(1), fixed_batch=tuned["batch"])
    assert len(hist) == 10 and [t.step_count for t in _trainers(m).values()] == [11] * 5
    first, last = hist[0]["scalar_ploss"], hist[-1]["scalar_ploss"]
    print(f"\nfit_head with the frequency LSTM, 10 steps on one batch: scalar_ploss {first:.6g} -> {last:.6g}")
    assert last < first
    m._freq_trainer.step()                                    # out of step: refused
    with pytest.raises(RuntimeError, match="frequency-LSTM trainer at step 12"):
        m.optimizer_step()


def _snapshot(model):
    out = {}
    for kind, tr in _trainers(model).items():
        mm, v = tr.moments()
        out[kind] = (tr.parameters(), mm, v, tr.step_count)
    out["scalers"] = {k: sc.state_dict() for k, sc in model._loss_scalers.items()}
    return out


def test_training_state_dict_resumes_bit_for_bit(synth_sd):
    hp, a = _model(synth_sd, **FLAGS)
    ts, batch = _batch(a, hp)
    rng = np.random.RandomState(1)
    a.fit_head(ts, 2, rng, fixed_batch=batch)
    state = a.training_state_dict()
    assert set(state["scalers"]) == {"dyn_p", "dyn_m"} and state["trainers"]["freq_lstm"]["step"] == 2 and state["flags"]["freq_lstm"] is True
    at_two = _snapshot(a)
    hist_a = a.fit_head(ts, 2, rng, fixed_batch=batch)
    hp_b, b = _model(synth_sd, **FLAGS)
    assert b.load_training_state_dict(state) is b
    back = _snapshot(b)
    for kind in _trainers(b):
        for x, y in zip(at_two[kind][:3], back[kind][:3]):
            for n in x:
                assert (bits(x[n]) == bits(y[n])).all(), (kind, n)
        assert back[kind][3] == 2
    assert back["scalers"] == at_two["scalers"]
    hist_b = b.fit_head(ts, 2, rng, fixed_batch=batch)
    assert hist_a == hist_b
    end_a, end_b = _snapshot(a), _snapshot(b)
    for kind in _trainers(a):
        for x, y, start in zip(end_a[kind][:3], end_b[kind][:3], at_two[kind][:3]):
            for n in x:
                assert (bits(x[n]) == bits(y[n])).all(), (kind, n)
                assert (bits(x[n]) != bits(start[n])).any(), (kind, n)
        assert end_a[kind][3] == end_b[kind][3] == 4
    assert end_a["scalers"] == end_b["scalers"] and end_a["scalers"] != at_two["scalers"]
