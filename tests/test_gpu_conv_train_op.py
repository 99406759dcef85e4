"""torch.ops.sdfa.conv_train and training the conv stack in SaberSpeechDrivenAnimation -- enable_head_training(attention=True,
bilstm_top=True, bilstm_bottom=True, freq_lstm=True, conv_stack=True), train_step, fit_head, head_state_dict, commit_head,
training_state_dict / load_training_state_dict -- on the synthetic offsets model, on the GPU.

A ConvTrainer holding the checkpoint's tensors maps features to C within 1 x kappa of tests/convtrain_ref64.py, and the engine's
sdfa_encoder_conv lies within the same kappa (other kernels and a fold on the host, the same function: bitwise equality is not
asked).  The operator equals the method; its backward leaves the bits of the direct calls and returns no gradient for the features.

One train_step(conv_stack=True) + the summed losses' backward + optimizer_step on the three-window synthetic batch of
tests/test_gpu_freq_train_op.py: the chain of that file (head -> attention -> both BiLSTM layers -> frequency LSTM, now with dC)
restated in float64 and carried on into convtrain_ref64 with k_dC; the conv gradients and parameters lie within 1 x kappa, every
tensor of all six trainers has moved and the six step counts are 1.  commit_head() makes an engine whose encoder_conv agrees with
the trainer's forward within kappa while the step moved C by many kappa.  Ten fit_head steps on one batch lower scalar_ploss.
training_state_dict() taken after two steps and loaded into a freshly enabled model continues for two more with the bits of the
uninterrupted run.  The flags of a model without conv_stack are what they were.  The refusals by name.  pytest -s prints the figures and the ambiguity counts.

The features.  The synthetic model's own features (sdfa_amd.synth's PCM through the front end) are smooth along frequency, and
neighbouring rows tie so closely that 1.2e-3 to 1.8e-3 of layer 3's pool routes are ambiguous on them: above the 1e-3 every case
is held to.  So the forward test and the train_step batch take seeded features of train_batch's scale instead
(convtrain_ref64.CHECKPOINT_CASES: the "default" family's, 12 and 6 frames); the batch is otherwise the sibling's three-window
batch (truth, weights, speaker ids).  On the checkpoint's tensors those features leave at most 178 of 3,145,728 elements (5.7e-5)
ambiguous; tests/test_convtrain_ref64_cpu.py asserts the cap for both on the model, and so do the tests here.

Measured on an MI355X (largest |gpu - ref64| / kappa): the conv stack on a checkpoint 0.031 (trainer) and 0.042 (engine), not the
same bits; train_step + optimizer_step: C 0.031, the conv gradients 7.8e-6 at most and the parameters 3e-10 (k_dC, carried in from
five stages above, dominates their kappa); commit_head: engine 0.035, trainer 0.036, the step having moved C by 628 x kappa;
fit_head: scalar_ploss 0.004756 -> 0.004271 in 10 steps.  The module takes 6 s.

This module fails to import without sdfa_amd.convtrain and tests/convtrain_ref64.py."""
import numpy as np
import pytest
import torch

import attntrain_ref64 as RA
import bilstm2_ref64 as B
import convtrain_ref64 as RC
import freqtrain_ref64 as RF
import headtrain_ref64 as RH
import lstmtrain_ref64 as R
from sdfa_amd import convtrain as CT        # the feature: absent before it
from test_gpu_freq_train_op import _batch, _device_rng_left_as_found, _model, bits, cols, dev, within  # noqa: F401  (the fixture is autouse)

pytestmark = pytest.mark.gpu

FLAGS = dict(attention=True, bilstm_top=True, bilstm_bottom=True, freq_lstm=True, conv_stack=True)
SLOTS = dict(head="_head_trainer", attn="_attn_trainer", lstm="_lstm_trainer", lstm0="_lstm0_trainer", freq="_freq_trainer", conv="_conv_trainer")


def _trainers(model):
    return {k: getattr(model, a) for k, a in SLOTS.items()}


def fcols(feat):
    """device audio_feat [N][64][128][3] -> the float64 model's [R][128][3]"""
    return feat.detach().cpu().numpy().reshape(-1, RC.BINS, RC.IN)


def conv_params(tr):
    return {**tr.parameters(), **tr.running_stats()}


def counts(r):
    return {L: (r["ambiguous_kink"][L], r["ambiguous_pool"][L], r["elements"][L]) for L in r["elements"]}


def test_trainer_forward_is_the_engines_conv_stack(synth_sd):
    from sdfa_amd import _lib, ops
    from sdfa_amd.engine import Engine
    assert CT.ABI_VERSION == _lib.lib.sdfa_convtrain_abi_version()
    sd = synth_sd["offsets"]
    eng = Engine(sd, device="cuda:0", max_frames=128)
    params, f = RC.checkpoint_case(sd, "forward")
    feat = dev(f.reshape(12, RC.COLS, RC.BINS, RC.IN))
    key = ops.register_model(None, eng)
    C_eng = torch.ops.sdfa.encoder_conv(feat, key)
    tr = CT.ConvTrainer(sd)
    C_tr = tr.forward(feat)
    got = conv_params(tr)
    assert all((bits(got[n]) == bits(params[n])).all() for n in params)
    r = RC.run(params, f)
    assert RC.under_cap(r), counts(r)
    worst = {}
    within(worst, "trainer's C", cols(C_tr), r["C"], r["k_C"])
    within(worst, "engine's C", cols(C_eng), r["C"], r["k_C"])
    print(f"\n12 frames: the conv stack on a checkpoint, largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items())
          + f"; (ambiguous kink, pool route, elements) {counts(r)}; bits equal: {bool(torch.equal(C_eng, C_tr))}")


def test_operator_backward_is_the_direct_calls():
    from sdfa_amd import ops  # noqa: F401  (registers torch.ops.sdfa.conv_train)
    N = 2
    c = RC.case(RC.COLS * N, 77, "edge")
    feat, dC = dev(c["feat"].reshape(N, RC.COLS, RC.BINS, RC.IN)), dev(c["dC"].reshape(N, RC.COLS, RC.OUT_BINS, RC.OUT))
    direct = CT.ConvTrainer(c["params"])
    Cd = direct.forward(feat)
    direct.backward(feat, dC)
    tr = CT.ConvTrainer(c["params"])
    fr = feat.detach().requires_grad_(True)
    Cx = torch.ops.sdfa.conv_train(fr, CT.register_trainer(tr))
    assert torch.equal(Cx.detach(), Cd)
    (Cx * dC).sum().backward()
    assert fr.grad is None                                   # the features are data
    ga, gb = tr.grads(), direct.grads()
    for n in ga:
        assert (bits(ga[n]) == bits(gb[n])).all(), n
    fake = torch.library.opcheck(torch.ops.sdfa.conv_train.default, (feat, CT.register_trainer(direct)), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake
    with pytest.raises(KeyError, match="no conv stack trainer registered"):
        CT.trainer_of("sdfa-conv-trainer-none")


def test_refusals_and_flags_by_name(synth_sd):
    msg = "head training: conv_stack=True needs freq_lstm=True: the conv stack is trained through the frequency LSTM's dC"
    with pytest.raises(NotImplementedError, match=msg):
        _model(synth_sd, attention=True, bilstm_top=True, bilstm_bottom=True, conv_stack=True)
    with pytest.raises(NotImplementedError, match=msg):
        _model(synth_sd, conv_stack=True)
    hp, with_conv = _model(synth_sd, **FLAGS)
    state = with_conv.training_state_dict()
    assert state["flags"] == dict(FLAGS, bilstm_dropout=0.0)
    assert set(state["trainers"]) == {"head", "attention", "bilstm_top", "bilstm_bottom", "freq_lstm", "conv_stack"}
    assert with_conv._freq_trainer.want_dC
    hp, without = _model(synth_sd, attention=True, bilstm_top=True, bilstm_bottom=True, freq_lstm=True)
    assert without._conv_trainer is None and not without._freq_trainer.want_dC
    # the flags of a model without it are the dict they were
    assert without.training_state_dict()["flags"] == dict(attention=True, bilstm_top=True, bilstm_bottom=True, bilstm_dropout=0.0, freq_lstm=True)
    with pytest.raises(ValueError, match=r"training state: taken with conv_stack=True \(this model: conv_stack=False\)"):
        without.load_training_state_dict(state)
    with pytest.raises(ValueError, match=r"taken with conv_stack=False \(this model: conv_stack=True\)"):
        with_conv.load_training_state_dict(without.training_state_dict())


def _seeded_batch(model, hp, synth_sd):
    """the sibling's three-window batch with the seeded features in place of the synthetic clips' (see "The features" above)"""
    ts, batch = _batch(model, hp)
    seeded = RC.checkpoint_case(synth_sd["offsets"], "train_step")[1]
    assert batch["audio_feat"].shape[0] * RC.COLS == len(seeded)
    return ts, dict(batch, audio_feat=dev(seeded.reshape(-1, RC.COLS, RC.BINS, RC.IN)))


@pytest.fixture(scope="module")
def tuned(synth_sd):
    """An offsets model after one train_step + optimizer_step with every stage enabled, with everything the checks need."""
    hp, model = _model(synth_sd, **FLAGS)
    ts, batch = _seeded_batch(model, hp, synth_sd)
    before = {k: t.parameters() for k, t in _trainers(model).items()}
    feat = batch["audio_feat"].contiguous()
    C_enc = torch.ops.sdfa.encoder_conv(feat, model._model._key)
    pred, losses, scalars = model.train_step(batch, 0)
    C_tr = model._freq_trainer._C.detach().clone()
    X0_tr = model._lstm0_trainer._X.detach().clone()
    H_tr = model._lstm_trainer._Y.detach().clone()
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    grads = {k: t.grads() for k, t in _trainers(model).items() if k != "head"}
    model.optimizer_step()
    return dict(model=model, hp=hp, ts=ts, batch=batch, before=before, feat=feat, C_enc=C_enc, C_tr=C_tr, X0_tr=X0_tr, H_tr=H_tr,
                coef=coef.detach(), dcoef=coef.grad.detach().clone(), pred=pred, scalars=scalars, losses=losses, grads=grads,
                stats=model._conv_trainer.running_stats())


def test_train_step_and_one_adam_step_within_kappa_of_the_restated_chain(tuned):
    m = tuned["model"]
    assert m.training and [t.step_count for t in _trainers(m).values()] == [1] * 6
    worst = {}
    before = {**tuned["before"]["conv"], **tuned["stats"]}
    cf = RC.run(before, fcols(tuned["feat"]))
    assert RC.under_cap(cf), counts(cf)
    within(worst, "C", cols(tuned["C_tr"]), cf["C"], cf["k_C"])
    within(worst, "C of the inference kernels", cols(tuned["C_enc"]), cf["C"], cf["k_C"])
    # the chain of tests/test_gpu_freq_train_op.py, each stage on the float32 input the device gave it, down to dC
    Cn, X0, H_dev = cols(tuned["C_tr"]), tuned["X0_tr"].cpu().numpy(), tuned["H_tr"].cpu().numpy()
    ones = np.ones(X0.shape[:2] + (R.NY,), np.float32)
    both = {**tuned["before"]["lstm0"], **tuned["before"]["lstm"]}
    z_dev = tuned["pred"]["condition"].detach().reshape(-1, 512).cpu().numpy()
    head = RH.run("offsets", tuned["before"]["head"], z_dev, tuned["batch"]["speaker_id"].cpu().numpy(), tuned["dcoef"].cpu().numpy())
    ab = RA.run(tuned["before"]["attn"], H_dev, head["dz"], ddz=head["k_dz"])
    lb = B.run(both, X0, ones, ab["dH"], kdH=ab["k_dH"])
    l0 = R.run(0, tuned["before"]["lstm0"], X0, lb["dY0"], kdY=lb["k_dY0"], want_dX=True)
    fb = RF.run(tuned["before"]["freq"], Cn, l0["dX"].reshape(-1, RF.NO), kdX0=l0["k_dX"].reshape(-1, RF.NO), want_dC=True)
    for n in RF.names():
        within(worst, "frequency grad", tuned["grads"]["freq"][n], fb["grads"][n], fb["k_grads"][n])
    cb = RC.run(before, fcols(tuned["feat"]), fb["dC"], kdC=fb["k_dC"])
    print(f"\n(ambiguous kink, pool route, elements) per layer {counts(cb)}")
    got = m._conv_trainer.parameters()
    assert set(got) == set(RC.names()) == set(cb["grads"])
    for n in RC.names():
        g = cb["grads"][n]
        kind = n[len(RC.P):]
        within(worst, f"conv {kind} grad", tuned["grads"]["conv"][n], g, cb["k_grads"][n])
        assert np.abs(g).max() > 0
        p1, _, _, kp, _, _ = RC.adam(tuned["before"]["conv"][n], g, 0.0 * g, 0.0 * g, 1, eg=cb["k_grads"][n])
        within(worst, f"conv {kind} param", got[n], p1, kp)
    for kind, tr in _trainers(m).items():                    # every tensor of all six trainers has moved
        now = tr.parameters()
        for n in now:
            assert (now[n] != tuned["before"][kind][n]).any(), (kind, n)
    for n, a in m._conv_trainer.running_stats().items():
        assert (bits(a) == bits(tuned["stats"][n])).all(), n
    print("train_step(conv_stack) + optimizer_step: largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert {"_model." + n for n in CT.tensor_shapes()} <= set(m.head_state_dict())
    assert not any("running" in k for k in m.head_state_dict())


def test_commit_head_feeds_the_tuned_conv_stack_to_inference(tuned):
    m = tuned["model"]
    old_engine = m._model._engine
    m.commit_head()
    assert m._model._engine is not old_engine
    C_new = torch.ops.sdfa.encoder_conv(tuned["feat"], m._model._key)
    C_tr = m._conv_trainer.forward(tuned["feat"])
    r = RC.run(conv_params(m._conv_trainer), fcols(tuned["feat"]))
    worst = {}
    within(worst, "engine's C", cols(C_new), r["C"], r["k_C"])
    within(worst, "trainer's C", cols(C_tr), r["C"], r["k_C"])
    kap = r["k_C"].reshape(C_new.shape)
    moved = np.abs((C_new - tuned["C_enc"]).cpu().numpy())
    assert (moved > 10 * kap).any()                          # the engine before the commit holds the untuned stack
    worst["moved C"] = float((moved / kap).max())
    print("\ncommit_head with the conv stack: |gpu - ref64| / kappa and what the step moved: " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items()))
    from sdfa_amd import synth
    ts_list, animes, _ = m.generate_animation(synth.make_pcm(3, 2 * 16000), "m0", 0, 0)
    assert len(ts_list) == animes.shape[0] > 0 and np.isfinite(animes).all()


def test_fit_head_with_the_conv_stack_on_a_fixed_batch_lowers_the_loss(tuned):
    m = tuned["model"]
    hist = m.fit_head(tuned["ts"], 10, np.random.RandomState(1), fixed_batch=tuned["batch"])
    assert len(hist) == 10 and [t.step_count for t in _trainers(m).values()] == [11] * 6
    first, last = hist[0]["scalar_ploss"], hist[-1]["scalar_ploss"]
    print(f"\nfit_head with the conv stack, 10 steps on one batch: scalar_ploss {first:.6g} -> {last:.6g}")
    assert last < first
    m._conv_trainer.step()                                    # out of step: refused
    with pytest.raises(RuntimeError, match="conv-stack trainer at step 12"):
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
    ts, batch = _seeded_batch(a, hp, synth_sd)
    rng = np.random.RandomState(1)
    a.fit_head(ts, 2, rng, fixed_batch=batch)
    state = a.training_state_dict()
    assert state["trainers"]["conv_stack"]["step"] == 2 and state["flags"]["conv_stack"] is True
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
