"""sdfa_encoder_x0 (include/sdfa_bilstm.h, torch.ops.sdfa.encoder_x0) and training BOTH layers of the BiLSTM in
SaberSpeechDrivenAnimation -- enable_head_training(attention=True, bilstm_top=True, bilstm_bottom=True), train_step, fit_head,
head_state_dict, commit_head, training_state_dict / load_training_state_dict -- on the synthetic offsets model, on the GPU.

sdfa_encoder_x0 at 72 frames and at 200 frames on an engine whose workspace holds one 128-frame chunk: X0 [N][64][256] is finite
and not zero, the operator equals the method, the option encoder_dedup_off gives the same bits, an LstmTrainer(layer=0) holding the
checkpoint's weights maps X0 to sdfa_encoder_layer0's X1 within kappa (other kernels, the same function), and sdfa_encoder_layer0
and sdfa_encoder_memory give after it the bits they gave before it.

The two trainers chained through torch.ops.sdfa.lstm_train with a seeded keep mask between them and a set dH, at N = 1, 2 and
65 = 2 x 32 + 1 frames (two whole recurrence tiles and one frame; three row blocks, the last of one frame): H, both layers'
gradients and both layers' parameters after one Adam step within 1 x kappa of tests/bilstm2_ref64.py, no factor applied; its
wrong variants at least 10 x kappa from the device; two runs the same bits.

One train_step(bilstm_bottom=True) + the summed losses' backward + optimizer_step on the three-window synthetic batch of
tests/test_gpu_lstm_train_op.py within 1 x kappa of the chain bilstm2_ref64 -> attention ref64 -> head ref64 -> Adam, built as
that module builds its chain: each stage's forward on the float32 input the device gave it (the two BiLSTM layers are one stage,
on the device's X0), each stage's gradient and kappa fed on backwards.  commit_head() makes an engine whose layer-0 output and H
agree with the trainers' within kappa while the step moved both by many kappa.  bilstm_dropout = 0.1 with a seeded generator is the
explicitly masked step, bit for bit.  Twenty fit_head steps on one batch lower scalar_ploss.  training_state_dict() taken after
two steps and loaded into a freshly enabled model continues for two more with the bits of the uninterrupted run (parameters,
moments, scalers, dropout draws).  The refusals by name.

Measured on an MI355X (largest |gpu - ref64| / kappa): layer 0 on sdfa_encoder_x0's X0 0.0141 (trainer) and 0.0153 (engine) at 72
frames, 0.0168 and 0.0168 at 200; the chained trainers at N = 1 / 2 / 65: H 0.0010 / 0.0012 / 0.0018, X1 0.0091 / 0.0075 / 0.0138, dX1
0.0024 / 0.0045 / 0.0052, dY0 0.0024 / 0.0038 / 0.0051, a gradient 0.0005 at most, a parameter after one step 0.0231 at most; the
controls 86.7 (layer 0 left untrained, N = 65) to 7.41e3 x kappa from the device; train_step + optimizer_step 0.0964 at most (a
head parameter; Y0 0.0121, H 0.0062, the BiLSTM gradients below 5e-5); commit_head: engine against model 0.0157 (X1) and 0.0044 (H),
the step having moved them by 734 and 604 x kappa; fit_head: scalar_ploss 0.00488 -> 0.00420.  The module takes 18 s.

This module fails to import without sdfa_amd.bilstmtrain and tests/bilstm2_ref64.py."""
import functools

import numpy as np
import pytest
import torch

import attntrain_ref64 as RA
import bilstm2_ref64 as B
import headtrain_ref64 as RH
import lstmtrain_ref64 as R
from sdfa_amd import attntrain as AT
from sdfa_amd import bilstmtrain as BT        # the feature: absent before it
from sdfa_amd import headtrain as HT
from sdfa_amd import lstmtrain as LT
from test_gpu_train_losses import _train_set

pytestmark = pytest.mark.gpu

P_DROP = 0.1


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


def away(got, val, kap):
    return float((np.abs(np.asarray(got, np.float64).reshape(val.shape) - val) / np.maximum(kap, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------- sdfa_encoder_x0
@pytest.mark.parametrize("n_frames", [72, 200], ids=["one-partial-chunk", "two-chunks"])
def test_encoder_x0_is_the_input_of_layer0(synth_sd, n_frames):
    from sdfa_amd import _lib, ops, synth
    from sdfa_amd.engine import Engine
    assert BT.ABI_VERSION == _lib.lib.sdfa_bilstm_abi_version()
    sd = synth_sd["offsets"]
    eng = Engine(sd, device="cuda:0", max_frames=128)        # a workspace of one 128-frame chunk: 200 frames take two
    pcm = synth.make_pcm(1, 16000 * n_frames // 60)
    feat, _, _ = eng.mel_frontend([pcm], 16000)
    feat = feat[:n_frames].contiguous()
    assert feat.shape[0] == n_frames
    X1_before = eng.encoder_layer0(feat)
    H_before, z_before, align_before = eng.encoder_memory(feat)
    X0 = eng.encoder_x0(feat)
    assert X0.shape == (n_frames, BT.STEPS, BT.FEATURES) and X0.dtype == torch.float32 and X0.is_contiguous()
    assert bool(torch.isfinite(X0).all()) and float(X0.abs().mean()) > 1e-4
    assert (X0.abs().amax(dim=(1, 2)) > 0).all()             # every frame was written, the second chunk's too
    key = ops.register_model(None, eng)
    assert torch.equal(torch.ops.sdfa.encoder_x0(feat, key), X0)
    fake = torch.library.opcheck(torch.ops.sdfa.encoder_x0.default, (feat, key), test_utils=("test_schema", "test_faketensor"))
    assert all(v == "SUCCESS" for v in fake.values()), fake
    # the every-column path gives the same bits
    _lib.set_option("encoder_dedup_off", 1)
    try:
        X0_off = eng.encoder_x0(feat)
    finally:
        _lib.set_option("encoder_dedup_off", 0)
    assert torch.equal(X0_off, X0)
    # layer 0 with the checkpoint's weights, the training kernels and the inference kernels, on this X0
    tr = LT.LstmTrainer(sd, layer=0)
    Y0 = tr.forward(X0)
    r = R.run(0, tr.parameters(), X0.cpu().numpy())
    worst = {}
    within(worst, "trainer's Y0", Y0.cpu().numpy(), r["Y"], r["k_Y"])
    within(worst, "engine's X1", X1_before.cpu().numpy(), r["Y"], r["k_Y"])
    print(f"\n{n_frames} frames: layer 0 on sdfa_encoder_x0's X0, largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    # the other entry points launch what they launched: the same bits after the X0 exit used the workspace
    assert torch.equal(eng.encoder_layer0(feat), X1_before)
    H_after, z_after, align_after = eng.encoder_memory(feat)
    assert torch.equal(H_after, H_before) and torch.equal(z_after, z_before) and torch.equal(align_after, align_before)
    # the refusals of sdfa_encoder_layer0, with real buffers
    ws = eng.workspace(n_frames)
    x0p, fp, wp = X0.data_ptr(), feat.data_ptr(), ws.data_ptr()
    call = _lib.lib.sdfa_encoder_x0
    assert call(eng._m, fp, n_frames, None, wp, ws.numel(), None) == _lib.EINVAL
    assert call(eng._m, fp, n_frames, x0p + 4, wp, ws.numel(), None) == _lib.EINVAL and b"16-byte aligned" in _lib.lib.sdfa_last_error()
    assert call(eng._m, None, n_frames, x0p, wp, ws.numel(), None) == _lib.EINVAL
    assert call(eng._m, fp, -1, x0p, wp, ws.numel(), None) == _lib.EINVAL
    assert call(eng._m, fp, n_frames, x0p, wp, 4096, None) == _lib.ENOSPACE
    assert call(eng._m, fp, 0, x0p, wp, ws.numel(), None) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(eng.encoder_x0(feat), X0)


# ---------------------------------------------------------------------------------------------------- the two trainers, chained
N_TILES_PLUS_ONE = 2 * LT.TILE_FRAMES + 1
SIZES = (1, 2, N_TILES_PLUS_ONE)


@functools.lru_cache(maxsize=None)
def chain_case(N):
    """lstmtrain_ref64's seeded two-layer "carry" case, a seeded keep mask, and a set dH with a common component: dH = (gaussian + 1) / N.
    The common component is there for the controls.  kappa of dW_ih, dW_hh adds the rows' errors linearly (lstmtrain_ref64: "rows"),
    so it grows with the 64 N rows; a zero-mean dH gives weight gradients that grow with their square root only, and at 4,160 rows
    kappa is then too loose for a control that acts on layer 0's gradients alone (on the CPU, wrong model against right model at
    N = 65 with the zero-mean dH: "layer 0 left untrained" 10.0 x kappa at most, "the mask left out of the backward" 1.9).  A dH
    with a common component -- what a loss hands back -- gives gradients that grow with the rows as kappa does (58 - 87 x kappa for the
    former at N = 65).  The latter changes a tenth of dY0's elements at random and averages out of the weight gradients at any dH
    (3.1 x kappa at N = 65): it is judged on dY0 itself, the gradient autograd hands to layer 0, which the device forms elementwise."""
    c = R.stack_case(N, 400 + N, "carry")
    keep = (np.random.RandomState(900 + N).uniform(size=(N, R.TS, R.NY)) >= P_DROP).astype(np.float32) / np.float32(1.0 - P_DROP)
    return dict(c, keep=keep, dY=(c["dY"] + np.float32(1.0 / N)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def chain_model(N):
    c = chain_case(N)
    p1, _, _, k1, _, _, first = B.train_steps(c["params"], c["X"], c["keep"], c["dY"], 1)
    return p1, k1, first


def chain_device(N):
    """H, X1, both layers' gradients and their parameters after one step, through torch.ops.sdfa.lstm_train with the mask in the graph"""
    from sdfa_amd import ops  # noqa: F401
    c = chain_case(N)
    t0 = LT.LstmTrainer(c["params"], layer=0, want_dX=False)
    t1 = LT.LstmTrainer(c["params"], layer=1, want_dX=True)
    X0 = dev(c["X"]).requires_grad_(True)
    Y0 = torch.ops.sdfa.lstm_train(X0, LT.register_trainer(t0))
    X1 = Y0 * dev(c["keep"])
    H = torch.ops.sdfa.lstm_train(X1, LT.register_trainer(t1))
    Y0.retain_grad()
    X1.retain_grad()
    H.backward(dev(c["dY"]))
    assert X0.grad is None                                   # nothing below layer 0 is trained: no dX0 is formed
    out = dict(H=H.detach().cpu().numpy(), X1=X1.detach().cpu().numpy(), dX1=X1.grad.cpu().numpy(), dY0=Y0.grad.cpu().numpy(),
               grads={**t0.grads(), **t1.grads()})
    t0.step()
    t1.step()
    out["params1"] = {**t0.parameters(), **t1.parameters()}
    return out


_DEVICE = {}


def chain_device_once(N):
    if N not in _DEVICE:
        _DEVICE[N] = chain_device(N)
    return _DEVICE[N]


@pytest.mark.parametrize("N", SIZES)
def test_chained_trainers_within_kappa_of_the_masked_two_layer_model(N):
    p1, k1, first = chain_model(N)
    got = chain_device_once(N)
    worst = {}
    within(worst, "H", got["H"], first["H"], first["k_H"])
    within(worst, "X1", got["X1"], first["X1"], first["k_X1"])
    within(worst, "dX1", got["dX1"], first["dX1"], first["k_dX1"])
    within(worst, "dY0", got["dY0"], first["dY0"], first["k_dY0"])
    dropped = chain_case(N)["keep"] == 0
    assert (got["X1"][dropped] == 0).all() and (got["dY0"][dropped] == 0).all() and 0.02 < dropped.mean() < 0.2
    for n in B.names():
        layer = n[-1] if not n.endswith("_reverse") else n[-9]
        within(worst, f"grad l{layer}", got["grads"][n], first["grads"][n], first["k_grads"][n])
        within(worst, f"param1 l{layer}", got["params1"][n], p1[n], k1[n])
        assert (bits(got["params1"][n]) != bits(chain_case(N)["params"][n])).mean() > 0.5, n
    print(f"\nN = {N}: layer 0 -> mask -> layer 1 through torch.ops.sdfa.lstm_train, largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    again = chain_device(N)
    for k in ("H", "X1", "dX1", "dY0"):
        assert (bits(again[k]) == bits(got[k])).all(), k
    for n in B.names():
        assert (bits(again["grads"][n]) == bits(got["grads"][n])).all() and (bits(again["params1"][n]) == bits(got["params1"][n])).all(), n


@pytest.mark.parametrize("flaw", B.FLAWS)
@pytest.mark.parametrize("N", SIZES)
def test_controls_are_outside_kappa_of_the_device(N, flaw):
    """Each wrong model lies at least 10 x kappa (the right model's, as it stands) from the device on at least one output.  "Layer 0
    left untrained" leaves H as it is and is judged on layer 0's gradients and parameters.  "The mask left out of the backward"
    leaves H as it is too, and kappa of layer 0's weight gradients is too loose for it beyond a few frames (chain_case): it is judged
    on dY0.  Where the mask is 0, dY0 is an exact 0 and its kappa is 0; the larger kappa of dX1 is taken there, so the figure is
    finite and the control has to clear more, not less."""
    c, got = chain_case(N), chain_device_once(N)
    p1, k1, first = chain_model(N)
    w = B.run(c["params"], c["X"], c["keep"], c["dY"], flaw=flaw, base=first)
    ratios = dict(H=away(got["H"], w["H"], first["k_H"]), dY0=away(got["dY0"], w["dY0"], np.maximum(first["k_dY0"], first["k_dX1"])))
    for n in B.names():
        s = n[len(R.P):]
        ratios["grad " + s] = away(got["grads"][n], w["grads"][n], first["k_grads"][n])
        wp = B.adam(c["params"][n], w["grads"][n], 0.0 * w["grads"][n], 0.0 * w["grads"][n], 1)[0]
        ratios["param1 " + s] = away(got["params1"][n], wp, k1[n])
    worst = max(ratios.values())
    print(f"\nN = {N}, {flaw}: the device lies {worst:.3g} x kappa from this wrong model (H {ratios['H']:.3g}; dY0 {ratios['dY0']:.3g}; layer 0: "
          f"{max(v for k, v in ratios.items() if '_l0' in k):.3g}; layer 1: {max(v for k, v in ratios.items() if '_l1' in k):.3g})")
    assert worst >= 10.0, (flaw, ratios)
    if flaw in ("mask_not_in_backward", "layer0_untrained"):
        assert ratios["H"] <= 1.0 and max(v for k, v in ratios.items() if "_l1" in k) <= 1.0      # they leave the forward and layer 1 alone


# ---------------------------------------------------------------------------------------------------- the model
FLAGS = dict(attention=True, bilstm_top=True, bilstm_bottom=True)


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
    return dict(head=model._head_trainer, attn=model._attn_trainer, lstm=model._lstm_trainer, lstm0=model._lstm0_trainer)


def test_refusals_by_name(synth_sd):
    with pytest.raises(NotImplementedError, match="bilstm_bottom=True needs bilstm_top=True"):
        _model(synth_sd, attention=True, bilstm_bottom=True)
    with pytest.raises(NotImplementedError, match="bilstm_bottom=True needs bilstm_top=True"):
        _model(synth_sd, bilstm_bottom=True)
    hp, both = _model(synth_sd, **FLAGS)
    state = both.training_state_dict()
    assert state["flags"] == dict(FLAGS, bilstm_dropout=0.0) and set(state["trainers"]) == {"head", "attention", "bilstm_top", "bilstm_bottom"}
    hp, top = _model(synth_sd, attention=True, bilstm_top=True)
    assert top._lstm0_trainer is None and not top._lstm_trainer.want_dX
    with pytest.raises(ValueError, match=r"training state: taken with bilstm_bottom=True \(this model: bilstm_bottom=False\)"):
        top.load_training_state_dict(state)
    with pytest.raises(ValueError, match=r"taken with bilstm_bottom=False \(this model: bilstm_bottom=True\)"):
        both.load_training_state_dict(top.training_state_dict())
    hp, drop = _model(synth_sd, bilstm_dropout=P_DROP, **FLAGS)
    with pytest.raises(ValueError, match=r"taken with bilstm_dropout=0.0 \(this model: bilstm_dropout=0.1\)"):
        drop.load_training_state_dict(state)
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    with pytest.raises(RuntimeError, match="head training is not enabled"):
        SaberSpeechDrivenAnimation(hp).training_state_dict()


@pytest.fixture(scope="module")
def tuned(synth_sd):
    """An offsets model after one train_step + optimizer_step with both BiLSTM layers enabled, with everything the checks need."""
    hp, model = _model(synth_sd, **FLAGS)
    assert model._attn_trainer.want_dH and model._lstm_trainer.want_dX and model._lstm_trainer.layer == 1
    assert not model._lstm0_trainer.want_dX and model._lstm0_trainer.layer == 0
    ts, batch = _batch(model, hp)
    before = {k: t.parameters() for k, t in _trainers(model).items()}
    feat = batch["audio_feat"].contiguous()
    X0 = torch.ops.sdfa.encoder_x0(feat, model._model._key)
    X1_enc = torch.ops.sdfa.encoder_layer0(feat, model._model._key)
    H_enc, _, _ = torch.ops.sdfa.encoder_memory(feat, model._model._key)
    pred, losses, scalars = model.train_step(batch, 0)
    assert torch.equal(model._lstm0_trainer._X, X0)
    Y0_tr = model._lstm0_trainer._Y.detach().clone()
    H_tr = model._lstm_trainer._Y.detach().clone()
    assert torch.equal(model._lstm_trainer._X, Y0_tr)         # bilstm_dropout = 0: no mask between the layers
    coef = pred["prediction"]["verts_off_3d_coef"]
    coef.retain_grad()
    sum(losses.values()).backward()
    grads = {k: t.grads() for k, t in _trainers(model).items() if k != "head"}
    model.optimizer_step()
    return dict(model=model, hp=hp, ts=ts, batch=batch, before=before, X0=X0, X1_enc=X1_enc, H_enc=H_enc, Y0_tr=Y0_tr, H_tr=H_tr,
                coef=coef.detach(), dcoef=coef.grad.detach().clone(), pred=pred, scalars=scalars, losses=losses, grads=grads)


def test_train_step_and_one_adam_step_within_kappa_of_the_restated_chain(tuned):
    m = tuned["model"]
    assert set(tuned["losses"]) == {"dyn_ploss", "dyn_mloss"} and tuned["scalars"]["scalar_ploss"] > 0
    assert m.training and [t.step_count for t in _trainers(m).values()] == [1, 1, 1, 1]
    X0 = tuned["X0"].cpu().numpy()
    ones = np.ones(X0.shape[:2] + (R.NY,), np.float32)
    sid = tuned["batch"]["speaker_id"].cpu().numpy()
    both = {**tuned["before"]["lstm0"], **tuned["before"]["lstm"]}
    worst = {}
    lf = B.run(both, X0, ones)
    within(worst, "Y0", tuned["Y0_tr"].cpu().numpy(), lf["Y0"], lf["k_Y0"])
    within(worst, "H", tuned["H_tr"].cpu().numpy(), lf["H"], lf["k_H"])
    # with untouched parameters the trained layers are the inference layers: other kernels, the same function
    within(worst, "X1 of the inference kernels", tuned["X1_enc"].cpu().numpy(), lf["Y0"], lf["k_Y0"])
    within(worst, "H of the inference kernels", tuned["H_enc"].cpu().numpy(), lf["H"], lf["k_H"])
    # each later stage's forward is judged on the float32 input the device gave it, as tests/test_gpu_lstm_train_op.py does
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
            assert np.abs(g).max() > 0
            p1, _, _, kp, _, _ = R.adam(tuned["before"][kind][n], g, 0.0 * g, 0.0 * g, 1, eg=lb["k_grads"][n])
            within(worst, f"BiLSTM l{layer} param", got[n], p1, kp)
            assert (got[n] != tuned["before"][kind][n]).mean() > 0.5, n          # every tensor of both layers has moved
    got = m._attn_trainer.parameters()
    for n, g in ab["grads"].items():
        p1, _, _, kp, _, _ = RA.adam(tuned["before"]["attn"][n], g, 0.0 * g, 0.0 * g, 1, eg=ab["k_grads"][n])
        within(worst, "attention param", got[n], p1, kp)
    got = m._head_trainer.parameters()
    for n, g in head["grads"].items():
        p1, _, _, kp, _, _ = RH.adam(tuned["before"]["head"][n], g, 0.0 * g, 0.0 * g, 1, eg=head["k_grads"][n])
        within(worst, "head param", got[n], p1.reshape(got[n].shape), kp.reshape(got[n].shape))
    print("\ntrain_step(bilstm_bottom) + optimizer_step: largest |gpu - ref64| / kappa: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert set(m.head_state_dict()) == {"_model." + n for n in list(HT.tensor_shapes("offsets")) + list(AT.tensor_shapes()) + list(LT.tensor_shapes(1)) + list(LT.tensor_shapes(0))}


def test_commit_head_feeds_both_tuned_layers_to_inference(tuned):
    m = tuned["model"]
    old_engine = m._model._engine
    feat = tuned["batch"]["audio_feat"].contiguous()
    m.commit_head()
    assert m._model._engine is not old_engine
    assert torch.equal(torch.ops.sdfa.encoder_x0(feat, m._model._key), tuned["X0"])          # everything below the BiLSTM is frozen
    X1_new = torch.ops.sdfa.encoder_layer0(feat, m._model._key)
    H_new, _, _ = torch.ops.sdfa.encoder_memory(feat, m._model._key)
    Y0_tr = m._lstm0_trainer.forward(tuned["X0"])
    H_tr = m._lstm_trainer.forward(Y0_tr)
    X0 = tuned["X0"].cpu().numpy()
    both = {**m._lstm0_trainer.parameters(), **m._lstm_trainer.parameters()}
    r = B.run(both, X0, np.ones(X0.shape[:2] + (R.NY,), np.float32))
    worst = {}
    for what, got, val, kap in (("engine's X1", X1_new, "Y0", "k_Y0"), ("trainer's Y0", Y0_tr, "Y0", "k_Y0"), ("engine's H", H_new, "H", "k_H"), ("trainer's H", H_tr, "H", "k_H")):
        within(worst, what, got.cpu().numpy(), r[val], r[kap])
    for new, tr, old, kap in ((X1_new, Y0_tr, tuned["X1_enc"], r["k_Y0"]), (H_new, H_tr, tuned["H_enc"], r["k_H"])):
        assert (np.abs((new - tr).cpu().numpy()) <= kap).all()
        moved = np.abs((new - old).cpu().numpy())
        assert (moved > 10 * kap).any()                       # the engine before the commit holds the untuned layers
        worst[f"moved {'X1' if kap is r['k_Y0'] else 'H'}"] = float((moved / kap).max())
    print("\ncommit_head with both layers: |gpu - ref64| / kappa and what the step moved: " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items()))
    from sdfa_amd import synth
    ts_list, animes, _ = m.generate_animation(synth.make_pcm(3, 2 * 16000), "m0", 0, 0)
    assert len(ts_list) == animes.shape[0] > 0 and np.isfinite(animes).all()


def test_fit_head_with_both_layers_on_a_fixed_batch_lowers_the_loss(tuned):
    m = tuned["model"]
    hist = m.fit_head(tuned["ts"], 20, np.random.RandomState(1), fixed_batch=tuned["batch"])
    assert len(hist) == 20 and [t.step_count for t in _trainers(m).values()] == [21, 21, 21, 21]
    first, last = hist[0]["scalar_ploss"], hist[-1]["scalar_ploss"]
    print(f"\nfit_head with both BiLSTM layers, 20 steps on one batch: scalar_ploss {first:.6g} -> {last:.6g}")
    assert last < first
    m._lstm0_trainer.step()                                   # out of step: refused
    with pytest.raises(RuntimeError, match="BiLSTM bottom-layer trainer at step 22"):
        m.optimizer_step()


def _one_step(model, batch):
    pred, losses, _ = model.train_step(batch, 0)
    sum(losses.values()).backward()
    return pred, {k: t.grads() for k, t in _trainers(model).items()}


def test_dropout_with_a_seeded_generator_is_the_explicitly_masked_step(synth_sd):
    hp, model = _model(synth_sd, bilstm_dropout=P_DROP, **FLAGS)
    ts, batch = _batch(model, hp)
    model._train_generator = torch.Generator(device="cuda").manual_seed(1234)
    pred, grads = _one_step(model, batch)
    # the same draw, applied by hand, in a graph over the trainers of a model without dropout
    hp2, plain = _model(synth_sd, **FLAGS)
    X0 = torch.ops.sdfa.encoder_x0(batch["audio_feat"].contiguous(), plain._model._key)
    keep = torch.empty(X0.shape[0], 64, 512, device="cuda").bernoulli_(1.0 - P_DROP, generator=torch.Generator(device="cuda").manual_seed(1234))
    assert 0.85 < float(keep.mean()) < 0.95
    keep = keep / (1.0 - P_DROP)
    Xr = X0.clone().requires_grad_(True)
    Y0 = torch.ops.sdfa.lstm_train(Xr, plain._lstm0_trainer_key)
    X1 = Y0 * keep
    assert torch.equal(model._lstm0_trainer._X, X0) and torch.equal(model._lstm_trainer._X, X1.detach())
    assert float((model._lstm_trainer._X == 0).float().mean()) > 0.05
    zz, align = torch.ops.sdfa.attn_train(torch.ops.sdfa.lstm_train(X1, plain._lstm_trainer_key), plain._attn_trainer_key)
    cc = torch.ops.sdfa.head_train(zz, batch["speaker_id"], plain._head_trainer_key)
    assert torch.equal(zz.detach(), pred["condition"].detach().reshape(-1, 512)) and torch.equal(align, pred["align_dict"]["audio_encoder10"].reshape(-1, 64))
    assert torch.equal(cc.detach(), pred["prediction"]["verts_off_3d_coef"].detach())
    plain.train()                                             # as train_step does: the dynamic loss scalers update in training mode
    losses, _ = plain.get_loss(dict(prediction={"verts_off_3d_coef": cc}, condition=zz.view(-1, 1, 512), align_dict={}, latent_dict={}), batch)
    sum(losses.values()).backward()
    for kind, tr in _trainers(plain).items():
        g = tr.grads()
        for n in g:
            assert (bits(g[n]) == bits(grads[kind][n])).all(), (kind, n)
    # another seed draws another mask; p = 0 draws none
    model._train_generator.manual_seed(99)
    model.train_step(batch, 1)
    assert not torch.equal(model._lstm_trainer._X, X1.detach())
    plain.train_step(batch, 0)
    assert torch.equal(plain._lstm_trainer._X, plain._lstm0_trainer._Y) and getattr(plain, "_train_generator", None) is None


def _snapshot(model):
    out = {}
    for kind, tr in _trainers(model).items():
        m, v = tr.moments()
        out[kind] = (tr.parameters(), m, v, tr.step_count)
    out["scalers"] = {k: sc.state_dict() for k, sc in model._loss_scalers.items()}
    out["generator"] = model._train_generator.get_state().clone()
    return out


def test_training_state_dict_resumes_bit_for_bit(synth_sd):
    hp, a = _model(synth_sd, bilstm_dropout=P_DROP, **FLAGS)
    ts, batch = _batch(a, hp)
    a._train_generator = torch.Generator(device="cuda").manual_seed(7)
    rng = np.random.RandomState(1)
    a.fit_head(ts, 2, rng, fixed_batch=batch)
    state = a.training_state_dict()
    assert state["generator"] is not None and set(state["scalers"]) == {"dyn_p", "dyn_m"} and state["trainers"]["bilstm_bottom"]["step"] == 2
    at_two = _snapshot(a)
    hist_a = a.fit_head(ts, 2, rng, fixed_batch=batch)
    hp_b, b = _model(synth_sd, bilstm_dropout=P_DROP, **FLAGS)
    assert b.load_training_state_dict(state) is b
    back = _snapshot(b)
    for kind in _trainers(b):
        for x, y in zip(at_two[kind][:3], back[kind][:3]):
            for n in x:
                assert (bits(x[n]) == bits(y[n])).all(), (kind, n)
        assert back[kind][3] == 2
    assert back["scalers"] == at_two["scalers"] and torch.equal(back["generator"], at_two["generator"])
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
    assert torch.equal(end_a["generator"], end_b["generator"]) and not torch.equal(end_a["generator"], at_two["generator"])
    # a model that drew other masks ends elsewhere: the draws are part of what is resumed
    hp_c, c = _model(synth_sd, bilstm_dropout=P_DROP, **FLAGS)
    c.load_training_state_dict(state)
    c._train_generator.manual_seed(8)
    c.fit_head(ts, 2, rng, fixed_batch=batch)
    pc, pa = c._lstm0_trainer.parameters(), a._lstm0_trainer.parameters()
    assert any((bits(pc[n]) != bits(pa[n])).any() for n in pa)
