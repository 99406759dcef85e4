"""PyTorch-ROCm custom operators over the C ABI: `torch.ops.sdfa.*` (BASELINE north_star: "called from the existing Python
host through PyTorch-ROCm custom ops"; SURVEY.md section 8(b) names them).

    torch.ops.sdfa.frame_index(n_samples, sample_rate, fps, ts_delta)                    -> (starts int64[F], tslist int32[F])   (host)
    torch.ops.sdfa.mel_frontend(pcm, clip_off, clip_len, frame_clip, frame_start, sr)     -> audio_feat f32[F,64,128,3]
    torch.ops.sdfa.encoder(audio_feat, model)                                             -> (z f32[N,512], align f32[N,64])
    torch.ops.sdfa.encoder_shared(audio_feat, frame_clip, frame_start, hop, model)        -> the same, bitwise, with the per-column stages
                                                                                             run once per distinct column of the frame table
    torch.ops.sdfa.regress(z, speaker_id, model)                                          -> dgrad f32[N,89784] | offsets f32[N,15069]
    torch.ops.sdfa.regress_into(z, speaker_id, out, model)                                -> None (rows written into `out`; ids must be validated)
    torch.ops.sdfa.regress_coef(z, speaker_id, model)                                     -> PCA coefficients f32[N,265 | 59]
    torch.ops.sdfa.objective(coef, truth, weight, model)                                  -> (loss f32[4], rec f64[2B,4], grad f32[2,2B,Kc])
    torch.ops.sdfa.train_losses(coef, truth, weight, model)                               -> loss f32[4] = (ps, ms, pr, mr), differentiable in coef
    torch.ops.sdfa.head_train(z, speaker_id, trainer_key)                                 -> PCA coefficients f32[N,265 | 59] of a HeadTrainer's head;
                                                                                             backward leaves the head's gradients in the trainer, returns dz
    torch.ops.sdfa.encoder_memory(audio_feat, model)                                      -> (H f32[N,64,512], z f32[N,512], align f32[N,64]); z, align bitwise encoder's
    torch.ops.sdfa.attn_train(H, trainer_key)                                             -> (z f32[N,512], align f32[N,64]) of an AttnTrainer's attention layer;
                                                                                             backward leaves the layer's gradients in the trainer, returns dH (or None)
    torch.ops.sdfa.encoder_layer0(audio_feat, model)                                      -> X1 f32[N,64,512], the BiLSTM's layer-0 output (no layer 1, no attention)
    torch.ops.sdfa.encoder_x0(audio_feat, model)                                          -> X0 f32[N,64,256], the BiLSTM's input (the frequency projection as rows; no BiLSTM)
    torch.ops.sdfa.lstm_train(X, trainer_key)                                           -> Y f32[N,64,512] of an LstmTrainer's BiLSTM layer, X f32[N,64,256 | 512];
                                                                                             backward leaves the layer's gradients in the trainer, returns dX (or None)
    torch.ops.sdfa.encoder_conv(audio_feat, model)                                        -> C f32[N,64,32,64], the conv stack's output as the frequency LSTM reads it (no frequency LSTM)
    torch.ops.sdfa.freq_train(C, trainer_key)                                             -> X0 f32[N,64,256] of a FreqTrainer's frequency LSTM and projection;
                                                                                             backward leaves their gradients in the trainer, returns dC (or None)
    torch.ops.sdfa.conv_train(audio_feat, trainer_key)                                    -> C f32[N,64,32,64] of a ConvTrainer's conv stack;
                                                                                             backward leaves its gradients in the trainer, returns None

Thin by design: each op is the matching `Engine` method (ctypes call into libsdfa_hip.so on the current stream), registered
with the dispatcher through `torch.library.custom_op` and given a fake-tensor shape function, so the ops compose with
torch.compile / torch.export / torch.jit.trace like any other operator.  `model` is the string key of a model in this
process' registry (`register_model` / `load_model`); a key that is the path of a checkpoint file is loaded on first use, which
is what lets a module traced by `speech_anime.api.jit_trace` run in a fresh process.  No CPU kernels are registered: calling a
device op with CPU tensors raises (the product path has no CPU fallback).
"""
import itertools
import os
import weakref
from typing import Tuple

import numpy as np
import torch
from torch import Tensor
from torch.library import custom_op

_MODELS = {}               # key -> Engine, for models loaded BY this module (load_model: the registry owns them)
_WEAK = {}                 # key -> weakref to an Engine owned by someone else (register_model): dropped with its owner
_ANON = itertools.count(1)


def register_model(key, engine, own=False):
    """`engine`: a sdfa_amd.engine.Engine (anything with encoder / regress / out_dim / coef_dim).  The registry keeps a WEAK
    reference unless `own` is set: an Engine holds the weights and a multi-GB workspace, and a model object that is dropped
    (SpeechDrivenAnimation re-loaded in a long-lived process) must free them, as a dropped module does in the reference.
    `key` None: a fresh key from a monotonically increasing counter (never reused, unlike id())."""
    key = f"sdfa-model-{next(_ANON)}" if key is None else str(key)
    _MODELS.pop(key, None)
    _WEAK.pop(key, None)
    if own:
        _MODELS[key] = engine
    else:
        _WEAK[key] = weakref.ref(engine, lambda _r, k=key: _WEAK.pop(k, None) if _WEAK.get(k) is _r else None)
    return key


def unregister_model(key):
    _MODELS.pop(str(key), None)
    _WEAK.pop(str(key), None)


def load_model(key, state_dict=None, **engine_kwargs):
    """Registers Engine(state_dict) under `key`; without a state_dict `key` must be a checkpoint path (torch.save'd dict
    with a "state" entry, the reference's layout: saber/trainer/manager/checkpoints.py:10-48)."""
    from .engine import Engine
    if state_dict is None:
        from .weights import ckpt_backward_compatible_preprocess
        ckpt = torch.load(os.path.expanduser(key), map_location="cpu", weights_only=False)
        if "hamm" in ckpt["state"]:
            ckpt = ckpt_backward_compatible_preprocess(ckpt)
        state_dict = ckpt["state"]
    return register_model(key, Engine(state_dict, **engine_kwargs), own=True)


def _model(key):
    m = _MODELS.get(key)
    if m is None and key in _WEAK:
        m = _WEAK[key]()
    if m is None:
        if os.path.isfile(os.path.expanduser(key)):
            load_model(key)
            return _MODELS[key]
        raise KeyError(f"sdfa: no model registered as {key!r} (sdfa_amd.ops.register_model / load_model)")
    return m


# --------------------------------------------------------------------------------------------------- frame_index (host)
@custom_op("sdfa::frame_index", mutates_args=())
def frame_index(n_samples: int, sample_rate: int, fps: int, ts_delta: int) -> Tuple[Tensor, Tensor]:
    from .engine import frame_index as _fi
    starts, ts = _fi(n_samples, sample_rate, fps, ts_delta)
    return torch.from_numpy(np.ascontiguousarray(starts)), torch.from_numpy(np.ascontiguousarray(ts))


@frame_index.register_fake
def _(n_samples, sample_rate, fps, ts_delta):
    ctx = torch.library.get_ctx()
    f = ctx.new_dynamic_size()          # F = floor((L + sliding) * fps / sr) + 2 in exact arithmetic; data dependent under float32 rounding
    return torch.empty(f, dtype=torch.int64), torch.empty(f, dtype=torch.int32)


# --------------------------------------------------------------------------------------------------- front end
_FE = {}


def _frontend(device):
    from .engine import FrontendOnly
    key = str(device)
    if key not in _FE:
        _FE[key] = FrontendOnly(device)
    return _FE[key]


@custom_op("sdfa::mel_frontend", mutates_args=(), device_types="cuda")
def mel_frontend(pcm: Tensor, clip_off: Tensor, clip_len: Tensor, frame_clip: Tensor, frame_start: Tensor, sample_rate: int) -> Tensor:
    assert pcm.dtype == torch.float32 and clip_off.dtype == torch.int64 and clip_len.dtype == torch.int64
    assert frame_clip.dtype == torch.int32 and frame_start.dtype == torch.int64
    return _frontend(pcm.device).mel_frontend_device(pcm.contiguous(), clip_off.contiguous(), clip_len.contiguous(),
                                                     frame_clip.contiguous(), frame_start.contiguous(), sample_rate)


@mel_frontend.register_fake
def _(pcm, clip_off, clip_len, frame_clip, frame_start, sample_rate):
    return pcm.new_empty((frame_clip.shape[0], 64, 128, 3))


# --------------------------------------------------------------------------------------------------- model
@custom_op("sdfa::encoder", mutates_args=(), device_types="cuda")
def encoder(audio_feat: Tensor, model: str) -> Tuple[Tensor, Tensor]:
    z, align = _model(model).encoder(audio_feat, want_align=True)
    return z, align


@encoder.register_fake
def _(audio_feat, model):
    n = audio_feat.shape[0]
    return audio_feat.new_empty((n, 512)), audio_feat.new_empty((n, 64))


@custom_op("sdfa::encoder_memory", mutates_args=(), device_types="cuda")
def encoder_memory(audio_feat: Tensor, model: str) -> Tuple[Tensor, Tensor, Tensor]:
    """sdfa_encoder_memory: the encoder's forward that also returns H, the BiLSTM output [N][64][512] the attention layer reads."""
    H, z, align = _model(model).encoder_memory(audio_feat)
    return H, z, align


@encoder_memory.register_fake
def _(audio_feat, model):
    n = audio_feat.shape[0]
    return audio_feat.new_empty((n, 64, 512)), audio_feat.new_empty((n, 512)), audio_feat.new_empty((n, 64))


@custom_op("sdfa::encoder_layer0", mutates_args=(), device_types="cuda")
def encoder_layer0(audio_feat: Tensor, model: str) -> Tensor:
    """sdfa_encoder_layer0: the encoder up to and including layer 0 of the BiLSTM, X1 [N][64][512], what the trained layer 1 reads."""
    return _model(model).encoder_layer0(audio_feat)


@encoder_layer0.register_fake
def _(audio_feat, model):
    return audio_feat.new_empty((audio_feat.shape[0], 64, 512))


@custom_op("sdfa::encoder_x0", mutates_args=(), device_types="cuda")
def encoder_x0(audio_feat: Tensor, model: str) -> Tensor:
    """sdfa_encoder_x0: the encoder up to the BiLSTM's input, X0 [N][64][256], what the trained layer 0 reads."""
    return _model(model).encoder_x0(audio_feat)


@encoder_x0.register_fake
def _(audio_feat, model):
    return audio_feat.new_empty((audio_feat.shape[0], 64, 256))


@custom_op("sdfa::encoder_conv", mutates_args=(), device_types="cuda")
def encoder_conv(audio_feat: Tensor, model: str) -> Tensor:
    """sdfa_encoder_conv: the encoder up to and including the conv stack, C [N][64][32][64], what the trained frequency LSTM reads."""
    return _model(model).encoder_conv(audio_feat)


@encoder_conv.register_fake
def _(audio_feat, model):
    return audio_feat.new_empty((audio_feat.shape[0], 64, 32, 64))


@custom_op("sdfa::encoder_shared", mutates_args=(), device_types="cuda")
def encoder_shared(audio_feat: Tensor, frame_clip: Tensor, frame_start: Tensor, hop: int, model: str) -> Tuple[Tensor, Tensor]:
    """sdfa_encoder_forward_shared: `audio_feat` must be what mel_frontend produced for exactly this frame table
    (frame_clip int32 [N], frame_start int64 [N], hop = int(0.008 * sr)); bitwise the result of sdfa::encoder."""
    assert frame_clip.dtype == torch.int32 and frame_start.dtype == torch.int64
    z, align = _model(model).encoder(audio_feat, want_align=True, frame_clip=frame_clip, frame_start=frame_start, hop=hop)
    return z, align


@encoder_shared.register_fake
def _(audio_feat, frame_clip, frame_start, hop, model):
    n = audio_feat.shape[0]
    return audio_feat.new_empty((n, 512)), audio_feat.new_empty((n, 64))


@custom_op("sdfa::regress", mutates_args=(), device_types="cuda")
def regress(z: Tensor, speaker_id: Tensor, model: str) -> Tensor:
    return _model(model).regress(z, speaker_id)[1]


@regress.register_fake
def _(z, speaker_id, model):
    return z.new_empty((z.shape[0], _model(model).out_dim))


@custom_op("sdfa::regress_into", mutates_args=("out",), device_types="cuda")
def regress_into(z: Tensor, speaker_id: Tensor, out: Tensor, model: str) -> None:
    """sdfa::regress writing into caller-owned rows (n, out_dim) -- the staging buffers of the pinned-output pipeline."""
    _model(model).regress(z, speaker_id, out=out, check_ids=False)


@regress_into.register_fake
def _(z, speaker_id, out, model):
    return None


@custom_op("sdfa::regress_coef", mutates_args=(), device_types="cuda")
def regress_coef(z: Tensor, speaker_id: Tensor, model: str) -> Tensor:
    return _model(model).regress(z, speaker_id, want_coef=True, want_out=False)[0]


@regress_coef.register_fake
def _(z, speaker_id, model):
    return z.new_empty((z.shape[0], _model(model).coef_dim))


# --------------------------------------------------------------------------------------------------- training objective
def _bases(model):
    """The PCA bases sdfa_amd.objective.attach_bases gave the model's engine (a KeyError that says so when it was never opted in)."""
    from .objective import bases_of
    return bases_of(_model(model))


@custom_op("sdfa::objective", mutates_args=(), device_types="cuda")
def objective(coef: Tensor, truth: Tensor, weight: Tensor, model: str) -> Tuple[Tensor, Tensor, Tensor]:
    """sdfa_objective on the model's PCA bases: (loss f32[4] = (ps, ms, pr, mr), rec f64[2B,4], grad f32[2,2B,Kc]); one pass."""
    from .objective import objective as _objective
    return _objective(coef.contiguous(), truth.contiguous(), weight.contiguous(), _bases(model))


@objective.register_fake
def _(coef, truth, weight, model):
    n, kc = coef.shape
    return coef.new_empty((4,)), coef.new_empty((n, 4), dtype=torch.float64), coef.new_empty((2, n, kc))


def combine_grads(grad_loss, grad, Ks):
    """sum_i grad_loss[i] * d loss_i / d coef from the operator's grad [2][N][Kc]: the p term's scale and rotat columns take
    grad_loss[0] and [2], the m term's [1] and [3]; a plain head (Ks = Kc) has no rotat columns.  Device arithmetic only."""
    kr = grad.shape[2] - Ks
    cp = torch.cat((grad_loss[0].expand(Ks), grad_loss[2].expand(kr)))
    cm = torch.cat((grad_loss[1].expand(Ks), grad_loss[3].expand(kr)))
    return grad[0] * cp + grad[1] * cm


def _objective_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])
    ctx.model = inputs[3]


def _objective_backward(ctx, grad_loss, grad_rec, grad_grad):
    (grad,) = ctx.saved_tensors
    if grad_loss is None:
        return None, None, None, None
    return combine_grads(grad_loss, grad, _bases(ctx.model).Ks), None, None, None


objective.register_autograd(_objective_backward, setup_context=_objective_setup)

# train_losses: the four losses alone, differentiable with respect to coef through sdfa::objective (whose forward has already
# computed and saved the gradients: backward is 2 x N x Kc elementwise work)
torch.library.define("sdfa::train_losses", "(Tensor coef, Tensor truth, Tensor weight, str model) -> Tensor")


@torch.library.impl("sdfa::train_losses", "CompositeImplicitAutograd")
def train_losses(coef, truth, weight, model):
    return torch.ops.sdfa.objective(coef, truth, weight, model)[0]


# --------------------------------------------------------------------------------------------------- head training
@custom_op("sdfa::head_train", mutates_args=(), device_types="cuda")
def head_train(z: Tensor, speaker_id: Tensor, trainer_key: str) -> Tensor:
    """sdfa_headtrain_forward of the HeadTrainer registered as `trainer_key` (sdfa_amd.headtrain.register_trainer): the
    training forward of the regressor head, z f32[N,512] -> coef f32[N,Kc].  The head's parameters live in the trainer, not in
    the graph: the backward needs z to require grad, runs sdfa_headtrain_backward, OVERWRITES the trainer's parameter
    gradients and returns dz."""
    from .headtrain import trainer_of
    return trainer_of(trainer_key).forward(z.contiguous(), speaker_id)


@head_train.register_fake
def _(z, speaker_id, trainer_key):
    from .headtrain import trainer_of
    return z.new_empty((z.shape[0], trainer_of(trainer_key).coef_dim))


def _head_train_setup(ctx, inputs, output):
    ctx.trainer_key = inputs[2]


def _head_train_backward(ctx, grad_coef):
    from .headtrain import trainer_of
    return trainer_of(ctx.trainer_key).backward(grad_coef.contiguous(), want_dz=True), None, None


head_train.register_autograd(_head_train_backward, setup_context=_head_train_setup)


# --------------------------------------------------------------------------------------------------- attention training
@custom_op("sdfa::attn_train", mutates_args=(), device_types="cuda")
def attn_train(H: Tensor, trainer_key: str) -> Tuple[Tensor, Tensor]:
    """sdfa_attntrain_forward of the AttnTrainer registered as `trainer_key` (sdfa_amd.attntrain.register_trainer): the training
    forward of the attention layer, H f32[N,64,512] -> (z f32[N,512], align f32[N,64]).  The layer's parameters live in the
    trainer, not in the graph: the backward needs H to require grad, runs sdfa_attntrain_backward, OVERWRITES the trainer's
    parameter gradients and returns dH -- or None when the trainer has want_dH = False (no trained layer below consumes dH).  align is not
    differentiable through this operator."""
    from .attntrain import trainer_of
    return trainer_of(trainer_key).forward(H.contiguous())


@attn_train.register_fake
def _(H, trainer_key):
    return H.new_empty((H.shape[0], 512)), H.new_empty((H.shape[0], 64))


def _attn_train_setup(ctx, inputs, output):
    ctx.trainer_key = inputs[1]
    ctx.set_materialize_grads(False)       # an unused align arrives as None, not as zeros: a real gradient for it is refused


def _attn_train_backward(ctx, grad_z, grad_align):
    from .attntrain import trainer_of
    if grad_align is not None:
        raise NotImplementedError("sdfa::attn_train: align is not differentiable through this operator (a gradient for align was given)")
    tr = trainer_of(ctx.trainer_key)
    return tr.backward(grad_z.contiguous(), want_dH=getattr(tr, "want_dH", True)), None


attn_train.register_autograd(_attn_train_backward, setup_context=_attn_train_setup)


# --------------------------------------------------------------------------------------------------- BiLSTM layer training
@custom_op("sdfa::lstm_train", mutates_args=(), device_types="cuda")
def lstm_train(X: Tensor, trainer_key: str) -> Tensor:
    """sdfa_lstmtrain_forward of the LstmTrainer registered as `trainer_key` (sdfa_amd.lstmtrain.register_trainer): the training
    forward of one bidirectional LSTM layer, X f32[N,64,I] -> Y f32[N,64,512].  The layer's parameters live in the trainer, not
    in the graph: the backward needs X to require grad, runs sdfa_lstmtrain_backward, OVERWRITES the trainer's parameter
    gradients and returns dX -- or None when the trainer has want_dX = False (the layer below is frozen)."""
    from .lstmtrain import trainer_of
    return trainer_of(trainer_key).forward(X.contiguous())


@lstm_train.register_fake
def _(X, trainer_key):
    return X.new_empty((X.shape[0], 64, 512))


def _lstm_train_setup(ctx, inputs, output):
    ctx.trainer_key = inputs[1]


def _lstm_train_backward(ctx, grad_Y):
    from .lstmtrain import trainer_of
    tr = trainer_of(ctx.trainer_key)
    return tr.backward(grad_Y.contiguous(), want_dX=getattr(tr, "want_dX", True)), None


lstm_train.register_autograd(_lstm_train_backward, setup_context=_lstm_train_setup)


# --------------------------------------------------------------------------------------------------- frequency LSTM training
@custom_op("sdfa::freq_train", mutates_args=(), device_types="cuda")
def freq_train(C: Tensor, trainer_key: str) -> Tensor:
    """sdfa_freqtrain_forward of the FreqTrainer registered as `trainer_key` (sdfa_amd.freqtrain.register_trainer): the training
    forward of the frequency LSTM and its projection, C f32[N,64,32,64] -> X0 f32[N,64,256].  The parameters live in the trainer,
    not in the graph: the backward needs C to require grad, runs sdfa_freqtrain_backward, OVERWRITES the trainer's parameter
    gradients and returns dC -- or None (a null d_dC) unless the trainer has want_dC = True, which a conv-stack trainer below it
    asks for."""
    from .freqtrain import trainer_of
    return trainer_of(trainer_key).forward(C.contiguous())


@freq_train.register_fake
def _(C, trainer_key):
    return C.new_empty((C.shape[0], 64, 256))


def _freq_train_setup(ctx, inputs, output):
    ctx.trainer_key = inputs[1]


def _freq_train_backward(ctx, grad_X0):
    from .freqtrain import trainer_of
    tr = trainer_of(ctx.trainer_key)
    return tr.backward(grad_X0.contiguous(), want_dC=getattr(tr, "want_dC", False)), None


freq_train.register_autograd(_freq_train_backward, setup_context=_freq_train_setup)


# --------------------------------------------------------------------------------------------------- conv stack training
@custom_op("sdfa::conv_train", mutates_args=(), device_types="cuda")
def conv_train(audio_feat: Tensor, trainer_key: str) -> Tensor:
    """sdfa_convtrain_forward of the ConvTrainer registered as `trainer_key` (sdfa_amd.convtrain.register_trainer): the training
    forward of the conv stack, audio_feat f32[N,64,128,3] -> C f32[N,64,32,64].  The parameters live in the trainer, not in the
    graph: the backward needs audio_feat to require grad (pass audio_feat.detach().requires_grad_(True)), runs
    sdfa_convtrain_backward, OVERWRITES the trainer's parameter gradients and returns None: the features are data."""
    from .convtrain import trainer_of
    return trainer_of(trainer_key).forward(audio_feat.contiguous())


@conv_train.register_fake
def _(audio_feat, trainer_key):
    return audio_feat.new_empty((audio_feat.shape[0], 64, 32, 64))


def _conv_train_setup(ctx, inputs, output):
    ctx.trainer_key = inputs[1]
    ctx.save_for_backward(inputs[0])


def _conv_train_backward(ctx, grad_C):
    from .convtrain import trainer_of
    trainer_of(ctx.trainer_key).backward(ctx.saved_tensors[0], grad_C.contiguous())
    return None, None


conv_train.register_autograd(_conv_train_backward, setup_context=_conv_train_setup)


class TraceableSpeechDrivenAnimation(torch.nn.Module):
    """SpeechDrivenAnimation.forward (speech_anime/model/model.py:28-45) as a graph of sdfa ops: what jit_trace traces.
    forward(audio_feat (N,64,128,3), speaker_id (N,)) -> ((scale (N,1,9976,6), rotat (N,1,9976,3)), z (N,1,512)) for the
    dgrad head, (pred (N,1,15069), z) for the offsets head."""

    def __init__(self, model_key, head):
        super().__init__()
        self.model_key, self.head = str(model_key), head

    def forward(self, audio_feat, speaker_id):
        z, _ = torch.ops.sdfa.encoder(audio_feat, self.model_key)
        out = torch.ops.sdfa.regress(z, speaker_id, self.model_key)
        n = audio_feat.shape[0]
        z_audio = z.view(n, 1, 512)
        if self.head == "dgrad":
            tri = out.view(n, 1, -1, 9)
            return (tri[..., :6], tri[..., 6:]), z_audio
        return out.view(n, 1, -1), z_audio
