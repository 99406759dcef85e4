"""Fine-tuning the encoder's conv stack on the GPU: host side of sdfa_convtrain* in libsdfa_hip.so (csrc/convtrain.hip and
api_convtrain.cpp, C ABI in include/sdfa_convtrain.h).  Layers 1, 3 and 5 of the reference's audio encoder
(speech_anime/config/model/dgrad.py:62-64) -- three weight-normed convolutions along frequency, each followed by LeakyReLU(0.2)
and BatchNorm, with two max-pools -- as a training forward that keeps the pre-activations, the backward from dC to the 15
parameter gradients, and torch.optim.Adam(lr=1e-4, weight_decay=0).  It consumes the dC that
sdfa_amd.freqtrain.FreqTrainer(want_dC=True) produces.  BatchNorm runs with its running statistics (the inference form): the
reference's train() mode, batch statistics and moving running ones, is not built.  The contract is written down in the header and
in DESIGN.md section 22.

ConvTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are stream-ordered
and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

import numpy as np
import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream
from ._trainer import PARAM, GRAD, EXP_AVG, EXP_AVG_SQ, Registry, Trainer

ABI_VERSION = 1          # include/sdfa_convtrain.h SDFA_CONVTRAIN_ABI_VERSION this binding was written against
COLUMNS, BINS, IN, OUT_BINS, OUT, NUMEL, BLOCK_FRAMES, MAX_FRAMES = 64, 128, 3, 32, 64, 11168, 8, 2048
BN_EPS = 1e-3
LAYERS = ((1, 32, 3, 3), (3, 64, 32, 3), (5, 64, 64, 1))        # (index in _audio_encoder._layers, co, ci, kf)
LAUNCHES = dict(forward=4, backward=6, adam=1)
PREFIX = "_audio_encoder._layers."

_p, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_convtrain_abi_version": (C.c_int, []),
    "sdfa_convtrain_create": (_p, []),
    "sdfa_convtrain_destroy": (None, [_p]),
    "sdfa_convtrain_set_tensor": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_convtrain_finalize": (C.c_int, [_p, _p]),
    "sdfa_convtrain_numel": (_i64, [_p]),
    "sdfa_convtrain_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_convtrain_forward": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_convtrain_backward": (C.c_int, [_p, _p, _p, _i64, _p, _i64, _p]),
    "sdfa_convtrain_adam": (C.c_int, [_p, _f64, _f64, _f64, _f64, _p]),
    "sdfa_convtrain_zero_grad": (C.c_int, [_p, _p]),
    "sdfa_convtrain_get_tensor": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_convtrain_set_grad": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_convtrain_set_state": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_convtrain_step_count": (_i64, [_p]),
    "sdfa_convtrain_set_step_count": (C.c_int, [_p, _i64]),
}


bind(SYMBOLS, "sdfa_convtrain_abi_version", ABI_VERSION, "convtrain")


def tensor_shapes():
    """{tensor name without "_model.": shape} of the 15 trainable tensors, as the reference's state dict has them, in the order of
    the device's flat buffers."""
    out = {}
    for L, co, ci, kf in LAYERS:
        n = f"{PREFIX}{L}."
        out[n + "weight_g"] = (co, 1, 1, 1)
        out[n + "weight_v"] = (co, ci, kf, 1)
        out[n + "bias"] = (co,)
        out[n + "_ext_post_bn.weight"] = (co,)
        out[n + "_ext_post_bn.bias"] = (co,)
    return out


def constant_shapes():
    """{name: shape} of the six running statistics: required, uploaded once, never stepped."""
    return {f"{PREFIX}{L}._ext_post_bn.running_{k}": (co,) for L, co, _, _ in LAYERS for k in ("mean", "var")}


class ConvTrainer(Trainer):
    """A checkpoint's conv stack with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; every other tensor is ignored.
    forward(audio_feat) -> C [N][64][32][64] for audio_feat float32 cuda [N][64][128][3] (train_batch's);  backward(audio_feat, dC)
    leaves the gradients in the trainer, OVERWRITTEN, once per forward (it consumes the kept pre-activations);  step() is one
    torch.optim.Adam step;  grads() / parameters() read back under the reference's names;  state_dict() / load_state_dict() carry
    parameters, both moments and the step count, so a fit can resume, and the running statistics, which load_state_dict compares
    with this trainer's and refuses by name when they differ.  BatchNorm's running statistics are running_stats()."""

    ABI = "convtrain"

    def __init__(self, state_dict, device=None, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(state_dict, tensor_shapes(), (), lr, betas, eps, device, constants=constant_shapes())

    def running_stats(self):
        """{name without "_model.": float32 array} of the running statistics, read back from the device."""
        out = {}
        with torch.cuda.device(self.device):
            for name, shape in self.constants.items():
                a = np.empty(shape, np.float32)
                check(self._fn("get_tensor")(self._h, name.encode(), PARAM, a.ctypes.data, a.size))
                out[name] = a
        return out

    @staticmethod
    def _feat_of(audio_feat):
        assert torch.is_tensor(audio_feat) and audio_feat.is_cuda and audio_feat.dtype == torch.float32, \
            "sdfa_amd.convtrain takes cuda tensors: there is no CPU path"
        assert audio_feat.dim() == 4 and tuple(audio_feat.shape[1:]) == (COLUMNS, BINS, IN), tuple(audio_feat.shape)
        return audio_feat.detach().contiguous()

    def forward(self, audio_feat):
        """audio_feat float32 cuda [N][64][128][3] -> C float32 [N][64][32][64]."""
        feat = self._feat_of(audio_feat)
        N = int(feat.shape[0])
        with torch.cuda.device(feat.device):
            ws = self._workspace(N, feat.device)
            Cout = torch.empty(N, COLUMNS, OUT_BINS, OUT, dtype=torch.float32, device=feat.device)
            check(lib.sdfa_convtrain_forward(self._h, _ptr(feat), N, _ptr(Cout), _ptr(ws), ws.numel(), _stream()))
        return Cout

    def backward(self, audio_feat, dC):
        """The features of the last forward and dC float32 cuda [N][64][32][64]: the gradients stay in the trainer."""
        feat = self._feat_of(audio_feat)
        assert torch.is_tensor(dC) and dC.is_cuda and dC.dtype == torch.float32
        dC = dC.detach().contiguous()
        N = int(feat.shape[0])
        assert tuple(dC.shape) == (N, COLUMNS, OUT_BINS, OUT), tuple(dC.shape)
        with torch.cuda.device(feat.device):
            ws = self._ws if self._ws is not None else torch.empty(256, dtype=torch.uint8, device=feat.device)
            check(lib.sdfa_convtrain_backward(self._h, _ptr(feat), _ptr(dC), N, _ptr(ws), ws.numel(), _stream()))

    def _state_extra(self):
        return dict(constants=self.running_stats())

    def load_state_dict(self, state):
        """As Trainer.load_state_dict; the running statistics the state was taken with must be this trainer's, bit for bit: they
        are part of the function that was trained and no call can change them."""
        mine = self.running_stats()
        theirs = state.get("constants")
        if theirs is None or set(theirs) != set(mine):
            raise ValueError("conv-stack training state: it carries no running statistics (\"constants\"), or other ones than this trainer holds")
        for name, a in mine.items():
            b = np.ascontiguousarray(np.asarray(theirs[name], np.float32))
            if b.shape != a.shape or not (a.view(np.uint32) == b.view(np.uint32)).all():
                raise ValueError(f"conv-stack training state: taken with another \"{name}\" than this trainer was enabled with")
        return super().load_state_dict(state)

    def conv_state_dict(self, prefix="_model."):
        """The 15 tuned tensors as torch tensors under the reference's names; the running statistics are not in it."""
        return self.tuned_state_dict(prefix)


# trainers the custom op torch.ops.sdfa.conv_train finds by key
_REGISTRY = Registry("conv", "conv stack")
register_trainer, trainer_of = _REGISTRY.register, _REGISTRY.find
