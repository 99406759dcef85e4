"""Fine-tuning a layer of the encoder's BiLSTM on the GPU: host side of sdfa_lstmtrain* in libsdfa_hip.so (csrc/lstmtrain.hip and
api_lstmtrain.cpp, C ABI in include/sdfa_lstmtrain.h).  One layer of the reference's torch.nn.LSTM(256, 256, num_layers=2,
bias=False, bidirectional=True) (speech_anime/layers/rnn.py) as a training forward that keeps the gates and the cell state,
back-propagation through time down to dX, and torch.optim.Adam(lr=1e-4, weight_decay=0).  Layer 1 consumes the dH that
sdfa_amd.attntrain produces.  The contract is written down in the header and in DESIGN.md section 18.

LstmTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are stream-ordered
and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream
from ._trainer import PARAM, GRAD, EXP_AVG, EXP_AVG_SQ, Registry, Trainer

ABI_VERSION = 1          # include/sdfa_lstmtrain.h SDFA_LSTMTRAIN_ABI_VERSION this binding was written against
STEPS, HIDDEN, GATES, OUT, TILE_FRAMES, BLOCK_FRAMES, MAX_FRAMES = 64, 256, 1024, 512, 32, 32, 3072
IN_DIM = {0: 256, 1: 512}
LAUNCHES = dict(forward=3, backward=3, adam=1)
PREFIX = "_audio_encoder._layers.9."

_p, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_lstmtrain_abi_version": (C.c_int, []),
    "sdfa_lstmtrain_create": (_p, [C.c_int]),
    "sdfa_lstmtrain_destroy": (None, [_p]),
    "sdfa_lstmtrain_set_tensor": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_lstmtrain_finalize": (C.c_int, [_p, _p]),
    "sdfa_lstmtrain_numel": (_i64, [_p]),
    "sdfa_lstmtrain_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_lstmtrain_forward": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_lstmtrain_backward": (C.c_int, [_p, _p, _p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_lstmtrain_adam": (C.c_int, [_p, _f64, _f64, _f64, _f64, _p]),
    "sdfa_lstmtrain_zero_grad": (C.c_int, [_p, _p]),
    "sdfa_lstmtrain_get_tensor": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_lstmtrain_set_grad": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_lstmtrain_set_state": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_lstmtrain_step_count": (_i64, [_p]),
    "sdfa_lstmtrain_set_step_count": (C.c_int, [_p, _i64]),
    "sdfa_encoder_layer0": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
}


bind(SYMBOLS, "sdfa_lstmtrain_abi_version", ABI_VERSION, "lstmtrain")


def tensor_shapes(layer):
    """{tensor name without "_model.": shape} of one layer's trainable tensors, as the reference's state dict has them."""
    assert layer in IN_DIM, f"the encoder's BiLSTM has layers 0 and 1, not {layer!r}"
    out = {}
    for kind, width in (("ih", IN_DIM[layer]), ("hh", HIDDEN)):
        for suffix in ("", "_reverse"):
            out[f"{PREFIX}weight_{kind}_l{layer}{suffix}"] = (GATES, width)
    return out


class LstmTrainer(Trainer):
    """One layer of a checkpoint's BiLSTM with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; every other tensor is ignored.
    forward(X) -> Y [N][64][512] for X float32 cuda [N][64][I], I = 256 (layer 0) or 512 (layer 1);  backward(dY, want_dX=True)
    -> dX [N][64][I] | None, gradients OVERWRITTEN in the trainer, once per forward (it consumes the kept gates);  step() is one
    torch.optim.Adam step;  grads() / parameters() read back under the reference's names;  state_dict() / load_state_dict() carry
    parameters, both moments and the step count, so a fit can resume."""

    ABI = "lstmtrain"

    def __init__(self, state_dict, layer=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None, want_dX=True):
        self.layer = int(layer)
        self.want_dX = bool(want_dX)          # what the backward of torch.ops.sdfa.lstm_train returns for X
        shapes = tensor_shapes(self.layer)
        self.in_dim = IN_DIM[self.layer]
        super().__init__(state_dict, shapes, (self.in_dim,), lr, betas, eps, device)
        self._X = self._Y = None

    def forward(self, X):
        """X float32 cuda [N][64][I] -> Y float32 [N][64][512].  X and Y are kept (not copied) for the backward."""
        assert torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float32, "sdfa_amd.lstmtrain takes cuda tensors: there is no CPU path"
        assert X.dim() == 3 and tuple(X.shape[1:]) == (STEPS, self.in_dim), tuple(X.shape)
        X = X.detach().contiguous()
        N = int(X.shape[0])
        with torch.cuda.device(X.device):
            ws = self._workspace(N, X.device)
            Y = torch.empty(N, STEPS, OUT, dtype=torch.float32, device=X.device)
            check(lib.sdfa_lstmtrain_forward(self._h, _ptr(X), N, _ptr(Y), _ptr(ws), ws.numel(), _stream()))
        self._X, self._Y = X, Y
        return Y

    def backward(self, dY, want_dX=True):
        """dY float32 cuda [N][64][512] for the N of the last forward -> dX [N][64][I] (None without want_dX)."""
        assert torch.is_tensor(dY) and dY.is_cuda and dY.dtype == torch.float32
        dY = dY.detach().contiguous()
        assert dY.dim() == 3 and tuple(dY.shape[1:]) == (STEPS, OUT), tuple(dY.shape)
        N = int(dY.shape[0])
        with torch.cuda.device(dY.device):
            kept = self._X is not None and self._X.shape[0] == N
            X = self._X if kept else torch.empty(max(N, 1), STEPS, self.in_dim, dtype=torch.float32, device=dY.device)
            Y = self._Y if kept else torch.empty(max(N, 1), STEPS, OUT, dtype=torch.float32, device=dY.device)
            dX = torch.empty(N, STEPS, self.in_dim, dtype=torch.float32, device=dY.device) if want_dX else None
            ws = self._ws if self._ws is not None else torch.empty(256, dtype=torch.uint8, device=dY.device)
            check(lib.sdfa_lstmtrain_backward(self._h, _ptr(X), _ptr(Y), _ptr(dY), N, _ptr(dX) if want_dX else None, _ptr(ws), ws.numel(), _stream()))
        return dX

    def _forget(self):
        self._X = self._Y = None

    def lstm_state_dict(self, prefix="_model."):
        """The tuned layer as torch tensors under the reference's names."""
        return self.tuned_state_dict(prefix)

    def _state_extra(self):
        return dict(layer=self.layer)

    def load_state_dict(self, state):
        assert int(state.get("layer", self.layer)) == self.layer, (state.get("layer"), self.layer)
        return super().load_state_dict(state)


# trainers the custom op torch.ops.sdfa.lstm_train finds by key
_REGISTRY = Registry("lstm", "BiLSTM")
register_trainer, trainer_of = _REGISTRY.register, _REGISTRY.find
