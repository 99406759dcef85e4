"""Fine-tuning the encoder's frequency LSTM on the GPU: host side of sdfa_freqtrain* in libsdfa_hip.so (csrc/freqtrain.hip and
api_freqtrain.cpp, C ABI in include/sdfa_freqtrain.h).  The reference's FreqLstm (speech_anime/layers/freq_lstm.py, layer 6 of the
audio encoder) -- torch.nn.LSTM(64, 128, bias=True, bidirectional=True) along the 32 frequency bins of every column, then
Linear(8192, 256) -- as a training forward that keeps the gates, the cell state and the hidden states, back-propagation through
the 32 steps down to dC, and torch.optim.Adam(lr=1e-4, weight_decay=0).  It consumes the dX that
sdfa_amd.lstmtrain.LstmTrainer(layer=0) produces.  The contract is written down in the header and in DESIGN.md section 21.

FreqTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are stream-ordered
and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream
from ._trainer import PARAM, GRAD, EXP_AVG, EXP_AVG_SQ, Registry, Trainer

ABI_VERSION = 1          # include/sdfa_freqtrain.h SDFA_FREQTRAIN_ABI_VERSION this binding was written against
COLUMNS, STEPS, IN, HIDDEN, GATES, OUT, TILE_COLUMNS, BLOCK_FRAMES, MAX_FRAMES = 64, 32, 64, 128, 512, 256, 32, 8, 2048
FEATURES = STEPS * 2 * HIDDEN      # of HF, the projection's input: 8,192
LAUNCHES = dict(forward=4, backward=4, adam=1)
PREFIX = "_audio_encoder._layers.6."

_p, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_freqtrain_abi_version": (C.c_int, []),
    "sdfa_freqtrain_create": (_p, []),
    "sdfa_freqtrain_destroy": (None, [_p]),
    "sdfa_freqtrain_set_tensor": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_freqtrain_finalize": (C.c_int, [_p, _p]),
    "sdfa_freqtrain_numel": (_i64, [_p]),
    "sdfa_freqtrain_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_freqtrain_forward": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_freqtrain_backward": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_freqtrain_adam": (C.c_int, [_p, _f64, _f64, _f64, _f64, _p]),
    "sdfa_freqtrain_zero_grad": (C.c_int, [_p, _p]),
    "sdfa_freqtrain_get_tensor": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_freqtrain_set_grad": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_freqtrain_set_state": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_freqtrain_step_count": (_i64, [_p]),
    "sdfa_freqtrain_set_step_count": (C.c_int, [_p, _i64]),
    "sdfa_encoder_conv": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
}


bind(SYMBOLS, "sdfa_freqtrain_abi_version", ABI_VERSION, "freqtrain")


def tensor_shapes():
    """{tensor name without "_model.": shape} of the ten trainable tensors, as the reference's state dict has them, in the order
    of the device's flat buffers."""
    out = {}
    for kind, shape in (("weight_ih", (GATES, IN)), ("weight_hh", (GATES, HIDDEN)), ("bias_ih", (GATES,)), ("bias_hh", (GATES,))):
        for suffix in ("", "_reverse"):
            out[f"{PREFIX}_lstm.{kind}_l0{suffix}"] = shape
    out[f"{PREFIX}_proj.weight"] = (OUT, FEATURES)
    out[f"{PREFIX}_proj.bias"] = (OUT,)
    return out


class FreqTrainer(Trainer):
    """A checkpoint's frequency LSTM and its projection with their gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; every other tensor is ignored.
    forward(C) -> X0 [N][64][256] for C float32 cuda [N][64][32][64] (torch.ops.sdfa.encoder_conv's output);  backward(dX0,
    want_dC) -> dC [N][64][32][64] | None, gradients OVERWRITTEN in the trainer, once per forward (it consumes the kept gates);
    step() is one torch.optim.Adam step;  grads() / parameters() read back under the reference's names;  state_dict() /
    load_state_dict() carry parameters, both moments and the step count, so a fit can resume."""

    ABI = "freqtrain"

    def __init__(self, state_dict, device=None, want_dC=False, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        self.want_dC = bool(want_dC)          # what the backward of torch.ops.sdfa.freq_train returns for C
        super().__init__(state_dict, tensor_shapes(), (), lr, betas, eps, device)
        self._C = None

    def forward(self, Cin):
        """C float32 cuda [N][64][32][64] -> X0 float32 [N][64][256].  C is kept (not copied) for the backward."""
        assert torch.is_tensor(Cin) and Cin.is_cuda and Cin.dtype == torch.float32, "sdfa_amd.freqtrain takes cuda tensors: there is no CPU path"
        assert Cin.dim() == 4 and tuple(Cin.shape[1:]) == (COLUMNS, STEPS, IN), tuple(Cin.shape)
        Cin = Cin.detach().contiguous()
        N = int(Cin.shape[0])
        with torch.cuda.device(Cin.device):
            ws = self._workspace(N, Cin.device)
            X0 = torch.empty(N, COLUMNS, OUT, dtype=torch.float32, device=Cin.device)
            check(lib.sdfa_freqtrain_forward(self._h, _ptr(Cin), N, _ptr(X0), _ptr(ws), ws.numel(), _stream()))
        self._C = Cin
        return X0

    def backward(self, dX0, want_dC=False):
        """dX0 float32 cuda [N][64][256] for the N of the last forward -> dC [N][64][32][64] (None without want_dC)."""
        assert torch.is_tensor(dX0) and dX0.is_cuda and dX0.dtype == torch.float32
        dX0 = dX0.detach().contiguous()
        assert dX0.dim() == 3 and tuple(dX0.shape[1:]) == (COLUMNS, OUT), tuple(dX0.shape)
        N = int(dX0.shape[0])
        with torch.cuda.device(dX0.device):
            kept = self._C is not None and self._C.shape[0] == N
            Cin = self._C if kept else torch.empty(max(N, 1), COLUMNS, STEPS, IN, dtype=torch.float32, device=dX0.device)
            dC = torch.empty(N, COLUMNS, STEPS, IN, dtype=torch.float32, device=dX0.device) if want_dC else None
            ws = self._ws if self._ws is not None else torch.empty(256, dtype=torch.uint8, device=dX0.device)
            check(lib.sdfa_freqtrain_backward(self._h, _ptr(Cin), _ptr(dX0), N, _ptr(dC) if want_dC else None, _ptr(ws), ws.numel(), _stream()))
        return dC

    def _forget(self):
        self._C = None

    def freq_state_dict(self, prefix="_model."):
        """The tuned module as torch tensors under the reference's names."""
        return self.tuned_state_dict(prefix)


# trainers the custom op torch.ops.sdfa.freq_train finds by key
_REGISTRY = Registry("freq", "frequency LSTM")
register_trainer, trainer_of = _REGISTRY.register, _REGISTRY.find
