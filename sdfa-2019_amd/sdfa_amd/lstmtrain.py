"""Fine-tuning a layer of the encoder's BiLSTM on the GPU: host side of sdfa_lstmtrain* in libsdfa_hip.so (csrc/lstmtrain.hip and
api_lstmtrain.cpp, C ABI in include/sdfa_lstmtrain.h).  One layer of the reference's torch.nn.LSTM(256, 256, num_layers=2,
bias=False, bidirectional=True) (speech_anime/layers/rnn.py) as a training forward that keeps the gates and the cell state,
back-propagation through time down to dX, and torch.optim.Adam(lr=1e-4, weight_decay=0).  Layer 1 consumes the dH that
sdfa_amd.attntrain produces.  The contract is written down in the header and in DESIGN.md section 18.

LstmTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are stream-ordered
and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import itertools
import weakref

import numpy as np
import torch

from ._lib import lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_lstmtrain.h SDFA_LSTMTRAIN_ABI_VERSION this binding was written against
PARAM, GRAD, EXP_AVG, EXP_AVG_SQ = 0, 1, 2, 3
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


def _bind():
    stale = "libsdfa_hip.so is a stale build (%s): rebuild it with `make -C sdfa-2019_amd/csrc`.  There is no CPU fallback."
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(stale % f"symbol {name} is not exported") from None
        fn.restype = res
        fn.argtypes = args
    have = int(lib.sdfa_lstmtrain_abi_version())
    if have != ABI_VERSION:
        raise ImportError(stale % f"lstmtrain ABI version {have}, this binding needs {ABI_VERSION}")


_bind()


def tensor_shapes(layer):
    """{tensor name without "_model.": shape} of one layer's trainable tensors, as the reference's state dict has them."""
    assert layer in IN_DIM, f"the encoder's BiLSTM has layers 0 and 1, not {layer!r}"
    out = {}
    for kind, width in (("ih", IN_DIM[layer]), ("hh", HIDDEN)):
        for suffix in ("", "_reverse"):
            out[f"{PREFIX}weight_{kind}_l{layer}{suffix}"] = (GATES, width)
    return out


def _strip(name):
    return name[len("_model."):] if name.startswith("_model.") else name


def _f32(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v, np.float32))


class LstmTrainer:
    """One layer of a checkpoint's BiLSTM with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; every other tensor is ignored.
    forward(X) -> Y [N][64][512] for X float32 cuda [N][64][I], I = 256 (layer 0) or 512 (layer 1);  backward(dY, want_dX=True)
    -> dX [N][64][I] | None, gradients OVERWRITTEN in the trainer, once per forward (it consumes the kept gates);  step() is one
    torch.optim.Adam step;  grads() / parameters() read back under the reference's names;  state_dict() / load_state_dict() carry
    parameters, both moments and the step count, so a fit can resume."""

    def __init__(self, state_dict, layer=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None, want_dX=True):
        self.layer = int(layer)
        self.want_dX = bool(want_dX)          # what the backward of torch.ops.sdfa.lstm_train returns for X
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.shapes = tensor_shapes(self.layer)
        self.in_dim = IN_DIM[self.layer]
        self._h = None
        h = lib.sdfa_lstmtrain_create(self.in_dim)
        if not h:
            check(-1)
        self._h = C.c_void_p(h)
        self._finalizer = weakref.finalize(self, lib.sdfa_lstmtrain_destroy, self._h)
        given = {_strip(k): v for k, v in state_dict.items()}
        for name in self.shapes:
            if name not in given:
                continue                                     # finalize names the first missing tensor
            a = _f32(given[name])
            check(lib.sdfa_lstmtrain_set_tensor(self._h, name.encode(), a.ctypes.data, a.size))
        with torch.cuda.device(self.device):
            check(lib.sdfa_lstmtrain_finalize(self._h, _stream()))
        self.numel = int(check(lib.sdfa_lstmtrain_numel(self._h)))
        self._ws = None
        self._X = self._Y = None

    # ------------------------------------------------------------------------------------------------ the step
    def workspace_bytes(self, frames):
        return int(check(lib.sdfa_lstmtrain_workspace_bytes(self._h, int(frames))))

    def forward(self, X):
        """X float32 cuda [N][64][I] -> Y float32 [N][64][512].  X and Y are kept (not copied) for the backward."""
        assert torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float32, "sdfa_amd.lstmtrain takes cuda tensors: there is no CPU path"
        assert X.dim() == 3 and tuple(X.shape[1:]) == (STEPS, self.in_dim), tuple(X.shape)
        X = X.detach().contiguous()
        N = int(X.shape[0])
        with torch.cuda.device(X.device):
            need = self.workspace_bytes(N)
            if self._ws is None or self._ws.numel() < need or self._ws.device != X.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=X.device)
            Y = torch.empty(N, STEPS, OUT, dtype=torch.float32, device=X.device)
            check(lib.sdfa_lstmtrain_forward(self._h, _ptr(X), N, _ptr(Y), _ptr(self._ws), self._ws.numel(), _stream()))
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

    def step(self):
        with torch.cuda.device(self.device):
            check(lib.sdfa_lstmtrain_adam(self._h, self.lr, self.betas[0], self.betas[1], self.eps, _stream()))
        self._X = self._Y = None

    def zero_grad(self):
        with torch.cuda.device(self.device):
            check(lib.sdfa_lstmtrain_zero_grad(self._h, _stream()))

    # ------------------------------------------------------------------------------------------------ access
    @property
    def step_count(self):
        return int(check(lib.sdfa_lstmtrain_step_count(self._h)))

    def _read(self, what):
        out = {}
        with torch.cuda.device(self.device):
            for name, shape in self.shapes.items():
                a = np.empty(shape, np.float32)
                check(lib.sdfa_lstmtrain_get_tensor(self._h, name.encode(), what, a.ctypes.data, a.size))
                out[name] = a
        return out

    def _write(self, what, tensors):
        with torch.cuda.device(self.device):
            for name, v in tensors.items():
                a = _f32(v)
                check(lib.sdfa_lstmtrain_set_state(self._h, _strip(name).encode(), what, a.ctypes.data, a.size))

    def parameters(self):
        """{name without "_model.": float32 array} read back from the device."""
        return self._read(PARAM)

    def grads(self):
        return self._read(GRAD)

    def moments(self):
        return self._read(EXP_AVG), self._read(EXP_AVG_SQ)

    def set_grads(self, grads):
        self._write(GRAD, grads)

    def lstm_state_dict(self, prefix="_model."):
        """The tuned layer as torch tensors under the reference's names."""
        return {prefix + k: torch.from_numpy(v) for k, v in self.parameters().items()}

    def state_dict(self):
        m, v = self.moments()
        return dict(params=self.parameters(), exp_avg=m, exp_avg_sq=v, step=self.step_count, lr=self.lr, betas=self.betas, eps=self.eps,
                    layer=self.layer)

    def load_state_dict(self, state):
        assert int(state.get("layer", self.layer)) == self.layer, (state.get("layer"), self.layer)
        self._write(PARAM, state["params"])
        self._write(EXP_AVG, state["exp_avg"])
        self._write(EXP_AVG_SQ, state["exp_avg_sq"])
        check(lib.sdfa_lstmtrain_set_step_count(self._h, int(state["step"])))
        self.lr, self.betas, self.eps = float(state["lr"]), tuple(float(b) for b in state["betas"]), float(state["eps"])
        self._X = self._Y = None
        return self


# trainers the custom op torch.ops.sdfa.lstm_train finds by key; weak, as the model registry of sdfa_amd.ops is
_TRAINERS = weakref.WeakValueDictionary()
_ANON = itertools.count(1)


def register_trainer(trainer, key=None):
    key = f"sdfa-lstm-trainer-{next(_ANON)}" if key is None else str(key)
    _TRAINERS[key] = trainer
    return key


def trainer_of(key):
    try:
        return _TRAINERS[key]
    except KeyError:
        raise KeyError(f"sdfa: no BiLSTM trainer registered as {key!r} (sdfa_amd.lstmtrain.register_trainer)") from None
