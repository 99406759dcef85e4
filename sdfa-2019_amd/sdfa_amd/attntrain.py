"""Fine-tuning the attention layer on the GPU: host side of sdfa_attntrain* in libsdfa_hip.so (csrc/attntrain.hip and
api_attntrain.cpp, C ABI in include/sdfa_attntrain.h).  The reference's Bahdanau attention (speech_anime/layers/attentions.py,
("attn", "bah", 512, 128, 2), called with query = H[:, 31:34] and key = H in training mode) as a training forward, the analytic
backward down to dH, and torch.optim.Adam(lr=1e-4, weight_decay=0).  It consumes the dz that sdfa_amd.headtrain produces.  The
contract is written down in the header and in DESIGN.md section 17.

AttnTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are stream-ordered
and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import itertools
import weakref

import numpy as np
import torch

from ._lib import lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_attntrain.h SDFA_ATTNTRAIN_ABI_VERSION this binding was written against
PARAM, GRAD, EXP_AVG, EXP_AVG_SQ = 0, 1, 2, 3
STEPS, DIM, ATT, BLOCK_FRAMES, MAX_FRAMES = 64, 512, 128, 16, 32768
LAUNCHES = dict(forward=3, backward=5, backward_without_dH=4, adam=1)
PREFIX = "_audio_encoder._layers.10."
SHAPES = {
    PREFIX + "_conv_query.weight": (512, 512, 3),
    PREFIX + "proj_qry.weight": (128, 512),
    PREFIX + "proj_key.weight": (128, 512),
    PREFIX + "v.weight": (1, 128),
    PREFIX + "b": (1, 1, 128),
}

_p, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_attntrain_abi_version": (C.c_int, []),
    "sdfa_attntrain_create": (_p, []),
    "sdfa_attntrain_destroy": (None, [_p]),
    "sdfa_attntrain_set_tensor": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_attntrain_finalize": (C.c_int, [_p, _p]),
    "sdfa_attntrain_numel": (_i64, [_p]),
    "sdfa_attntrain_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_attntrain_forward": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, _p]),
    "sdfa_attntrain_backward": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_attntrain_adam": (C.c_int, [_p, _f64, _f64, _f64, _f64, _p]),
    "sdfa_attntrain_zero_grad": (C.c_int, [_p, _p]),
    "sdfa_attntrain_get_tensor": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_attntrain_set_grad": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_attntrain_set_state": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_attntrain_step_count": (_i64, [_p]),
    "sdfa_attntrain_set_step_count": (C.c_int, [_p, _i64]),
    "sdfa_encoder_memory": (C.c_int, [_p, _p, _i64, _p, _p, _p, _p, _i64, _p]),
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
    have = int(lib.sdfa_attntrain_abi_version())
    if have != ABI_VERSION:
        raise ImportError(stale % f"attntrain ABI version {have}, this binding needs {ABI_VERSION}")


_bind()


def tensor_shapes():
    """{tensor name without "_model.": shape} of the layer's trainable tensors, as the reference's state dict has them."""
    return dict(SHAPES)


def _strip(name):
    return name[len("_model."):] if name.startswith("_model.") else name


def _f32(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v, np.float32))


class AttnTrainer:
    """The attention layer of a checkpoint with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; every other tensor is ignored.
    forward(H) -> (z [N][512], align [N][64]) for H float32 cuda [N][64][512];  backward(dz, want_dH=True) -> dH [N][64][512] |
    None, gradients OVERWRITTEN in the trainer;  step() is one torch.optim.Adam step;  grads() / parameters() read back under the
    reference's names;  state_dict() / load_state_dict() carry parameters, both moments and the step count, so a fit can resume."""

    def __init__(self, state_dict, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None, want_dH=True):
        self.want_dH = bool(want_dH)          # what the backward of torch.ops.sdfa.attn_train returns for H
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.shapes = tensor_shapes()
        self._h = None
        h = lib.sdfa_attntrain_create()
        if not h:
            check(-1)
        self._h = C.c_void_p(h)
        self._finalizer = weakref.finalize(self, lib.sdfa_attntrain_destroy, self._h)
        given = {_strip(k): v for k, v in state_dict.items()}
        for name in self.shapes:
            if name not in given:
                continue                                     # finalize names the first missing tensor
            a = _f32(given[name])
            check(lib.sdfa_attntrain_set_tensor(self._h, name.encode(), a.ctypes.data, a.size))
        with torch.cuda.device(self.device):
            check(lib.sdfa_attntrain_finalize(self._h, _stream()))
        self.numel = int(check(lib.sdfa_attntrain_numel(self._h)))
        self._ws = None
        self._H = None

    # ------------------------------------------------------------------------------------------------ the step
    def workspace_bytes(self, frames):
        return int(check(lib.sdfa_attntrain_workspace_bytes(self._h, int(frames))))

    def forward(self, H):
        """H float32 cuda [N][64][512] -> (z float32 [N][512], align float32 [N][64]).  H is kept (not copied) for the backward."""
        assert torch.is_tensor(H) and H.is_cuda and H.dtype == torch.float32, "sdfa_amd.attntrain takes cuda tensors: there is no CPU path"
        assert H.dim() == 3 and tuple(H.shape[1:]) == (STEPS, DIM), tuple(H.shape)
        H = H.detach().contiguous()
        N = int(H.shape[0])
        with torch.cuda.device(H.device):
            need = self.workspace_bytes(N)
            if self._ws is None or self._ws.numel() < need or self._ws.device != H.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=H.device)
            z = torch.empty(N, DIM, dtype=torch.float32, device=H.device)
            align = torch.empty(N, STEPS, dtype=torch.float32, device=H.device)
            check(lib.sdfa_attntrain_forward(self._h, _ptr(H), N, _ptr(z), _ptr(align), _ptr(self._ws), self._ws.numel(), _stream()))
        self._H = H
        return z, align

    def backward(self, dz, want_dH=True):
        """dz float32 cuda [N][512] for the N of the last forward -> dH [N][64][512] (None without want_dH)."""
        assert torch.is_tensor(dz) and dz.is_cuda and dz.dtype == torch.float32
        dz = dz.detach().contiguous()
        assert dz.dim() == 2 and dz.shape[1] == DIM, tuple(dz.shape)
        N = int(dz.shape[0])
        with torch.cuda.device(dz.device):
            H = self._H if self._H is not None and self._H.shape[0] == N else torch.empty(max(N, 1), STEPS, DIM, dtype=torch.float32, device=dz.device)
            dH = torch.empty(N, STEPS, DIM, dtype=torch.float32, device=dz.device) if want_dH else None
            ws = self._ws if self._ws is not None else torch.empty(256, dtype=torch.uint8, device=dz.device)
            check(lib.sdfa_attntrain_backward(self._h, _ptr(H), _ptr(dz), N, _ptr(dH) if want_dH else None, _ptr(ws), ws.numel(), _stream()))
        return dH

    def step(self):
        with torch.cuda.device(self.device):
            check(lib.sdfa_attntrain_adam(self._h, self.lr, self.betas[0], self.betas[1], self.eps, _stream()))
        self._H = None

    def zero_grad(self):
        with torch.cuda.device(self.device):
            check(lib.sdfa_attntrain_zero_grad(self._h, _stream()))

    # ------------------------------------------------------------------------------------------------ access
    @property
    def step_count(self):
        return int(check(lib.sdfa_attntrain_step_count(self._h)))

    def _read(self, what):
        out = {}
        with torch.cuda.device(self.device):
            for name, shape in self.shapes.items():
                a = np.empty(shape, np.float32)
                check(lib.sdfa_attntrain_get_tensor(self._h, name.encode(), what, a.ctypes.data, a.size))
                out[name] = a
        return out

    def _write(self, what, tensors):
        with torch.cuda.device(self.device):
            for name, v in tensors.items():
                a = _f32(v)
                check(lib.sdfa_attntrain_set_state(self._h, _strip(name).encode(), what, a.ctypes.data, a.size))

    def parameters(self):
        """{name without "_model.": float32 array} read back from the device."""
        return self._read(PARAM)

    def grads(self):
        return self._read(GRAD)

    def moments(self):
        return self._read(EXP_AVG), self._read(EXP_AVG_SQ)

    def set_grads(self, grads):
        self._write(GRAD, grads)

    def attn_state_dict(self, prefix="_model."):
        """The tuned layer as torch tensors under the reference's names."""
        return {prefix + k: torch.from_numpy(v) for k, v in self.parameters().items()}

    def state_dict(self):
        m, v = self.moments()
        return dict(params=self.parameters(), exp_avg=m, exp_avg_sq=v, step=self.step_count, lr=self.lr, betas=self.betas, eps=self.eps)

    def load_state_dict(self, state):
        self._write(PARAM, state["params"])
        self._write(EXP_AVG, state["exp_avg"])
        self._write(EXP_AVG_SQ, state["exp_avg_sq"])
        check(lib.sdfa_attntrain_set_step_count(self._h, int(state["step"])))
        self.lr, self.betas, self.eps = float(state["lr"]), tuple(float(b) for b in state["betas"]), float(state["eps"])
        self._H = None
        return self


# trainers the custom op torch.ops.sdfa.attn_train finds by key; weak, as the model registry of sdfa_amd.ops is
_TRAINERS = weakref.WeakValueDictionary()
_ANON = itertools.count(1)


def register_trainer(trainer, key=None):
    key = f"sdfa-attn-trainer-{next(_ANON)}" if key is None else str(key)
    _TRAINERS[key] = trainer
    return key


def trainer_of(key):
    try:
        return _TRAINERS[key]
    except KeyError:
        raise KeyError(f"sdfa: no attention trainer registered as {key!r} (sdfa_amd.attntrain.register_trainer)") from None
