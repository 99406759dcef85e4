"""Fine-tuning the regressor head on the GPU: host side of sdfa_headtrain* in libsdfa_hip.so (csrc/headtrain.hip and
api_headtrain.cpp, C ABI in include/sdfa_headtrain.h).  The reference's output module (speech_anime/modules/output_module.py
with config/model/{dgrad,offsets}.py) as a training forward, the backward through the fully connected stack and its weight
normalisation, the gradient with respect to the encoder output, and torch.optim.Adam(lr=1e-4, weight_decay=0) as
saber_model.configure_optimizers builds it.  The contract is written down in the header and in DESIGN.md section 16.

HeadTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are
stream-ordered and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import itertools
import weakref

import numpy as np
import torch

from ._lib import lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_headtrain.h SDFA_HEADTRAIN_ABI_VERSION this binding was written against
HEAD_DGRAD, HEAD_OFFSETS = 0, 1
PARAM, GRAD, EXP_AVG, EXP_AVG_SQ = 0, 1, 2, 3
Z_DIM, SPEAKERS, TILE, MAX_ROWS = 512, 8, 64, 1 << 21
LAUNCHES = {"dgrad": dict(forward=5, backward=5, adam=1), "offsets": dict(forward=4, backward=4, adam=1)}    # the fold is the forward's first

_p, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_headtrain_abi_version": (C.c_int, []),
    "sdfa_headtrain_create": (_p, [C.c_int]),
    "sdfa_headtrain_destroy": (None, [_p]),
    "sdfa_headtrain_set_tensor": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_headtrain_finalize": (C.c_int, [_p, _p]),
    "sdfa_headtrain_coef_dim": (C.c_int, [_p]),
    "sdfa_headtrain_numel": (_i64, [_p]),
    "sdfa_headtrain_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_headtrain_forward": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_headtrain_backward": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
    "sdfa_headtrain_adam": (C.c_int, [_p, _f64, _f64, _f64, _f64, _p]),
    "sdfa_headtrain_zero_grad": (C.c_int, [_p, _p]),
    "sdfa_headtrain_get_tensor": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_headtrain_set_grad": (C.c_int, [_p, C.c_char_p, _p, _i64]),
    "sdfa_headtrain_set_state": (C.c_int, [_p, C.c_char_p, C.c_int, _p, _i64]),
    "sdfa_headtrain_step_count": (_i64, [_p]),
    "sdfa_headtrain_set_step_count": (C.c_int, [_p, _i64]),
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
    have = int(lib.sdfa_headtrain_abi_version())
    if have != ABI_VERSION:
        raise ImportError(stale % f"headtrain ABI version {have}, this binding needs {ABI_VERSION}")


_bind()

_BRANCH = ((512, 520), (256, 512), (None, 256))


def layer_shapes(head):
    """[(layer name without "_model.", P, K)] in the order of the flat buffers: the trunk, the scale branch, the rotat branch
    (speech_anime/config/model/dgrad.py); the three layers of config/model/offsets.py."""
    o = "_output_module."
    if head == "dgrad":
        out = [(o + "_layers.0", 512, 520)]
        for br, nco in (("_scale", 85), ("_rotat", 180)):
            out += [(f"{o}{br}_layers.{i}", p or nco, k) for i, (p, k) in enumerate(_BRANCH)]
        return out
    assert head == "offsets", head
    return [(f"{o}_layers.{i}", p or 59, k) for i, (p, k) in enumerate(_BRANCH)]


def tensor_shapes(head):
    """{tensor name without "_model.": shape} of the head's trainable tensors, as the reference's state dict has them."""
    t = {}
    for name, p, k in layer_shapes(head):
        t[name + ".weight_g"], t[name + ".weight_v"], t[name + ".bias"] = (p, 1), (p, k), (p,)
    return t


def _strip(name):
    return name[len("_model."):] if name.startswith("_model.") else name


def _f32(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v, np.float32))


class HeadTrainer:
    """The regressor head of a checkpoint with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; tensors of the encoder and the PCA are ignored.
    forward(z, speaker_id) -> coef [N][Kc];  backward(dcoef, want_dz=True) -> dz [N][512] | None, gradients OVERWRITTEN in
    the trainer;  step() is one torch.optim.Adam step;  grads() / parameters() read back under the reference's names;
    state_dict() / load_state_dict() carry parameters, both moments and the step count, so a fit can resume."""

    def __init__(self, state_dict, head, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None):
        assert head in ("dgrad", "offsets"), head
        self.head = head
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.shapes = tensor_shapes(head)
        self._h = None
        h = lib.sdfa_headtrain_create(HEAD_DGRAD if head == "dgrad" else HEAD_OFFSETS)
        if not h:
            check(-1)
        self._h = C.c_void_p(h)
        self._finalizer = weakref.finalize(self, lib.sdfa_headtrain_destroy, self._h)
        given = {_strip(k): v for k, v in state_dict.items()}
        for name, shape in self.shapes.items():
            if name not in given:
                continue                                     # finalize names the first missing tensor
            a = _f32(given[name])
            check(lib.sdfa_headtrain_set_tensor(self._h, name.encode(), a.ctypes.data, a.size))
        with torch.cuda.device(self.device):
            check(lib.sdfa_headtrain_finalize(self._h, _stream()))
        self.coef_dim = int(check(lib.sdfa_headtrain_coef_dim(self._h)))
        self.numel = int(check(lib.sdfa_headtrain_numel(self._h)))
        self._ws = None
        self._n = 0

    # ------------------------------------------------------------------------------------------------ the step
    def workspace_bytes(self, rows):
        return int(check(lib.sdfa_headtrain_workspace_bytes(self._h, int(rows))))

    def forward(self, z, speaker_id, check_ids=True):
        """z float32 cuda [N][512], speaker_id int64 [N] (host or device) -> coef float32 [N][Kc].  An id outside 0 .. 7 raises
        what the reference's one_hot raises; check_ids=False: the caller has validated them."""
        assert torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32, "sdfa_amd.headtrain takes cuda tensors: there is no CPU path"
        z = z.detach().reshape(-1, Z_DIM).contiguous()
        N = int(z.shape[0])
        if check_ids:
            from .engine import Engine
            Engine.check_speaker_ids(speaker_id)
        spk = torch.as_tensor(speaker_id).to(device=z.device, dtype=torch.int64).reshape(-1).contiguous()
        assert spk.numel() == N, (spk.shape, N)
        with torch.cuda.device(z.device):
            need = self.workspace_bytes(N)
            if self._ws is None or self._ws.numel() < need or self._ws.device != z.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=z.device)
            coef = torch.empty(N, self.coef_dim, dtype=torch.float32, device=z.device)
            check(lib.sdfa_headtrain_forward(self._h, _ptr(z), _ptr(spk), N, _ptr(coef), _ptr(self._ws), self._ws.numel(), _stream()))
        self._n = N
        return coef

    def backward(self, dcoef, want_dz=True):
        """dcoef float32 cuda [N][Kc] for the N of the last forward -> dz [N][512] (None without want_dz)."""
        assert torch.is_tensor(dcoef) and dcoef.is_cuda and dcoef.dtype == torch.float32
        dcoef = dcoef.detach().contiguous()
        N = int(dcoef.shape[0])
        assert dcoef.dim() == 2 and dcoef.shape[1] == self.coef_dim, (dcoef.shape, self.coef_dim)
        with torch.cuda.device(dcoef.device):
            dz = torch.empty(N, Z_DIM, dtype=torch.float32, device=dcoef.device) if want_dz else None
            ws = self._ws if self._ws is not None else torch.empty(max(self.workspace_bytes(max(N, 2)), 256), dtype=torch.uint8, device=dcoef.device)
            check(lib.sdfa_headtrain_backward(self._h, _ptr(dcoef), N, _ptr(dz) if want_dz else None, _ptr(ws), ws.numel(), _stream()))
        return dz

    def step(self):
        with torch.cuda.device(self.device):
            check(lib.sdfa_headtrain_adam(self._h, self.lr, self.betas[0], self.betas[1], self.eps, _stream()))

    def zero_grad(self):
        with torch.cuda.device(self.device):
            check(lib.sdfa_headtrain_zero_grad(self._h, _stream()))

    # ------------------------------------------------------------------------------------------------ access
    @property
    def step_count(self):
        return int(check(lib.sdfa_headtrain_step_count(self._h)))

    def _read(self, what):
        out = {}
        with torch.cuda.device(self.device):
            for name, shape in self.shapes.items():
                a = np.empty(shape, np.float32)
                check(lib.sdfa_headtrain_get_tensor(self._h, name.encode(), what, a.ctypes.data, a.size))
                out[name] = a
        return out

    def _write(self, what, tensors):
        with torch.cuda.device(self.device):
            for name, v in tensors.items():
                a = _f32(v)
                check(lib.sdfa_headtrain_set_state(self._h, _strip(name).encode(), what, a.ctypes.data, a.size))

    def parameters(self):
        """{name without "_model.": float32 array} read back from the device."""
        return self._read(PARAM)

    def grads(self):
        return self._read(GRAD)

    def moments(self):
        return self._read(EXP_AVG), self._read(EXP_AVG_SQ)

    def set_grads(self, grads):
        self._write(GRAD, grads)

    def head_state_dict(self, prefix="_model."):
        """The tuned head as torch tensors under the reference's names."""
        return {prefix + k: torch.from_numpy(v) for k, v in self.parameters().items()}

    def state_dict(self):
        m, v = self.moments()
        return dict(head=self.head, params=self.parameters(), exp_avg=m, exp_avg_sq=v, step=self.step_count,
                    lr=self.lr, betas=self.betas, eps=self.eps)

    def load_state_dict(self, state):
        assert state["head"] == self.head, (state["head"], self.head)
        self._write(PARAM, state["params"])
        self._write(EXP_AVG, state["exp_avg"])
        self._write(EXP_AVG_SQ, state["exp_avg_sq"])
        check(lib.sdfa_headtrain_set_step_count(self._h, int(state["step"])))
        self.lr, self.betas, self.eps = float(state["lr"]), tuple(float(b) for b in state["betas"]), float(state["eps"])
        return self


# trainers the custom op torch.ops.sdfa.head_train finds by key; weak, as the model registry of sdfa_amd.ops is
_TRAINERS = weakref.WeakValueDictionary()
_ANON = itertools.count(1)


def register_trainer(trainer, key=None):
    key = f"sdfa-head-trainer-{next(_ANON)}" if key is None else str(key)
    _TRAINERS[key] = trainer
    return key


def trainer_of(key):
    try:
        return _TRAINERS[key]
    except KeyError:
        raise KeyError(f"sdfa: no head trainer registered as {key!r} (sdfa_amd.headtrain.register_trainer)") from None
