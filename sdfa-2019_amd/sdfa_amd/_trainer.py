"""What the GPU trainers (sdfa_amd.headtrain, attntrain, lstmtrain, freqtrain, convtrain) share on the host: a handle of
libsdfa_hip.so that owns parameters, gradients and the Adam state on the device (csrc/trainstate.h), read and written under the reference's tensor names,
and the weak registry through which a custom op of sdfa_amd.ops finds its trainer.  A subclass names its symbol prefix and its
tensors and supplies forward and backward; DESIGN.md section 20."""
import ctypes as C
import itertools
import weakref

import numpy as np
import torch

from ._lib import lib, check
from ._packed import stream as _stream

PARAM, GRAD, EXP_AVG, EXP_AVG_SQ = 0, 1, 2, 3      # `what` of get_tensor / set_state, the same in the three headers


def _strip(name):
    return name[len("_model."):] if name.startswith("_model.") else name


def _f32(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v, np.float32))


class Trainer:
    """A training handle `sdfa_<ABI>_*`: created with `create_args`, given the tensors of `shapes` ({name without "_model.": shape})
    and of `constants` (required, never stepped) that `state_dict` has, and finalised on `device`.  step() is one torch.optim.Adam
    step;  grads() / parameters() read back under the reference's names;  state_dict() / load_state_dict() carry parameters, both
    moments and the step count, so a fit can resume."""

    ABI = None          # "headtrain": the symbols are sdfa_headtrain_create, ...

    def _fn(self, name):
        return getattr(lib, f"sdfa_{self.ABI}_{name}")

    def __init__(self, state_dict, shapes, create_args=(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None, constants=None):
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.shapes = shapes
        self.constants = dict(constants or {})               # tensors the handle requires and never steps: {name: shape}
        self._h = None
        h = self._fn("create")(*create_args)
        if not h:
            check(-1)
        self._h = C.c_void_p(h)
        self._finalizer = weakref.finalize(self, self._fn("destroy"), self._h)
        given = {_strip(k): v for k, v in state_dict.items()}
        for name in (*self.shapes, *self.constants):
            if name not in given:
                continue                                     # finalize names the first missing tensor
            a = _f32(given[name])
            check(self._fn("set_tensor")(self._h, name.encode(), a.ctypes.data, a.size))
        with torch.cuda.device(self.device):
            check(self._fn("finalize")(self._h, _stream()))
        self.numel = int(check(self._fn("numel")(self._h)))
        self._ws = None

    # ------------------------------------------------------------------------------------------------ the step
    def workspace_bytes(self, n):
        return int(check(self._fn("workspace_bytes")(self._h, int(n))))

    def _workspace(self, n, device):
        """the trainer's workspace, grown to a batch of n rows / frames on `device`"""
        need = self.workspace_bytes(n)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def _forget(self):
        """drop what the forward kept for the backward: the parameters have changed"""

    def step(self):
        with torch.cuda.device(self.device):
            check(self._fn("adam")(self._h, self.lr, self.betas[0], self.betas[1], self.eps, _stream()))
        self._forget()

    def zero_grad(self):
        with torch.cuda.device(self.device):
            check(self._fn("zero_grad")(self._h, _stream()))

    # ------------------------------------------------------------------------------------------------ access
    @property
    def step_count(self):
        return int(check(self._fn("step_count")(self._h)))

    def _read(self, what):
        out = {}
        with torch.cuda.device(self.device):
            for name, shape in self.shapes.items():
                a = np.empty(shape, np.float32)
                check(self._fn("get_tensor")(self._h, name.encode(), what, a.ctypes.data, a.size))
                out[name] = a
        return out

    def _write(self, what, tensors):
        with torch.cuda.device(self.device):
            for name, v in tensors.items():
                a = _f32(v)
                check(self._fn("set_state")(self._h, _strip(name).encode(), what, a.ctypes.data, a.size))

    def parameters(self):
        """{name without "_model.": float32 array} read back from the device."""
        return self._read(PARAM)

    def grads(self):
        return self._read(GRAD)

    def moments(self):
        return self._read(EXP_AVG), self._read(EXP_AVG_SQ)

    def set_grads(self, grads):
        self._write(GRAD, grads)

    def tuned_state_dict(self, prefix="_model."):
        """The tuned parameters as torch tensors under the reference's names."""
        return {prefix + k: torch.from_numpy(v) for k, v in self.parameters().items()}

    def _state_extra(self):
        """what state_dict() carries besides the parameters, the Adam state and its arguments"""
        return {}

    def state_dict(self):
        m, v = self.moments()
        return dict(params=self.parameters(), exp_avg=m, exp_avg_sq=v, step=self.step_count, lr=self.lr, betas=self.betas, eps=self.eps,
                    **self._state_extra())

    def load_state_dict(self, state):
        self._write(PARAM, state["params"])
        self._write(EXP_AVG, state["exp_avg"])
        self._write(EXP_AVG_SQ, state["exp_avg_sq"])
        check(self._fn("set_step_count")(self._h, int(state["step"])))
        self.lr, self.betas, self.eps = float(state["lr"]), tuple(float(b) for b in state["betas"]), float(state["eps"])
        self._forget()
        return self


class Registry:
    """Trainers a custom op of sdfa_amd.ops finds by key; weak, as the model registry of sdfa_amd.ops is.  kind: "head" (the key is
    sdfa-head-trainer-N, the module sdfa_amd.headtrain); noun: the KeyError's word for it."""

    def __init__(self, kind, noun):
        self.kind, self.noun = kind, noun
        self._TRAINERS = weakref.WeakValueDictionary()
        self._ANON = itertools.count(1)

    def register(self, trainer, key=None):
        key = f"sdfa-{self.kind}-trainer-{next(self._ANON)}" if key is None else str(key)
        self._TRAINERS[key] = trainer
        return key

    def find(self, key):
        try:
            return self._TRAINERS[key]
        except KeyError:
            raise KeyError(f"sdfa: no {self.noun} trainer registered as {key!r} (sdfa_amd.{self.kind}train.register_trainer)") from None
