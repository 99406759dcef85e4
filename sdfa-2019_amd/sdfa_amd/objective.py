"""The reference's training objective on the GPU: host side of sdfa_objective* in libsdfa_hip.so (csrc/objective.hip and
api_objective.cpp, C ABI in include/sdfa_objective.h).  get_loss (speech_anime/model/model.py:261-330) as an objective for
prediction_type "face_data" with pca_trainable = False: PcaInversion (modules/output_module.py:94-116), PLoss and MLoss
(model/criterion.py:7-73) of a collated batch [a; b] and their gradients with respect to the PCA coefficients, in one pass
over the basis and the targets.  The contract is written down in the header and in DESIGN.md section 15.

objective() is stream-ordered and reads nothing back.  attach_bases() puts a head's plain compT / means on the device once
per model, for models that opt in; bases_of() finds them.  DynamicLossScaler restates criterion.py:90-112 as host state.  Absent: ELoss (this model emits no evector).  A library
without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import math
import weakref

import numpy as np
import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_objective.h SDFA_OBJECTIVE_ABI_VERSION this binding was written against
LAYOUT_DGRAD, LAYOUT_PLAIN = 0, 1
MAX_K, COLS, PAIRS, KSTEP = 192, 128, 16, 8      # SDFA_OBJECTIVE_MAX_K / _COLS / _PAIRS / _KSTEP (the expansion's step along k)
LOSS_NAMES = ("ps", "ms", "pr", "mr")            # the order of loss[4] and of a record's slots

_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_objective_abi_version": (C.c_int, []),
    "sdfa_objective_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64, C.c_int]),
    "sdfa_objective": (C.c_int, [_p, _i64, _i64, _i64, _i64, C.c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
}


bind(SYMBOLS, "sdfa_objective_abi_version", ABI_VERSION, "objective")


class Bases:
    """A head's PCA bases in the reference's layout, on the device: layout, compT_s [6T | W][Ks], means_s, and for dgrad
    compT_r [3T][Kr], means_r."""

    def __init__(self, layout, compT_s, means_s, compT_r=None, means_r=None):
        self.layout = int(layout)
        self.compT_s, self.means_s, self.compT_r, self.means_r = compT_s, means_s, compT_r, means_r
        for t in (compT_s, means_s) + ((compT_r, means_r) if self.layout == LAYOUT_DGRAD else ()):
            assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "bases are contiguous float32 cuda tensors"
        self.Ks = int(compT_s.shape[1])
        self.Kr = int(compT_r.shape[1]) if self.layout == LAYOUT_DGRAD else 0
        if self.layout == LAYOUT_DGRAD:
            T = compT_r.shape[0] // 3
            assert compT_s.shape[0] == 6 * T and compT_r.shape[0] == 3 * T and means_s.numel() == 6 * T and means_r.numel() == 3 * T, "dgrad bases: [6T][Ks] and [3T][Kr]"
            self.W = 9 * T
        else:
            self.W = int(compT_s.shape[0])
            assert means_s.numel() == self.W
        self.Kc = self.Ks + self.Kr
        self.n = self.W // 9 if self.layout == LAYOUT_DGRAD else self.W      # the divisor PLoss / MLoss end up with


_PCA_KEYS = (("_scale_pca.compT", "_scale_pca.means", "_rotat_pca.compT", "_rotat_pca.means"), ("_pca.compT", "_pca.means"))


_ATTACHED = weakref.WeakKeyDictionary()      # Engine -> Bases: dropped with the engine


def attach_bases(engine, source):
    """Opt a model in to the objective: `source` is the state dict the engine was made from (or a sdfa_amd.pca result under
    the reference's names), or a Bases.  The plain compT / means go to the engine's device once and stay with the engine; an
    engine that is never attached pays nothing for this feature."""
    bases = source if isinstance(source, Bases) else bases_of(source, engine.device)
    want = LAYOUT_DGRAD if engine.head == "dgrad" else LAYOUT_PLAIN
    assert bases.layout == want and bases.W == engine.out_dim and bases.Kc == engine.coef_dim, "these bases are not this engine's head"
    _ATTACHED[engine] = bases
    return bases


def bases_of(model, device=None):
    """Engine -> the Bases attach_bases gave it (the engine's own packed copies are in another layout, and it does not keep
    the state dict); a state dict in the reference's names -> new Bases on `device` (default: the current one)."""
    if not isinstance(model, dict) and not hasattr(model, "keys"):
        try:
            return _ATTACHED[model]
        except KeyError:
            raise KeyError("no PCA bases attached to this engine: call sdfa_amd.objective.attach_bases(engine, state_dict) "
                           "(SaberSpeechDrivenAnimation.enable_training_objective) once before the objective is used") from None
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def find(suffix):
        hit = [k for k in model if k.endswith("_output_module." + suffix) or k == suffix]
        assert len(hit) == 1, f"state dict holds {len(hit)} tensors named *{suffix}"
        v = model[hit[0]]
        v = v.detach() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32)))
        return v.to(device=dev, dtype=torch.float32).contiguous()

    if any("_scale_pca" in k for k in model):
        return Bases(LAYOUT_DGRAD, *(find(s) for s in _PCA_KEYS[0]))
    return Bases(LAYOUT_PLAIN, *(find(s) for s in _PCA_KEYS[1]))


def workspace_bytes(N, W, Ks, Kr, layout):
    return int(check(lib.sdfa_objective_workspace_bytes(int(N), int(W), int(Ks), int(Kr), int(layout))))


def objective(coef, truth, weight, bases, layout=None):
    """coef [2B][Kc], truth [2B][W], weight [2B] float32 cuda, bases a Bases -> (loss float32 [4] = (ps, ms, pr, mr),
    rec float64 [2B][4], grad float32 [2][2B][Kc]) on the device.  Stream-ordered; nothing is read back."""
    assert torch.is_tensor(coef) and coef.is_cuda and coef.dtype == torch.float32, "sdfa_amd.objective takes cuda tensors: there is no CPU path"
    layout = bases.layout if layout is None else int(layout)
    assert layout == bases.layout, (layout, bases.layout)
    dev = coef.device
    coef = coef.detach()
    N = int(coef.shape[0])
    truth = truth.reshape(N, -1) if N else truth
    for t in (truth, weight):
        assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == dev
    assert coef.is_contiguous() and truth.is_contiguous() and weight.is_contiguous(), "inputs must be contiguous: they are read in place"
    assert coef.dim() == 2 and coef.shape[1] == bases.Kc, (coef.shape, bases.Kc)
    assert truth.shape[1] == bases.W and weight.numel() == N, (truth.shape, weight.shape, bases.W)
    assert bases.compT_s.device == dev
    with torch.cuda.device(dev):
        need = workspace_bytes(N, bases.W, bases.Ks, bases.Kr, layout)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        loss = torch.empty(4, dtype=torch.float32, device=dev)
        rec = torch.empty(N, 4, dtype=torch.float64, device=dev)
        grad = torch.empty(2, N, bases.Kc, dtype=torch.float32, device=dev)
        dg = layout == LAYOUT_DGRAD
        check(lib.sdfa_objective(_ptr(coef), N, bases.W, bases.Ks, bases.Kr, layout, _ptr(bases.compT_s), _ptr(bases.means_s),
                                 _ptr(bases.compT_r) if dg else None, _ptr(bases.means_r) if dg else None, _ptr(truth), _ptr(weight),
                                 _ptr(loss), _ptr(rec), _ptr(grad), _ptr(ws), need, _stream()))
    return loss, rec, grad


def scalars_of(rec, weight, n):
    """Records [2B][4] and weights [2B] -> the four losses in float64 on the host, without the kernel's float32 rounding:
    {"ps", "ms", "pr", "mr"}.  h_k is the float32 sum the reference forms."""
    rec = rec.detach().cpu().numpy() if torch.is_tensor(rec) else np.asarray(rec)
    w = weight.detach().cpu().numpy() if torch.is_tensor(weight) else np.asarray(weight)
    w = np.asarray(w, np.float32).reshape(-1)
    N = rec.shape[0]
    B = N // 2
    h = (w[B:] + w[:B]).astype(np.float64)
    w = w.astype(np.float64)
    out = {}
    for slot, name in enumerate(LOSS_NAMES):
        out[name] = float((h * rec[B:, slot]).sum() / (B * n)) if slot & 1 else float((w * rec[:, slot]).sum() / (N * n))
    return out


class DynamicLossScaler:
    """criterion.py:90-112 as host state: beta, eps, vt, beta_t, scale.  scale_loss(loss, training) takes the 0-dim loss tensor
    (or a float); in training it reads the value -- one synchronising .item(), as the reference's float(...) is -- and
    updates the running second moment with loss_ms = loss^2, the float32 square the reference takes from the 0-dim tensor;
    it returns loss / scale.  state_dict() / load_state_dict() let a run resume, which the reference cannot."""

    def __init__(self, beta=0.99, eps=1e-8):
        self.beta = beta
        self.eps = eps
        self.reset_state()

    def reset_state(self):
        self.vt = 0.0
        self.beta_t = 1.0
        self.scale = 1.0

    def update(self, loss_value):
        """loss_value: the loss as a float32 value.  loss_ms is its float32 square, as (loss ** 2).mean(dim=0) of a float32
        0-dim tensor gives."""
        loss_ms = float(np.float32(loss_value) * np.float32(loss_value))
        self.beta_t = self.beta_t * self.beta
        self.vt = self.beta * self.vt + (1.0 - self.beta) * loss_ms
        self.scale = math.sqrt(self.vt / (1.0 - self.beta_t)) + self.eps
        return self.scale

    def scale_loss(self, loss, training):
        if training:
            self.update(float(loss.detach()) if torch.is_tensor(loss) else float(loss))
        return loss / self.scale

    def state_dict(self):
        return dict(beta=self.beta, eps=self.eps, vt=self.vt, beta_t=self.beta_t, scale=self.scale)

    def load_state_dict(self, state):
        self.beta, self.eps = float(state["beta"]), float(state["eps"])
        self.vt, self.beta_t, self.scale = float(state["vt"]), float(state["beta_t"]), float(state["scale"])
        return self
