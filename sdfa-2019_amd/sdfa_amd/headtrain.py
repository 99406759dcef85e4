"""Fine-tuning the regressor head on the GPU: host side of sdfa_headtrain* in libsdfa_hip.so (csrc/headtrain.hip and
api_headtrain.cpp, C ABI in include/sdfa_headtrain.h).  The reference's output module (speech_anime/modules/output_module.py
with config/model/{dgrad,offsets}.py) as a training forward, the backward through the fully connected stack and its weight
normalisation, the gradient with respect to the encoder output, and torch.optim.Adam(lr=1e-4, weight_decay=0) as
saber_model.configure_optimizers builds it.  The contract is written down in the header and in DESIGN.md section 16.

HeadTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are
stream-ordered and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream
from ._trainer import PARAM, GRAD, EXP_AVG, EXP_AVG_SQ, Registry, Trainer

ABI_VERSION = 1          # include/sdfa_headtrain.h SDFA_HEADTRAIN_ABI_VERSION this binding was written against
HEAD_DGRAD, HEAD_OFFSETS = 0, 1
Z_DIM, SPEAKERS, TILE, MAX_ROWS = 512, 8, 64, 1 << 21
LAUNCHES = {"dgrad": dict(forward=5, backward=5, adam=1), "offsets": dict(forward=4, backward=4, adam=1)}    # the fold is the forward's first; above 4,096 rows the backward has one more, the row blocks' reduce

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


bind(SYMBOLS, "sdfa_headtrain_abi_version", ABI_VERSION, "headtrain")

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


class HeadTrainer(Trainer):
    """The regressor head of a checkpoint with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; tensors of the encoder and the PCA are ignored.
    forward(z, speaker_id) -> coef [N][Kc];  backward(dcoef, want_dz=True) -> dz [N][512] | None, gradients OVERWRITTEN in
    the trainer;  step() is one torch.optim.Adam step;  grads() / parameters() read back under the reference's names;
    state_dict() / load_state_dict() carry parameters, both moments and the step count, so a fit can resume."""

    ABI = "headtrain"

    def __init__(self, state_dict, head, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None):
        assert head in ("dgrad", "offsets"), head
        self.head = head
        super().__init__(state_dict, tensor_shapes(head), (HEAD_DGRAD if head == "dgrad" else HEAD_OFFSETS,), lr, betas, eps, device)
        self.coef_dim = int(check(lib.sdfa_headtrain_coef_dim(self._h)))

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
            ws = self._workspace(N, z.device)
            coef = torch.empty(N, self.coef_dim, dtype=torch.float32, device=z.device)
            check(lib.sdfa_headtrain_forward(self._h, _ptr(z), _ptr(spk), N, _ptr(coef), _ptr(ws), ws.numel(), _stream()))
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

    def head_state_dict(self, prefix="_model."):
        """The tuned head as torch tensors under the reference's names."""
        return self.tuned_state_dict(prefix)

    def _state_extra(self):
        return dict(head=self.head)

    def load_state_dict(self, state):
        assert state["head"] == self.head, (state["head"], self.head)
        return super().load_state_dict(state)


# trainers the custom op torch.ops.sdfa.head_train finds by key
_REGISTRY = Registry("head", "head")
register_trainer, trainer_of = _REGISTRY.register, _REGISTRY.find
