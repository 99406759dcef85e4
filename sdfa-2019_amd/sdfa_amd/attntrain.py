"""Fine-tuning the attention layer on the GPU: host side of sdfa_attntrain* in libsdfa_hip.so (csrc/attntrain.hip and
api_attntrain.cpp, C ABI in include/sdfa_attntrain.h).  The reference's Bahdanau attention (speech_anime/layers/attentions.py,
("attn", "bah", 512, 128, 2), called with query = H[:, 31:34] and key = H in training mode) as a training forward, the analytic
backward down to dH, and torch.optim.Adam(lr=1e-4, weight_decay=0).  It consumes the dz that sdfa_amd.headtrain produces.  The
contract is written down in the header and in DESIGN.md section 17.

AttnTrainer owns the parameters, the gradients and the Adam state on the device; forward / backward / step are stream-ordered
and read nothing back.  A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream
from ._trainer import PARAM, GRAD, EXP_AVG, EXP_AVG_SQ, Registry, Trainer

ABI_VERSION = 1          # include/sdfa_attntrain.h SDFA_ATTNTRAIN_ABI_VERSION this binding was written against
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


bind(SYMBOLS, "sdfa_attntrain_abi_version", ABI_VERSION, "attntrain")


def tensor_shapes():
    """{tensor name without "_model.": shape} of the layer's trainable tensors, as the reference's state dict has them."""
    return dict(SHAPES)


class AttnTrainer(Trainer):
    """The attention layer of a checkpoint with its gradients and Adam state on the device.

    state_dict: the reference's names, with or without "_model."; every other tensor is ignored.
    forward(H) -> (z [N][512], align [N][64]) for H float32 cuda [N][64][512];  backward(dz, want_dH=True) -> dH [N][64][512] |
    None, gradients OVERWRITTEN in the trainer;  step() is one torch.optim.Adam step;  grads() / parameters() read back under the
    reference's names;  state_dict() / load_state_dict() carry parameters, both moments and the step count, so a fit can resume."""

    ABI = "attntrain"

    def __init__(self, state_dict, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, device=None, want_dH=True):
        self.want_dH = bool(want_dH)          # what the backward of torch.ops.sdfa.attn_train returns for H
        super().__init__(state_dict, tensor_shapes(), (), lr, betas, eps, device)
        self._H = None

    def forward(self, H):
        """H float32 cuda [N][64][512] -> (z float32 [N][512], align float32 [N][64]).  H is kept (not copied) for the backward."""
        assert torch.is_tensor(H) and H.is_cuda and H.dtype == torch.float32, "sdfa_amd.attntrain takes cuda tensors: there is no CPU path"
        assert H.dim() == 3 and tuple(H.shape[1:]) == (STEPS, DIM), tuple(H.shape)
        H = H.detach().contiguous()
        N = int(H.shape[0])
        with torch.cuda.device(H.device):
            ws = self._workspace(N, H.device)
            z = torch.empty(N, DIM, dtype=torch.float32, device=H.device)
            align = torch.empty(N, STEPS, dtype=torch.float32, device=H.device)
            check(lib.sdfa_attntrain_forward(self._h, _ptr(H), N, _ptr(z), _ptr(align), _ptr(ws), ws.numel(), _stream()))
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

    def _forget(self):
        self._H = None

    def attn_state_dict(self, prefix="_model."):
        """The tuned layer as torch tensors under the reference's names."""
        return self.tuned_state_dict(prefix)


# trainers the custom op torch.ops.sdfa.attn_train finds by key
_REGISTRY = Registry("attn", "attention")
register_trainer, trainer_of = _REGISTRY.register, _REGISTRY.find
