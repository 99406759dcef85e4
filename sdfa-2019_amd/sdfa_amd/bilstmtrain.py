"""The frozen encoder's exit in front of the BiLSTM: host side of sdfa_encoder_x0 in libsdfa_hip.so (csrc/api_forward.cpp, C ABI in
include/sdfa_bilstm.h).  X0 [N][64][256] is the 256-feature frequency projection of every column of every frame as rows, what
layer 0 of the reference's torch.nn.LSTM(256, 256, num_layers=2, bias=False, bidirectional=True) reads -- the input of
sdfa_amd.lstmtrain.LstmTrainer(layer=0).  With it both layers of the BiLSTM train from train_step
(enable_head_training(attention=True, bilstm_top=True, bilstm_bottom=True)).  The contract is written down in the header and in
DESIGN.md section 19.

A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

from ._lib import bind, lib

ABI_VERSION = 1          # include/sdfa_bilstm.h SDFA_BILSTM_ABI_VERSION this binding was written against
STEPS, FEATURES = 64, 256

_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_bilstm_abi_version": (C.c_int, []),
    "sdfa_encoder_x0": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
}


bind(SYMBOLS, "sdfa_bilstm_abi_version", ABI_VERSION, "bilstm")
