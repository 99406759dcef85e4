"""Augmented training-window features on the GPU: host side of sdfa_augment_* in libsdfa_hip.so (csrc/frontend.hip
frontend_augment_kernel and api_augment.cpp, C ABI in include/sdfa_augment.h).  The training branch of the reference's
windowed_features (speech_anime/datasets/get_features.py:8-223): a window at an arbitrary sample offset, additive noise, a
per-window pre-emphasis, a stretch in time (56 - 72 STFT columns resized to 64), a shift / stretch in frequency (123 - 133 mel
rows resized to 128), a per-band gain, band dropout, then the deltas.  The contract is written down in the header and in
DESIGN.md section 14.

augment_frontend() is stream-ordered.  pack_desc() and check_desc() are host arithmetic; white_noise() draws on the device
with torch.randn -- NOT NumPy's stream: a caller who needs the reference's very noise draws it with numpy and uploads it.
A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C

import numpy as np
import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_augment.h SDFA_AUGMENT_ABI_VERSION this binding was written against
EX_TIME_MAX, EX_FEAT_MAX = 4, 5
LOWER_FREQ, TRUNCK, PAD_REFLECT = 1, 2, 4
# sdfa_augment_desc, 48 bytes
DESC = np.dtype([("clip", "<i4"), ("ex_time", "<i4"), ("start", "<i8"), ("preemph", "<f4"), ("ex_feat", "<i4"),
                 ("flags", "<u4"), ("reserved", "<u4"), ("drop", "<u4", (4,))])
assert DESC.itemsize == 48

_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_augment_abi_version": (C.c_int, []),
    "sdfa_augment_noise_samples": (_i64, [C.c_int]),
    "sdfa_augment_check": (C.c_int, [_p, _i64, _p, C.c_int32]),
    "sdfa_augment_frontend": (C.c_int, [_p, _p, _p, C.c_int32, _p, _i64, C.c_int, _p, _i64, _p, _p, _p]),
}


bind(SYMBOLS, "sdfa_augment_abi_version", ABI_VERSION, "augment")


def noise_samples(sr):
    """Samples of the longest cut, 71 hop + win: the least noise_stride."""
    return int(check(lib.sdfa_augment_noise_samples(int(sr))))


def drop_words(mask_idx):
    """Row indices (duplicates allowed, as np.random.choice draws them) -> the 128-bit mask as uint32 [4]."""
    w = np.zeros(4, np.uint32)
    for r in np.asarray(mask_idx, np.int64).reshape(-1):
        assert 0 <= r < 128, r
        w[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return w


def pack_desc(clip, start, ex_time=0, preemph=0.65, ex_feat=0, lower_freq=False, trunck=False, pad_reflect=False, drop=None):
    """Arrays (or scalars, broadcast against `start`) -> sdfa_augment_desc records, a numpy array of dtype DESC.  drop: None, or
    per window a list of row indices / a uint32 [4] mask (an array [n][4] of masks is taken as it is)."""
    start = np.atleast_1d(np.asarray(start, np.int64))
    n = start.shape[0]
    d = np.zeros(n, DESC)
    d["start"] = start
    d["clip"] = np.broadcast_to(np.asarray(clip, np.int32), n)
    d["ex_time"] = np.broadcast_to(np.asarray(ex_time, np.int32), n)
    d["ex_feat"] = np.broadcast_to(np.asarray(ex_feat, np.int32), n)
    d["preemph"] = np.broadcast_to(np.asarray(preemph, np.float32), n)
    bit = lambda v, b: np.broadcast_to(np.asarray(v, bool), n).astype(np.uint32) * np.uint32(b)
    d["flags"] = bit(lower_freq, LOWER_FREQ) | bit(trunck, TRUNCK) | bit(pad_reflect, PAD_REFLECT)
    if drop is not None:
        if isinstance(drop, np.ndarray) and drop.dtype == np.uint32 and drop.shape == (n, 4):
            d["drop"] = drop
        else:
            assert len(drop) == n, (len(drop), n)
            for i, m in enumerate(drop):
                m = np.asarray([] if m is None else m)
                d["drop"][i] = m if (m.dtype == np.uint32 and m.shape == (4,)) else drop_words(m)
    return d


def unpack_desc(desc):
    """The fields of DESC records as a dict of arrays (flags split, drop as lists of row indices): pack_desc's inverse."""
    d = np.asarray(desc, DESC)
    rows = [[r for r in range(128) if (int(w[r >> 5]) >> (r & 31)) & 1] for w in d["drop"]]
    return dict(clip=d["clip"].copy(), start=d["start"].copy(), ex_time=d["ex_time"].copy(), preemph=d["preemph"].copy(),
                ex_feat=d["ex_feat"].copy(), lower_freq=(d["flags"] & LOWER_FREQ) != 0, trunck=(d["flags"] & TRUNCK) != 0,
                pad_reflect=(d["flags"] & PAD_REFLECT) != 0, drop=rows)


def check_desc(desc, clip_len=None):
    """sdfa_augment_check: raises SdfaError (SDFA_EINVAL) for a descriptor the kernel's contract excludes.  clip_len: host
    integers [n_clips], or None."""
    d = np.ascontiguousarray(np.asarray(desc, DESC))
    ln = None if clip_len is None else np.ascontiguousarray(np.asarray(clip_len, np.int64).reshape(-1))
    check(lib.sdfa_augment_check(d.ctypes.data if d.size else None, d.size, None if ln is None else ln.ctypes.data,
                                 0 if ln is None else ln.size))


def white_noise(n, stride, scales, generator=None, device="cuda"):
    """n rows of `stride` float32 samples N(0, 1) * scales[i] on the device (saber.audio.white_noise is
    np.random.normal(0, 1) * scale).  torch.randn's stream, not NumPy's: the values differ from the reference's, their
    distribution does not.  A scale of 0 gives a row of zeros (noise type "none")."""
    sc = torch.as_tensor(np.asarray(scales, np.float32).reshape(-1)).to(device)
    assert sc.shape[0] == n, (sc.shape, n)
    z = torch.randn((n, int(stride)), dtype=torch.float32, device=device, generator=generator)
    return z.mul_(sc[:, None])


def augment_frontend(pcm, clip_off, clip_len, desc, sr, noise=None, scale=None, out=None):
    """pcm float32, clip_off / clip_len int64 [n_clips] (cuda tensors, as sdfa_amd.ops.mel_frontend takes them); desc: DESC
    records on the host (checked, then uploaded) or a cuda uint8 tensor of them (taken as it is); noise [n][stride >=
    noise_samples(sr)] and scale [n][128] float32 cuda or None -> audio_feat (n, 64, 128, 3) float32 on the device."""
    assert torch.is_tensor(pcm) and pcm.is_cuda and pcm.dtype == torch.float32 and pcm.is_contiguous(), "sdfa_amd.augment takes cuda tensors: there is no CPU path"
    dev = pcm.device
    for t in (clip_off, clip_len):
        assert torch.is_tensor(t) and t.device == dev and t.dtype == torch.int64 and t.is_contiguous()
    n_clips = int(clip_len.numel())
    assert clip_off.numel() == n_clips
    if torch.is_tensor(desc):
        assert desc.device == dev and desc.dtype == torch.uint8 and desc.is_contiguous() and desc.numel() % DESC.itemsize == 0
        d_desc = desc
    else:
        h = np.ascontiguousarray(np.asarray(desc, DESC))
        check_desc(h)
        assert h.size == 0 or int(h["clip"].max()) < n_clips, "descriptor names a clip the batch does not have"
        d_desc = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    n = d_desc.numel() // DESC.itemsize
    stride = 0
    if noise is not None:
        assert noise.device == dev and noise.dtype == torch.float32 and noise.is_contiguous() and noise.dim() == 2 and noise.shape[0] == n, noise.shape
        stride = int(noise.shape[1])
    if scale is not None:
        assert scale.device == dev and scale.dtype == torch.float32 and scale.is_contiguous() and tuple(scale.shape) == (n, 128), scale.shape
    if out is None:
        out = torch.empty((n, 64, 128, 3), dtype=torch.float32, device=dev)
    assert out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, 64, 128, 3), out.shape
    with torch.cuda.device(dev):
        check(lib.sdfa_augment_frontend(_ptr(pcm), _ptr(clip_off), _ptr(clip_len), n_clips, _ptr(d_desc), n, int(sr),
                                        None if noise is None else _ptr(noise), stride, None if scale is None else _ptr(scale),
                                        _ptr(out), _stream()))
    return out


def upload_clips(clips, device="cuda"):
    """A list of float32 arrays -> (pcm, clip_off, clip_len) on the device, one sample of padding behind the last clip so that a
    batch of empty clips still owns an address."""
    arrs = [np.asarray(c, np.float32).reshape(-1) for c in clips]
    lens = np.asarray([len(a) for a in arrs], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    flat = np.concatenate(arrs + [np.zeros(1, np.float32)])
    return torch.from_numpy(flat).to(device), torch.from_numpy(offs).to(device), torch.from_numpy(lens).to(device)
