"""The reference's validation losses on the GPU: host side of sdfa_score_* in libsdfa_hip.so (csrc/score.hip and api_score.cpp,
C ABI in include/sdfa_score.h).  get_loss (speech_anime/model/model.py:261-330) with PLoss and MLoss
(speech_anime/model/criterion.py:7-73) for prediction_type "face_data": scalar_ps / scalar_ms / scalar_pr / scalar_mr and
their sums scalar_ploss / scalar_mloss -- scalar_ploss is what the reference picks checkpoints by.  The contract -- truth,
per-frame record, clip scalars -- is written down in the header and in DESIGN.md section 12.

score_rows() is stream-ordered; the prediction rows and the track stay where they are on the device and the blended truth
is never materialised.  truth_plan(), dataset_frame_starts(), anime_weights() and clip_scalars() are host arithmetic.
Absent: ELoss (this model emits no evector) and DynamicLossScaler (its state is not in a checkpoint).  A library without the
symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_score.h SDFA_SCORE_ABI_VERSION this binding was written against
LAYOUT_DGRAD, LAYOUT_PLAIN = 0, 1
COLS, RUN, PARTS = 9216, 32, 4          # SDFA_SCORE_COLS (columns per slab), SDFA_SCORE_RUN (frames per run), SDFA_SCORE_PARTS
SCALAR_KEYS = ("scalar_ps", "scalar_pr", "scalar_ms", "scalar_mr", "scalar_ploss", "scalar_mloss")

_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_score_abi_version": (C.c_int, []),
    "sdfa_score_workspace_bytes": (_i64, [_i64, _i64, C.c_int]),
    "sdfa_score_rows": (C.c_int, [_p, _i64, _i64, C.c_int, _p, _i64, _p, _p, _p, _i64, _p, _p, _i64, _p]),
}


bind(SYMBOLS, "sdfa_score_abi_version", ABI_VERSION, "score")


def sliding_samples(sr, win_size=0.064, hop_size=0.008, frames=64):
    """int(sr * (hop_size * (frames - 1) + win_size)): the dataset's window in samples (sliding_window.py:29,48)."""
    return int(sr * (hop_size * (frames - 1) + win_size))


def dataset_frame_starts(L, sr, fps=60, sliding=None):
    """The window starts the reference's dataset enumerates for a clip of L samples (sliding_window.py:45-61): margins of
    sr // 3 on both sides, `left += sr / fps` in double, ceil.  int64 [F]."""
    sliding = sliding_samples(sr) if sliding is None else int(sliding)
    extra = sr // 3
    delta = float(sr) / float(fps)
    end = int(L) + extra
    starts = []
    left = 0 - extra
    while left + sliding <= end:
        starts.append(math.ceil(left))
        left += delta
    return np.asarray(starts, np.int64)


def truth_plan(starts, sr, start_ts, minfi, maxfi, fps=60, ts_delta=100, sliding=None):
    """get_anime's index arithmetic (sliding_window.py:205-227) for the windows (start, start + sliding): which two track
    frames each animation frame blends and with which float32 weights.  Returns (src int64 [F][2] -- frame NUMBERS, as the
    track's files are named --, w float32 [F][2]).  Every operation after sample_to_ms's float32 result is a float32
    operation, as NumPy evaluates the reference's expressions on a float32 scalar; 1 - a is taken in double."""
    f32 = np.float32
    sliding = sliding_samples(sr) if sliding is None else int(sliding)
    l = np.asarray(starts, np.int64).reshape(-1)
    mid = (l + (l + sliding)) / 2                                        # true division: double
    ts = (mid * 1000.0 / float(sr)).astype(f32)                          # sample_to_ms
    ts = ts - f32(ts_delta) + f32(start_ts)
    pos = ts * f32(fps) / f32(1000.0)
    lower = np.floor(pos).astype(np.int64)
    upper = lower + 1
    below = lower < int(minfi)
    above = ~below & (upper > int(maxfi))
    lower = np.where(below, int(minfi), np.where(above, int(maxfi), lower))
    upper = np.where(below, int(minfi), np.where(above, int(maxfi), upper))
    a = pos - lower.astype(f32)
    w = np.stack(((1.0 - a.astype(np.float64)).astype(f32), a), axis=1)
    return np.stack((lower, upper), axis=1), np.ascontiguousarray(w)


def anime_weights(lips_dist, src, w):
    """anime_weight = exp((0.002 - dist) * 50) * 2 with dist blended like the rows (sliding_window.py:229-237): lips_dist
    float32 [n_track], src indices into it, float32 [F]."""
    d = np.asarray(lips_dist, np.float32).reshape(-1)
    dist = d[src[:, 0]] * w[:, 0] + d[src[:, 1]] * w[:, 1]
    return (np.exp((np.float32(0.002) - dist) * np.float32(50)) * np.float32(2)).astype(np.float32)


def score_rows(pred, track, src, w, clip_frame_off, layout):
    """pred [F][W] and track [n_track][W] float32 cuda, src [F][2] int64 and w [F][2] float32 (cuda, or host arrays that are
    uploaded), clip_frame_off [n_clips + 1] host integers -> the records [F][4] float64 on the device.  Stream-ordered."""
    assert torch.is_tensor(pred) and pred.is_cuda and pred.dtype == torch.float32, "sdfa_amd.score takes cuda tensors: there is no CPU path"
    assert torch.is_tensor(track) and track.is_cuda and track.dtype == torch.float32 and track.device == pred.device
    dev = pred.device
    pred = pred.reshape(pred.shape[0], -1)
    track = track.reshape(track.shape[0], -1)
    assert pred.is_contiguous() and track.is_contiguous(), "rows must be contiguous (row stride W): they are read in place"
    F, W = int(pred.shape[0]), int(pred.shape[1])
    assert track.shape[1] == W, (track.shape, W)
    src = torch.as_tensor(src).to(device=dev, dtype=torch.int64).contiguous()
    w = torch.as_tensor(w).to(device=dev, dtype=torch.float32).contiguous()
    assert tuple(src.shape) == (F, 2) and tuple(w.shape) == (F, 2), (src.shape, w.shape, F)
    off = np.ascontiguousarray(np.asarray(clip_frame_off, np.int64).reshape(-1))
    assert off.size >= 2
    with torch.cuda.device(dev):
        need = int(check(lib.sdfa_score_workspace_bytes(F, W, int(layout))))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(F, 4, dtype=torch.float64, device=dev)
        check(lib.sdfa_score_rows(_ptr(pred), F, W, int(layout), _ptr(track), int(track.shape[0]), _ptr(src), _ptr(w), off.ctypes.data,
                                  off.size - 1, _ptr(out), _ptr(ws), need, _stream()))
    return out


def clip_scalars(out, clip_frame_off, n, weights=None):
    """Records [F][4] -> the reference's scalars, float64 on the host.  For a clip of F_c frames the validation samples are the
    pairs a = [0 .. F_c - 2, F_c - 2], b = [1 .. F_c - 1, F_c - 1] (sliding_window.py:66-76), collated as the batch [a; b]:
        scalar_ps = 1 / (2 F_c) sum_{k in a + b} w_k out[k][0] / n        scalar_ms = 1 / F_c sum_i (w_a_i + w_b_i) out[b_i][2] / n
    scalar_pr / scalar_mr from slots 1 / 3, scalar_ploss = ps + pr, scalar_mloss = ms + mr.  n = T for dgrad (the criterion
    sums a triangle's values and averages the triangles), W for plain.  Returns {"clips": [dict per clip], "corpus": dict},
    the corpus value being the mean over clips weighted by F_c."""
    rec = out.detach().cpu().numpy() if torch.is_tensor(out) else np.asarray(out)
    rec = np.asarray(rec, np.float64).reshape(-1, 4)
    off = np.asarray(clip_frame_off, np.int64).reshape(-1)
    wt = np.ones(rec.shape[0], np.float64) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    assert wt.shape[0] == rec.shape[0] == off[-1], (wt.shape, rec.shape, off[-1])
    clips = []
    for c in range(off.size - 1):
        f0, fc = int(off[c]), int(off[c + 1] - off[c])
        assert fc >= 2, f"clip {c} has {fc} frames, the motion loss needs at least 2"
        a = np.concatenate((np.arange(fc - 1), [fc - 2])) + f0
        b = np.concatenate((np.arange(1, fc), [fc - 1])) + f0
        ab = np.concatenate((a, b))
        ps, pr = ((wt[ab] * rec[ab, s] / n).sum() / (2 * fc) for s in (0, 1))
        ms, mr = (((wt[a] + wt[b]) * rec[b, s] / n).sum() / fc for s in (2, 3))
        clips.append({"scalar_ps": float(ps), "scalar_pr": float(pr), "scalar_ms": float(ms), "scalar_mr": float(mr),
                      "scalar_ploss": float(ps + pr), "scalar_mloss": float(ms + mr), "frames": fc})
    total = float(sum(c["frames"] for c in clips))
    corpus = {k: float(sum(c[k] * c["frames"] for c in clips) / total) for k in SCALAR_KEYS}
    return {"clips": clips, "corpus": corpus}
