"""Temporal filters of per-frame tracks on the GPU: host side of sdfa_track_fir / sdfa_track_bilateral in libsdfa_hip.so
(csrc/tfilter.hip and api_tfilter.cpp, C ABI in include/sdfa_tfilter.h).

correlate_symmetric() is bit for bit scipy.ndimage.correlate1d(rows, taps, axis=0, mode="reflect") for float32 rows and
symmetric float64 taps, gaussian_filter1d() hence scipy's gaussian_filter1d -- the smoothing step of the reference's
generate_dgrad (speech_anime/datasets/vocaset/preload.py:819).  bilateral() is the reference's BilateralFilter1D
(saber/utils/bilateral.py) evaluated in double.  A batch of clips is filtered clip by clip (clip_frame_off), never across
a boundary.  Every call is stream-ordered; arguments are checked on the host and touch no device when they are wrong.
A library without the symbols fails at import.  There is no CPU implementation."""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import bind, lib, check
from ._packed import ptr as _ptr, stream as _stream

ABI_VERSION = 1          # include/sdfa_tfilter.h SDFA_TFILTER_ABI_VERSION this binding was written against
MAX_RADIUS, WINDOW_RADIUS, COLS, RUN, CLIPS = 32, 8, 1024, 32, 512      # the header's SDFA_TFILTER_* constants
FLAG_GENERIC = 1

_p, _i64, _d = C.c_void_p, C.c_int64, C.c_double
SYMBOLS = {
    "sdfa_tfilter_abi_version": (C.c_int, []),
    "sdfa_track_fir": (C.c_int, [_p, _p, _i64, _i64, _p, _i64, _p, C.c_int, C.c_int, _p]),
    "sdfa_track_bilateral": (C.c_int, [_p, _p, _i64, _i64, _p, _i64, _d, _d, _d, C.c_int, _p, C.c_int, _p]),
}


bind(SYMBOLS, "sdfa_tfilter_abi_version", ABI_VERSION, "tfilter")


def gaussian_taps(sigma, truncate=4.0):
    """The kernel scipy.ndimage.gaussian_filter1d builds (order 0), by scipy's own numpy expression: float64 [2 lw + 1],
    lw = int(truncate * sigma + 0.5)."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma {sigma!r} must be finite and positive")
    lw = int(float(truncate) * sigma + 0.5)
    if not 0 <= lw <= MAX_RADIUS:
        raise ValueError(f"sigma {sigma} with truncate {truncate} gives radius {lw}, outside 0 .. {MAX_RADIUS}")
    sigma2 = sigma * sigma
    x = np.arange(-lw, lw + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def distance_weights(distance_sigma, radius, factor=-0.5):
    """BilateralFilter1D's distance table (bilateral.py:20-25) with Python's math.exp: float64 [2 radius + 1]."""
    ds, factor = float(distance_sigma), float(factor)
    table = []
    for idx in range(-int(radius), int(radius) + 1):
        delta = float(idx) / ds
        table.append(math.exp(delta * delta * factor))
    return np.asarray(table, np.float64)


def parse_filter(spec):
    """"gaussian:SIGMA" -> ("gaussian", {"sigma"}); "bilateral:DISTANCE_SIGMA,RANGE_SIGMA,RADIUS[,FACTOR]" -> ("bilateral",
    {"distance_sigma", "range_sigma", "radius", "factor"}).  Anything else raises ValueError."""
    if isinstance(spec, tuple) and len(spec) == 2 and spec[0] in ("gaussian", "bilateral") and isinstance(spec[1], dict):
        return spec
    if not isinstance(spec, str) or ":" not in spec:
        raise ValueError(f"filter {spec!r}: expected gaussian:SIGMA or bilateral:DISTANCE_SIGMA,RANGE_SIGMA,RADIUS[,FACTOR]")
    kind, _, rest = spec.partition(":")
    kind = kind.strip().lower()
    parts = [p.strip() for p in rest.split(",")]
    try:
        if kind == "gaussian":
            if len(parts) != 1:
                raise ValueError("one value")
            kw = {"sigma": float(parts[0])}
            gaussian_taps(kw["sigma"])
        elif kind == "bilateral":
            if len(parts) not in (3, 4):
                raise ValueError("three or four values")
            kw = {"distance_sigma": float(parts[0]), "range_sigma": float(parts[1]), "radius": int(parts[2]),
                  "factor": float(parts[3]) if len(parts) == 4 else -0.5}
            _check_bilateral(**kw)
        else:
            raise ValueError("unknown filter")
    except ValueError as e:
        raise ValueError(f"filter {spec!r}: {e}; expected gaussian:SIGMA or bilateral:DISTANCE_SIGMA,RANGE_SIGMA,RADIUS[,FACTOR]") from None
    return kind, kw


def _check_bilateral(distance_sigma, range_sigma, radius, factor):
    for name, v in (("distance_sigma", distance_sigma), ("range_sigma", range_sigma)):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{name} {v!r} must be finite and positive")
    if not math.isfinite(factor):
        raise ValueError(f"factor {factor!r} must be finite")
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius {radius} outside 0 .. {MAX_RADIUS}")


def _frame(rows, clip_frame_off, out):
    """The checks every filter shares -> (rows as (F, W), out as (F, W), the result in rows' shape, offsets or None)."""
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32):
        raise TypeError("sdfa_amd.tfilter takes float32 cuda tensors: there is no CPU path")
    if rows.dim() < 1 or rows.shape[0] < 1 or rows.numel() == 0:
        raise ValueError(f"rows of shape {tuple(rows.shape)}: at least one frame and one column")
    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous (row stride W): they are read in place")
    F = int(rows.shape[0])
    flat = rows.reshape(F, -1)
    if out is None:
        out = torch.empty_like(rows)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.device == rows.device
              and out.is_contiguous() and out.numel() == rows.numel()):
        raise ValueError("out must be a contiguous float32 cuda tensor of rows' size on rows' device")
    off = None
    if clip_frame_off is not None:
        off = np.ascontiguousarray(np.asarray(clip_frame_off, np.int64).reshape(-1))
        if off.size < 2 or off[0] != 0 or off[-1] != F or np.any(np.diff(off) <= 0):
            raise ValueError(f"clip_frame_off {off.tolist()[:8]}... must ascend strictly from 0 to {F}")
    return flat, out.reshape(F, -1), out, off


def correlate_symmetric(rows, taps, clip_frame_off=None, out=None, generic=False):
    """scipy.ndimage.correlate1d(rows, taps, axis=0, mode="reflect") per clip, bit for bit: rows float32 cuda (F, W) or
    (F, ...), taps 2 r + 1 bitwise symmetric float64 (r <= 32), clip_frame_off host integers from 0 to F (None: one clip).
    generic=True forces the form that re-reads its neighbours (the tests compare the two).  Returns out, in rows' shape."""
    taps = np.ascontiguousarray(np.asarray(taps, np.float64).reshape(-1))
    if taps.size % 2 != 1 or taps.size > 2 * MAX_RADIUS + 1:
        raise ValueError(f"{taps.size} taps: an odd number up to {2 * MAX_RADIUS + 1}")
    if taps.tobytes() != taps[::-1].tobytes():
        raise ValueError("taps are not bitwise symmetric")
    flat, oflat, out, off = _frame(rows, clip_frame_off, out)
    with torch.cuda.device(rows.device):
        check(lib.sdfa_track_fir(_ptr(flat), _ptr(oflat), flat.shape[0], flat.shape[1], None if off is None else off.ctypes.data,
                                 0 if off is None else off.size - 1, taps.ctypes.data, taps.size // 2,
                                 FLAG_GENERIC if generic else 0, _stream()))
    return out


def gaussian_filter1d(rows, sigma, truncate=4.0, clip_frame_off=None, out=None, generic=False):
    """scipy.ndimage.gaussian_filter1d(rows, sigma, axis=0, truncate=truncate) per clip, bit for bit."""
    return correlate_symmetric(rows, gaussian_taps(sigma, truncate), clip_frame_off, out, generic)


def bilateral(rows, distance_sigma=1.0, range_sigma=1.0, radius=5, factor=-0.5, clip_frame_off=None, out=None, generic=False):
    """BilateralFilter1D(factor, distance_sigma, range_sigma, radius)(rows) per clip, evaluated in double on the float32 rows
    and rounded once to float32.  Returns out, in rows' shape."""
    distance_sigma, range_sigma, radius, factor = float(distance_sigma), float(range_sigma), int(radius), float(factor)
    _check_bilateral(distance_sigma, range_sigma, radius, factor)
    dw = distance_weights(distance_sigma, radius, factor)
    flat, oflat, out, off = _frame(rows, clip_frame_off, out)
    with torch.cuda.device(rows.device):
        check(lib.sdfa_track_bilateral(_ptr(flat), _ptr(oflat), flat.shape[0], flat.shape[1], None if off is None else off.ctypes.data,
                                       0 if off is None else off.size - 1, factor, distance_sigma, range_sigma, radius,
                                       dw.ctypes.data, FLAG_GENERIC if generic else 0, _stream()))
    return out


def apply(spec, rows, clip_frame_off=None, out=None):
    """Runs the filter that parse_filter(spec) names."""
    kind, kw = parse_filter(spec)
    fn = gaussian_filter1d if kind == "gaussian" else bilateral
    return fn(rows, clip_frame_off=clip_frame_off, out=out, **kw)
