"""Numpy restatements of the two temporal track filters exactly as include/sdfa_tfilter.h states them: fir_ref / gaussian_ref
(scipy's correlate1d with reflect boundaries, operation by operation in float64) and bilateral_ref (the reference's
BilateralFilter1D in float64).  Inputs are float32 (F, W) arrays -- or a list of 1-D arrays, as the reference passes --;
clip_frame_off cuts the frames into clips that are filtered independently."""
import numpy as np


def refl(i, n):
    """scipy's reflect, d c b a | a b c d | d c b a, for a clip of n frames; i: integer array, any depth of reflection."""
    p = 2 * n
    j = np.mod(np.asarray(i, np.int64), p)
    return np.where(j < n, j, p - 1 - j)


def gaussian_taps_ref(sigma, truncate=4.0):
    sd = float(sigma)
    lw = int(float(truncate) * sd + 0.5)
    x = np.arange(-lw, lw + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum()


def _clips(F, clip_frame_off):
    off = np.asarray([0, F] if clip_frame_off is None else clip_frame_off, np.int64)
    assert off[0] == 0 and off[-1] == F and np.all(np.diff(off) > 0), off
    return [(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


def fir_ref(x, taps, clip_frame_off=None):
    """acc = x[f] w[r]; for i = -r .. -1: acc = acc + (x[refl(f + i)] + x[refl(f - i)]) w[i + r]; float32(acc)."""
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    shape = x.shape
    x = x.reshape(shape[0], -1)
    w = np.asarray(taps, np.float64).reshape(-1)
    r = w.size // 2
    assert w.size == 2 * r + 1
    out = np.empty_like(x)
    for a, b in _clips(shape[0], clip_frame_off):
        xc = x[a:b].astype(np.float64)
        n = b - a
        f = np.arange(n)
        acc = xc * w[r]
        for i in range(-r, 0):
            acc = acc + (xc[refl(f + i, n)] + xc[refl(f - i, n)]) * w[i + r]
        out[a:b] = acc.astype(np.float32)
    return out.reshape(shape)


def gaussian_ref(x, sigma, truncate=4.0, clip_frame_off=None):
    return fir_ref(x, gaussian_taps_ref(sigma, truncate), clip_frame_off)


def bilateral_ref64(x, distance_sigma=1.0, range_sigma=1.0, radius=5, factor=-0.5, clip_frame_off=None):
    """The double values before the final rounding, (F, W) float64."""
    import math
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    shape = x.shape
    x = x.reshape(shape[0], -1)
    r, ds, rs, factor = int(radius), float(distance_sigma), float(range_sigma), float(factor)
    dw = [math.exp((float(d) / ds) * (float(d) / ds) * factor) for d in range(-r, r + 1)]
    out = np.empty(x.shape, np.float64)
    with np.errstate(all="ignore"):
        for a, b in _clips(shape[0], clip_frame_off):
            xc = x[a:b].astype(np.float64)
            n = b - a
            ws = np.zeros_like(xc)
            mean = np.zeros_like(xc)
            for d in range(-r, r + 1):
                lo, hi = max(0, -d), min(n, n - d)              # the frames f with 0 <= f + d < n
                if lo >= hi:
                    continue
                xn = xc[lo + d:hi + d]
                delta = xc[lo:hi] - xn
                s = np.sqrt(delta * delta) / rs
                sw = np.exp(s * s * factor)
                wt = dw[d + r] * sw
                ws[lo:hi] = ws[lo:hi] + wt
                mean[lo:hi] = mean[lo:hi] + wt * xn
            out[a:b] = mean / ws
    return out.reshape(shape)


def bilateral_ref(x, distance_sigma=1.0, range_sigma=1.0, radius=5, factor=-0.5, clip_frame_off=None):
    with np.errstate(all="ignore"):
        return bilateral_ref64(x, distance_sigma, range_sigma, radius, factor, clip_frame_off).astype(np.float32)
