"""Float64 restatement of the augmented training-window front end (include/sdfa_augment.h stages 1-6; the reference's
speech_anime/datasets/get_features.py:8-223), for judging frontend_augment_kernel element by element.

TEST INFRASTRUCTURE ONLY.  Built on the pieces of tests/frontend_ref64.py (clip sampling, DFT matmul, dense mel matrix, delta
filters): the spectrum is a float64 matrix product and the frequency edit MATERIALISES the padded / cut image with np.pad-like
concatenations, so nothing here shares an algorithm with the kernel's Stockham transforms, its 8-tap mel table or its row map;
nothing here calls a project kernel.  The resize takes its source coordinates in float64: for the sizes in question (56 - 72
columns -> 64, 123 - 133 rows -> 128) the coordinate ((2 d + 1) n_in - n_out) / (2 n_out) is a small integer over a power of two,
so the float32 rounding the contract names is exact and both agree to the last bit.

Two roundings of the CONTRACT are applied as float32 because they define the input of what follows rather than an error of it:
cut + noise (stage 1 adds in float32) and the scale (rounded to float32 before it is used).

`kappa`, the error scale of each element for an fp32 implementation of exact algorithm:
  * kappa_mel of frontend_ref64.py for the T x 128 mel image; a padded row of zeros is exact: 0;
  * through the resize the maximum of the four contributing values plus one ulp (U) of the result;
  * times scale, plus U;
  * exactly 0 on dropped rows, in all three channels;
  * the deltas by frontend_ref64's root-sum-square rule.
ratio() divides by it with 0 / 0 = 0 and x / 0 = inf.

Perturbations, each a plausible kernel bug (AugmentRef64.window's keywords):
  no_half_pixel       resize with source coordinate d n_in / n_out
  freq_first          frequency axis resized before time: exact arithmetic commutes, so this is the CONTROL that must stay inside the bound
  one_sided           the cut extended by 2 ex_time hop at its end only, not by ex_time hop on both sides
  edge_replicate      np.pad "edge" in place of "reflect"
  trunck_wrong_end    trunck cuts the padded end again
  scale_first         the band gain applied to the mel rows before the frequency edit and the resize
  drop_after_deltas   the deltas computed from the undropped image; only channel 0 of a dropped row is zeroed
  noise_after_preemph noise added to the pre-emphasised cut
  preemph_first       the cut's first sample pre-emphasised with the clip sample in front of it
"""
import numpy as np
import torch

from frontend_ref64 import EPS, F64, LOG_SLOPE, U, FrontendRef64
import math

PERTURBATIONS = ("no_half_pixel", "freq_first", "one_sided", "edge_replicate", "trunck_wrong_end", "scale_first",
                 "drop_after_deltas", "noise_after_preemph", "preemph_first")
CONTROL = "freq_first"


def resize_axis(img, n_out, dim, half_pixel=True):
    """Bilinear resize of `img` along `dim` to n_out, OpenCV INTER_LINEAR rule: source coordinate (d + 0.5) n_in / n_out - 0.5,
    floor, fraction; both ends clamped with fraction 0.  Returns (resized, i0, i1) with the contributing source indices."""
    n_in = img.shape[dim]
    d = torch.arange(n_out, dtype=F64)
    s = (d + 0.5) * (n_in / n_out) - 0.5 if half_pixel else d * (n_in / n_out)
    i0 = torch.floor(s)
    f = s - i0
    i0 = i0.to(torch.int64)
    lo, hi = i0 < 0, i0 >= n_in - 1
    f = torch.where(lo | hi, torch.zeros_like(f), f)
    i0 = torch.where(lo, torch.zeros_like(i0), torch.where(hi, torch.full_like(i0, n_in - 1), i0))
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    shape = [1] * img.dim()
    shape[dim] = n_out
    f = f.reshape(shape).to(img.device)
    i0, i1 = i0.to(img.device), i1.to(img.device)
    return img.index_select(dim, i0) * (1.0 - f) + img.index_select(dim, i1) * f, i0, i1


def resize_image(img, kap, rows_out=128, cols_out=64, half_pixel=True, freq_first=False):
    """img, kap (R, T) -> (rows_out, cols_out): time axis (dim 1) first, then frequency (dim 0); kappa = max of the four
    contributing values + U."""
    order = (0, 1) if freq_first else (1, 0)
    out, k = img, kap
    for dim in order:
        n_out = cols_out if dim == 1 else rows_out
        out, i0, i1 = resize_axis(out, n_out, dim, half_pixel)
        k = torch.maximum(k.index_select(dim, i0), k.index_select(dim, i1))
    return out, k + U


def edit_rows(img, ex_feat, lower_freq, trunck, pad_reflect, edge_replicate=False, trunck_wrong_end=False, zero=0.0):
    """get_features.py:125-140 on an image whose dim 0 is the mel axis, as explicit cuts and concatenations."""
    e = int(ex_feat)
    if e < 0:
        return img[-e:] if lower_freq else img[:e]
    if e == 0:
        return img
    pad0 = torch.full((e,) + tuple(img.shape[1:]), zero, dtype=img.dtype, device=img.device)
    if lower_freq:
        out = torch.cat([pad0, img])
        if trunck:
            out = out[e:] if trunck_wrong_end else out[:-e]
        return out
    if pad_reflect:
        ext = img[-1:].expand(e, *img.shape[1:]) if edge_replicate else torch.flip(img[-1 - e:-1], [0])     # rows 126, 125, ...
    else:
        ext = pad0
    out = torch.cat([img, ext])
    if trunck:
        out = out[:-e] if trunck_wrong_end else out[e:]
    return out


class AugmentRef64:
    def __init__(self, sr, device="cpu"):
        self.fe = FrontendRef64(sr, device)
        self.sr, self.device = sr, device
        self.win, self.hop, self.sliding = self.fe.win, self.fe.hop, self.fe.sliding

    @torch.no_grad()
    def window(self, flat, off, ln, start, ex_time=0, preemph=0.65, ex_feat=0, lower_freq=False, trunck=False, pad_reflect=False,
               drop=(), noise=None, scale=None, **pert):
        """One window -> (feat, kappa) (64, 128, 3) float64.  flat / off / ln: FrontendRef64._clips' buffer and this clip's offset and
        length; noise: float32 array of at least the cut's length or None; scale: 128 values or None; drop: row indices."""
        for k in pert:
            assert k in PERTURBATIONS, k
        fe, win, hop, dev = self.fe, self.win, self.hop, self.device
        ex = int(ex_time)
        T = 64 + 2 * ex
        LEN = (T - 1) * hop + win
        w0 = int(start) if pert.get("one_sided") else int(start) - ex * hop
        a = float(np.float32(preemph))
        pos = w0 + torch.arange(-1, LEN, device=dev)
        x = fe._samples(flat, torch.as_tensor(off, device=dev), torch.as_tensor(ln, device=dev), pos)
        before, x = x[0], x[1:]
        nz = None if noise is None else torch.as_tensor(np.asarray(noise, np.float32)[:LEN]).to(dev)
        if nz is not None and not pert.get("noise_after_preemph"):
            x = (x.float() + nz).double()                                  # stage 1 adds in float32: the noisy cut IS an fp32 signal
        y = x.clone()
        y[1:] = x[1:] - a * x[:-1]
        if pert.get("preemph_first"):
            y[0] = x[0] - a * before
        if nz is not None and pert.get("noise_after_preemph"):
            y = y + nz.double()
        fr = (y.unfold(0, win, hop) * fe.hamm)[None]                       # (1, T, win)
        E = (fr * fr).sum(-1)
        mel = fe.spectrum(fr) @ fe.melw.T                                  # (1, T, 128)
        db = 10.0 * torch.log10(torch.clamp(mel, min=EPS))
        m = torch.clamp((db - 20.0 + 80.0) / 80.0, 0.0, 1.0)[0]            # (T, 128)
        W = fe.melw.sum(1)
        km = (U * (1.0 + 2.0 * LOG_SLOPE * math.log2(win) * torch.sqrt(E[..., None] * W / torch.clamp(mel, min=1e-6))))[0]
        sc = None if scale is None else torch.as_tensor(np.asarray(scale, np.float32).astype(np.float64)).to(dev)
        img, kap = m.T.contiguous(), km.T.contiguous()                     # (128, T): rows are mel bands, as the reference holds it
        if sc is not None and pert.get("scale_first"):
            img, kap = img * sc[:, None], kap * sc[:, None]
        kw = dict(edge_replicate=bool(pert.get("edge_replicate")), trunck_wrong_end=bool(pert.get("trunck_wrong_end")))
        img = edit_rows(img, ex_feat, lower_freq, trunck, pad_reflect, **kw)
        kap = edit_rows(kap, ex_feat, lower_freq, trunck, pad_reflect, **kw)
        img, kap = resize_image(img, kap, half_pixel=not pert.get("no_half_pixel"), freq_first=bool(pert.get("freq_first")))
        if sc is not None and not pert.get("scale_first"):
            img, kap = img * sc[:, None], kap * sc[:, None] + U
        rows = torch.as_tensor(sorted(set(int(r) for r in drop)), dtype=torch.int64, device=dev)
        full = img.clone()
        if len(rows):
            img[rows] = 0.0
            kap[rows] = 0.0
        src = full if pert.get("drop_after_deltas") else img
        mt = img.T[None]                                                   # (1, 64, 128)
        d1, d2 = fe._deltas(src.T[None].contiguous())
        k1, k2 = fe._kappa_deltas(kap.T[None].contiguous())
        if len(rows):
            k1[:, :, rows] = 0.0
            k2[:, :, rows] = 0.0
        return torch.stack([mt, d1, d2], -1)[0], torch.stack([kap.T[None], k1, k2], -1)[0]

    def __call__(self, clips, desc, noise=None, scale=None, **pert):
        """clips: list of float32 arrays; desc: a dict of arrays as sdfa_amd.augment.unpack_desc returns (clip, start, ex_time,
        preemph, ex_feat, lower_freq, trunck, pad_reflect, drop); noise [n][stride] / scale [n][128] numpy or None.
        -> (feat, kappa) (n, 64, 128, 3) float64."""
        flat, offs, lens = self.fe._clips(clips)
        n = len(desc["start"])
        feats, kaps = [], []
        for i in range(n):
            c = int(desc["clip"][i])
            f, k = self.window(flat, int(offs[c]), int(lens[c]), int(desc["start"][i]), int(desc["ex_time"][i]), desc["preemph"][i],
                               int(desc["ex_feat"][i]), bool(desc["lower_freq"][i]), bool(desc["trunck"][i]), bool(desc["pad_reflect"][i]),
                               desc["drop"][i], None if noise is None else noise[i], None if scale is None else scale[i], **pert)
            feats.append(f)
            kaps.append(k)
        if not feats:
            z = torch.zeros((0, 64, 128, 3), dtype=F64, device=self.device)
            return z, z.clone()
        return torch.stack(feats), torch.stack(kaps)


def ratio(err, kappa):
    """|err| / kappa elementwise with 0 / 0 = 0 and x / 0 = inf (kappa is exactly 0 where the value must be exactly 0)."""
    err = torch.as_tensor(err).abs().double()
    kappa = torch.as_tensor(kappa).double().to(err.device)
    r = err / torch.where(kappa > 0, kappa, torch.ones_like(kappa))
    return torch.where(kappa > 0, r, torch.where(err > 0, torch.full_like(r, float("inf")), torch.zeros_like(r)))
