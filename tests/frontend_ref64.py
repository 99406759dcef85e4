"""Float64 restatement of the front end (PCM + frame table -> (F, 64, 128, 3) log-mel + deltas), for judging the fp32 kernels of
csrc/frontend.hip element by element.

TEST INFRASTRUCTURE ONLY.  The operations follow oracle/sdfa_oracle.py (fetch_audio_features / frontend_windows) and the reference
lines it cites: zero-padded window cut, per-window pre-emphasis with y[0] = x[0], symmetric Hamming window, center=False STFT,
power, Slaney mel, 10 log10(max(m, eps)), (dB - 20 + 80) / 80 clamped to [0, 1], Savitzky-Golay deltas of width 9 whose edges
replicate the first / last interior value, (T, F, C) order.  The constants are the fp32 values the kernels use (Hamming window, mel
weights, float32(0.65)) promoted to float64; everything else is exact float64.  The spectrum is a plain float64 DFT matmul over a
win x (win/2 + 1) cos / sin matrix and the mel step the dense matrix over every bin, so nothing here shares an algorithm with the
kernels' Stockham transforms or their 8-tap mel table; nothing here calls a project kernel.

Besides the features, every call returns `kappa`, the error scale of each element for an fp32 front end of exact algorithm, derived
from the float64 quantities alone:
  * an fp32 FFT of a column of energy E = sum of its windowed, pre-emphasised samples squared errs by about u log2(win) sqrt(E) per
    bin; for a band of power m and weight sum W (the mel matrix's row sum) Cauchy-Schwarz gives dm / m <= 2 u log2(win) sqrt(E W / m);
  * the log maps dm / m onto the feature as 10 / (80 ln 10) = 0.0543 dm / m, the output's own rounding adds one ulp, and the clamp is
    1-Lipschitz (below m = 1e-6 the feature is clamped to 0: the floor of m):
        kappa_mel = u (1 + 2 * 0.0543 * log2(win) * sqrt(E W / max(m, 1e-6))),   u = 2^-24;
  * a delta channel: the root-sum-square sqrt(sum_k c_k^2 kappa_mel(t + k)^2) over its 9 taps, plus one ulp; the edge columns take
    their interior column's value.  (Against the reference's fp32 fixtures and the fp32 oracle its max |err| / kappa was 0.16 - 0.68
    where the linear sum_k |c_k| kappa_mel gave 0.12 - 0.39: the taps' errors are independent, and the closer fit is the sharper test.)

Pinned to the reference project's fixtures and to the fp32 oracle by tests/test_frontend_ref64_cpu.py.

The keyword arguments perturb the reference the way a plausible kernel bug would (see FrontendRef64.chunks); the GPU tests use them to
show that their bounds catch such a bug.
"""
import math

import numpy as np
import torch

from librosa_restate import mel_filters

F64 = torch.float64
U = 2.0 ** -24
LOG_SLOPE = 10.0 / (80.0 * math.log(10.0))            # d feature / d ln(m)
EPS = float(np.float32(1.1920929e-07))                 # torch.finfo(float32).eps, spectrogram.py:238
PREEMPH = float(np.float32(0.65))
SG1 = np.arange(-4, 5) / 60.0                           # librosa.feature.delta(order=1), width 9
SG2 = np.array([28, 7, -8, -17, -20, -17, -8, 7, 28], np.float64) / 462.0


def geometry(sr):
    """(win, hop, sliding): speech_anime/datasets/sliding_window.py:339-343 (64 columns of 64 ms every 8 ms)."""
    win, hop = int(0.064 * sr), int(0.008 * sr)
    return win, hop, hop * 63 + win


def dft_matrices(win, device="cpu"):
    """(cos, sin) of 2 pi n k / win, (win, win/2 + 1) float64; n k is reduced mod win in integers first."""
    n = torch.arange(win, dtype=torch.int64)
    k = torch.arange(win // 2 + 1, dtype=torch.int64)
    ang = (torch.outer(n, k) % win).to(F64) * (2.0 * math.pi / win)
    return torch.cos(ang).to(device), torch.sin(ang).to(device)


class FrontendRef64:
    def __init__(self, sr, device="cpu"):
        self.sr = sr
        self.device = device
        self.win, self.hop, self.sliding = geometry(sr)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=F64)
        self.hamm = t(np.hamming(self.win).astype(np.float32))                          # features/misc.py:94-100
        n = np.arange(self.win)
        self.hamm_periodic = t((0.54 - 0.46 * np.cos(2 * np.pi * n / self.win)).astype(np.float32))
        self.melw = t(mel_filters(sr, self.win, 128, 50, 3600).astype(np.float32))      # features/misc.py:110-117, (128, bins)
        self.cos, self.sin = dft_matrices(self.win, device)
        self.sg1, self.sg2 = t(SG1), t(SG2)

    # ------------------------------------------------------------------------------------------------------------------ pieces
    def spectrum(self, frames):
        """(..., win) float64 -> power (..., win/2 + 1): |sum_n x_n e^(-2 pi i n k / win)|^2 as two matrix products."""
        return (frames @ self.cos) ** 2 + (frames @ self.sin) ** 2

    def _clips(self, clips):
        pcm = [torch.as_tensor(np.asarray(c, np.float32).reshape(-1) if not torch.is_tensor(c) else c.detach().reshape(-1).float().cpu())
               for c in clips]
        lens = torch.tensor([len(c) for c in pcm], dtype=torch.int64)
        offs = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int64), lens[:-1]]), 0)
        flat = torch.cat(pcm + [torch.zeros(1)]).to(device=self.device, dtype=F64)
        return flat, offs.to(self.device), lens.to(self.device)

    @staticmethod
    def _samples(flat, off, ln, pos):
        """Clip samples at positions `pos` (any shape, per-row clip offset / length broadcast), zero outside [0, len)."""
        ok = (pos >= 0) & (pos < ln)
        return torch.where(ok, flat[torch.where(ok, off + pos, torch.zeros_like(pos))], torch.zeros((), dtype=F64, device=flat.device))

    def _deltas(self, m, zero_edges=False):
        """m (n, T, 128) -> (d1, d2): width-9 Savitzky-Golay along T; edges replicate the first / last interior value (or, with
        zero_edges, the taps read zeros beyond the ends)."""
        T = m.shape[1]
        if zero_edges:
            mp = torch.nn.functional.pad(m.transpose(1, 2), (4, 4)).transpose(1, 2)
            return [sum(c[j] * mp[:, j:j + T] for j in range(9)) for c in (self.sg1, self.sg2)]
        out = []
        for c in (self.sg1, self.sg2):
            acc = sum(c[j] * m[:, j:j + T - 8] for j in range(9))
            out.append(torch.cat([acc[:, :1].expand(-1, 4, -1), acc, acc[:, -1:].expand(-1, 4, -1)], 1))
        return out

    def _kappa_deltas(self, km):
        T = km.shape[1]
        out = []
        for c in (self.sg1, self.sg2):
            acc = torch.sqrt(sum(float(c[j]) ** 2 * km[:, j:j + T - 8] ** 2 for j in range(9))) + U
            out.append(torch.cat([acc[:, :1].expand(-1, 4, -1), acc, acc[:, -1:].expand(-1, 4, -1)], 1))
        return out

    # ------------------------------------------------------------------------------------------------------------------ frames
    @torch.no_grad()
    def chunks(self, clips, frame_clip, frame_start, chunk=256, preemph_col0=False, stale_col=None, mel_shift=None,
               delta_edge_zero=False, pad_off_by_one=False, periodic_hamming=False):
        """Yield (f0, f1, feat, kappa) over the frame table in chunks of `chunk` frames: feat, kappa (f1 - f0, 64, 128, 3) float64.

        Perturbations (each a plausible kernel bug):
          preemph_col0      column 0's first sample pre-emphasised with the sample before the window (the raw-first-sample rule lost)
          stale_col=(f, t)  column t of frame f replaced by the column one hop later (a stale ring slot of its chain)
          mel_shift=b       band b's filter taps moved up by one bin
          delta_edge_zero   the delta filters read zeros beyond the ends instead of replicating the interior edge values
          pad_off_by_one    frames that start before their clip: the zero / sample boundary one sample late (clip sample 0 dropped)
          periodic_hamming  0.54 - 0.46 cos(2 pi n / win) in place of the symmetric window's / (win - 1)
        """
        win, hop, sliding = self.win, self.hop, self.sliding
        flat, offs, lens = self._clips(clips)
        fc = torch.as_tensor(np.asarray(frame_clip.cpu() if torch.is_tensor(frame_clip) else frame_clip), dtype=torch.int64).to(self.device)
        fs = torch.as_tensor(np.asarray(frame_start.cpu() if torch.is_tensor(frame_start) else frame_start), dtype=torch.int64).to(self.device)
        hamm = self.hamm_periodic if periodic_hamming else self.hamm
        melw = self.melw
        if mel_shift is not None:
            melw = melw.clone()
            melw[mel_shift] = torch.roll(melw[mel_shift], 1)
            melw[mel_shift, 0] = 0
        W = melw.sum(1)
        lg = math.log2(win)
        ar = torch.arange(-1, sliding, device=self.device)
        T = (sliding - win) // hop + 1
        for f0 in range(0, len(fs), chunk):
            s = fs[f0:f0 + chunk, None]
            off, ln = offs[fc[f0:f0 + chunk]][:, None], lens[fc[f0:f0 + chunk]][:, None]
            pos = s + ar                                                               # sample before the window, then the window
            x = self._samples(flat, off, ln, pos)
            if pad_off_by_one:
                x = torch.where((s < 0) & (pos == 0), torch.zeros_like(x), x)
            y = x[:, 1:] - PREEMPH * x[:, :-1]                                         # features/misc.py:8-17
            if not preemph_col0:
                y[:, 0] = x[:, 1]
            fr = y.unfold(1, win, hop) * hamm                                          # (n, T, win), spectrogram.py:82-98
            E = (fr * fr).sum(-1)
            mel = self.spectrum(fr) @ melw.T                                           # (n, T, 128)
            if stale_col is not None and f0 <= stale_col[0] < f0 + len(s):
                u, t = stale_col[0] - f0, stale_col[1]
                p = s[u, 0] + (t + 1) * hop + torch.arange(-1, win, device=self.device)
                xs = self._samples(flat, off[u], ln[u], p)
                col = (xs[1:] - PREEMPH * xs[:-1]) * hamm
                mel[u, t] = self.spectrum(col) @ melw.T
                E[u, t] = (col * col).sum()
            db = 10.0 * torch.log10(torch.clamp(mel, min=EPS))                         # spectrogram.py:238,245-249
            m = torch.clamp((db - 20.0 + 80.0) / 80.0, 0.0, 1.0)
            d1, d2 = self._deltas(m, delta_edge_zero)                                   # get_features.py:199-223
            km = U * (1.0 + 2.0 * LOG_SLOPE * lg * torch.sqrt(E[..., None] * W / torch.clamp(mel, min=1e-6)))
            k1, k2 = self._kappa_deltas(km)
            assert m.shape[1] == T
            yield f0, f0 + len(s), torch.stack([m, d1, d2], -1), torch.stack([km, k1, k2], -1)

    def __call__(self, clips, frame_clip, frame_start, **kw):
        """The whole table at once: (feat, kappa), each (F, 64, 128, 3) float64."""
        parts = list(self.chunks(clips, frame_clip, frame_start, **kw))
        if not parts:
            z = torch.zeros((0, 64, 128, 3), dtype=F64, device=self.device)
            return z, z.clone()
        return torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts])


def frame_table(clips, sr, fps=60):
    """(frame_clip int32, frame_start int64) of the regular enumeration of every clip (sdfa_oracle.frame_index) at `fps`."""
    import sdfa_oracle as O
    fc, fs = [], []
    for ci, c in enumerate(clips):
        st, _ = O.frame_index(len(c), sr, fps=fps)
        fc.append(np.full(len(st), ci, np.int32))
        fs.append(st)
    return np.concatenate(fc), np.concatenate(fs)
