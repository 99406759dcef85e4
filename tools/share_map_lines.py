"""CPU model of what the mapped layer-0 recurrence reads through the encoder's share map.  No GPU.

Features: oracle/sdfa_oracle.py fetch_audio_features of three 10 s clips (synth.make_pcm(i, 160000)), one chunk.  Two columns are equal
when their 384 words are (the device's hash + full compare amounts to that).  Three maps, each numbered as share.hip numbers it (owners
in t * Nc + n order, col_to_u = number of the owner):
  search  the rule of the retired per-frame search: the (p, d), n - 64 <= p < n, 1 <= d <= 63, with the most t for which column (n, t)
          equals column (p, t + d); ties to the nearest frame, then the smallest shift; links followed to the end
  group   every column's owner is the first column in t * Nc + n order with the same bits
  table   the frame table's rule: nearest earlier frame of the clip a whole number of hops back, window columns 6..58
The recurrence reads GX[row][col_to_u[t * Nc + n]] in 16-byte quads, 32 consecutive frames per half-wave request; the model counts the
128-byte lines (8 consecutive u) each request touches, per request and per 64-frame tile (2 half-waves x 64 steps), tiles that hold a
clip's first or last frame apart from the others."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import sdfa_oracle as O
from sdfa_amd import synth

SR, HOP = 16000, 128
feats = [O.fetch_audio_features(synth.make_pcm(i, 10 * SR), SR) for i in range(3)]
feat = np.concatenate([f["audio_feat"] for f in feats], 0).astype(np.float32)
clip = np.concatenate([np.full(len(f["starts"]), i) for i, f in enumerate(feats)])
start = np.concatenate([f["starts"] for f in feats])
N = feat.shape[0]
Nc = (N + 127) // 128 * 128
cols = np.ascontiguousarray(feat).reshape(N * 64, 384).view(np.uint32)
_, ident = np.unique(cols.view(np.dtype((np.void, 384 * 4))), return_inverse=True)
ident = ident.reshape(N, 64)                                         # content id of column (n, t)
T = np.arange(64)


def owners_search():
    prev, shift = np.full(N, -1), np.zeros(N, int)
    for n in range(1, N):
        lo = max(n - 64, 0)
        eq = ident[lo:n][:, None, :] == ident[n][None, :, None]      # [p - lo][t][tt]
        cnt = np.stack([eq[:, T[:64 - d], T[:64 - d] + d].sum(1) for d in range(1, 64)])      # [d - 1][p - lo]
        if cnt.max() == 0:
            continue
        ds, ps = np.nonzero(cnt == cnt.max())
        back, d = min(zip(n - (lo + ps), ds + 1))                   # ties: nearest frame, then smallest shift
        prev[n], shift[n] = n - back, d
    own = np.empty((N, 64), int)
    for n in range(N):
        for t in range(64):
            a, b = n, t
            while prev[a] >= 0 and b + shift[a] <= 63 and ident[a, b] == ident[prev[a], b + shift[a]]:
                a, b = prev[a], b + shift[a]
            own[n, t] = b * Nc + a
    return own


def owners_group():
    idx = (T[None, :] * Nc + np.arange(N)[:, None])                  # t-major index of (n, t)
    first = np.full(ident.max() + 1, np.iinfo(np.int64).max)
    np.minimum.at(first, ident.ravel(), idx.ravel())
    return first[ident]


def owners_table():
    prev, shift = np.full(N, -1), np.zeros(N, int)
    for n in range(N):
        for q in range(n - 1, max(n - 65, -1), -1):
            diff = start[n] - start[q]
            if clip[q] != clip[n] or diff <= 0 or diff > 52 * HOP:
                break
            if diff % HOP == 0:
                prev[n], shift[n] = q, diff // HOP
                break
    own = np.empty((N, 64), int)
    for n in range(N):
        for t in range(64):
            a, b = n, t
            while 6 <= b <= 58 and prev[a] >= 0 and b + shift[a] <= 58:
                a, b = prev[a], b + shift[a]
            own[n, t] = b * Nc + a
    return own


def report(name, own):
    idx = T[None, :] * Nc + np.arange(N)[:, None]
    flag = np.zeros(64 * Nc, int)
    flag[idx[own == idx]] = 1
    uid = np.cumsum(flag) - flag
    u = np.zeros((64, Nc), int)
    u[:, :N] = uid[own].T                                            # col_to_u[t][n]; padding frames read column 0
    lines = np.array([[len(np.unique(u[t, h:h + 32] >> 3)) for t in range(64)] for h in range(0, Nc, 32)])     # [half-wave][t]
    tile = lines.reshape(-1, 2, 64).sum((1, 2))
    edge = np.zeros(Nc // 64, bool)
    for n in range(N):
        if n == 0 or n == N - 1 or clip[n] != clip[n - 1] or clip[n] != clip[min(n + 1, N - 1)]:
            edge[n // 64] = True
    full = np.arange(Nc // 64) * 64 + 64 <= N
    print(f"{name:7s} distinct {flag.sum() / (64 * N):.4f}   lines per request: mean {lines[:N // 32].mean():.2f} max {lines.max()}   "
          f"lines per 64-frame tile: interior {tile[full & ~edge].min()}-{tile[full & ~edge].max()}, "
          f"with a clip's end {tile[full & edge].min()}-{tile[full & edge].max()}")


print(f"{N} frames of 3 clips, chunk of {Nc}; {ident.max() + 1} distinct columns of {64 * N}")
report("search", owners_search())
report("group", owners_group())
report("table", owners_table())
