"""The reference's "PCA of dgrad, offsets" step (speech_anime/datasets/vocaset/preload.py pca_dgrad / pca_offsets) on the
GPU: gathers the per-frame .npy tracks, uploads them in chunks and fits the bases with sdfa_amd.pca; writes the reference's
files, {out_root}/pca/[scale_|rotat_]{compT,means}.npy, float32.  Like the reference it skips, with a message, when the
files are there, and takes every `step`-th frame of each directory.

    python -m speech_anime.datasets.pca --dgrad_root ROOT | --offsets_root ROOT [--step N]

ROOT holds train.csv with an `npy_data_path:path` column, as the reference's prepared data roots do."""
import argparse
import csv
import os
import re
import sys

import numpy as np

CHUNK_BYTES = 1 << 30            # frames are uploaded in chunks of about this size and fitted as a chunk list
_FRAME = re.compile(r"-*\d+(_dgrad|_offsets)?\.npy$")      # the reference's  -*\d+\.npy  and the exporter's NNNNNN_dgrad.npy


def find_frames(data_dir, step=1):
    """The frame files under one directory, every `step`-th of them, in the reference's order: the tree is walked and the
    paths are sorted as strings (its find_files), so `i % step` picks the same frames.  Zero-padded names, which the
    reference's tools and the exporter write, are then in frame order; unpadded ones (7.npy, 10.npy) are not, there as here."""
    paths = sorted(os.path.join(root, n) for root, _, names in os.walk(data_dir) for n in names if _FRAME.fullmatch(n))
    return [p for i, p in enumerate(paths) if step <= 1 or i % step == 0]


def _csv_dirs(csv_file):
    with open(csv_file, newline="") as fp:
        rows = list(csv.DictReader(fp))
    if not rows or "npy_data_path:path" not in rows[0]:
        raise ValueError(f"{csv_file}: no npy_data_path:path column")
    base = os.path.dirname(os.path.abspath(csv_file))
    return [r["npy_data_path:path"] if os.path.isabs(r["npy_data_path:path"]) else os.path.join(base, r["npy_data_path:path"]) for r in rows]


def load_chunks(source, step=1, device="cuda"):
    """source -> a list of float32 cuda [F_c][W] chunks.  source: a list of directories of per-frame .npy files, a train.csv
    (or a root that holds one), a numpy array, a cuda tensor, or a list of arrays / tensors."""
    import torch

    def as_chunks(a):
        """Every `step`-th row of one array or tensor, in pieces of about CHUNK_BYTES.  A host array is cut before it is uploaded,
        so no piece larger than that is ever staged; a device tensor taken whole (step 1, float32, contiguous) is not copied."""
        t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
        t = t.reshape(t.shape[0], -1)[::max(1, step)]
        if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous():
            return [t]
        per = max(1, CHUNK_BYTES // (4 * max(1, t.shape[1])))
        return [t[r0:r0 + per].to(device=device, dtype=torch.float32).contiguous() for r0 in range(0, t.shape[0], per)]

    if torch.is_tensor(source) or isinstance(source, np.ndarray):
        return as_chunks(source)
    if isinstance(source, (str, os.PathLike)):
        source = str(source)
        if os.path.isdir(source) and os.path.exists(os.path.join(source, "train.csv")):
            source = os.path.join(source, "train.csv")
        source = _csv_dirs(source) if source.endswith(".csv") else [source]
    source = list(source)
    if source and not isinstance(source[0], (str, os.PathLike)):
        return [c for a in source for c in as_chunks(a)]
    paths = [p for d in source for p in find_frames(str(d), step)]
    if not paths:
        raise FileNotFoundError(f"no frame files (NNN.npy, NNNNNN_dgrad.npy) under {source}")
    width = int(np.load(paths[0]).size)
    per = max(1, CHUNK_BYTES // (4 * width))
    chunks = []
    for i0 in range(0, len(paths), per):
        part = paths[i0:i0 + per]
        host = torch.empty(len(part), width, dtype=torch.float32, pin_memory=True)
        buf = host.numpy()
        for r, p in enumerate(part):
            buf[r] = np.load(p).reshape(-1)
        chunks.append(host.to(device))
    return chunks


def _say(msg):
    print(msg, file=sys.stderr)


def _have(out_root, names):
    return all(os.path.exists(os.path.join(out_root, "pca", n)) for n in names)


def pca_offsets(source, out_root, step=1, n_components=0.97):
    """Fits the offsets basis and writes {out_root}/pca/compT.npy, means.npy.  Returns the fit, or None when skipped."""
    if _have(out_root, ("compT.npy", "means.npy")):
        _say("PCA of offsets is already calculated.")
        return None
    from sdfa_amd import pca
    fit = pca.fit_offsets(load_chunks(source, step), n_components)
    fit.save(out_root)
    _say(f"offsets: {fit.k} components explain {float(fit.explained_variance_ratio.sum()):.6f}; compT {tuple(fit.compT.shape)}")
    return fit


def pca_dgrad(source, out_root, step=1, n_components=0.97):
    """Fits the scale and rotat bases of interleaved dgrad frames and writes {out_root}/pca/{scale,rotat}_{compT,means}.npy.
    Returns (scale, rotat), or None when skipped."""
    if _have(out_root, ("scale_compT.npy", "scale_means.npy", "rotat_compT.npy", "rotat_means.npy")):
        _say("PCA of dgrad is already calculated.")
        return None
    from sdfa_amd import pca
    fits = pca.fit_dgrad(load_chunks(source, step), n_components)
    for name, fit in zip(("scale", "rotat"), fits):
        fit.save(out_root)
        _say(f"{name}: {fit.k} components explain {float(fit.explained_variance_ratio.sum()):.6f}; compT {tuple(fit.compT.shape)}")
    return fits


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m speech_anime.datasets.pca", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dgrad_root", help="data root with train.csv; writes pca/{scale,rotat}_{compT,means}.npy into it")
    ap.add_argument("--offsets_root", help="data root with train.csv; writes pca/compT.npy and pca/means.npy into it")
    ap.add_argument("--step", type=int, default=1, help="take every N-th frame of each directory")
    args = ap.parse_args(argv)
    if not args.dgrad_root and not args.offsets_root:
        ap.error("give --dgrad_root and / or --offsets_root")
    if args.offsets_root:
        pca_offsets(args.offsets_root, args.offsets_root, args.step)
    if args.dgrad_root:
        pca_dgrad(args.dgrad_root, args.dgrad_root, args.step)


if __name__ == "__main__":
    main()
