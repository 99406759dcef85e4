"""The reference's validation scalars of a checkpoint on a prepared data root: get_loss (speech_anime/model/model.py:261-330)
with PLoss and MLoss over the clips of the reference's info list, scored on the GPU (sdfa_amd.score).

    python -m speech_anime.validate --load_from CKPT --custom_hparams dgrad|offsets|hparams.json --valid_csv ROOT/valid.csv
                                    [--frames dataset] [--anime_loss_weight anime_weight]

The csv is the reference's info list: npy_data_path:path (a directory of NNNNNN.npy track frames, next to it the pickle
`<path>_audio` with {"sr", "audio"}), speaker:str, start_ts:float, anime_minfi:int, anime_maxfi:int, audio_samples:int.
Prints one JSON line: {"clips": [...], "corpus": {"scalar_ploss": ..., ...}}; scalar_ploss is what the reference picks
checkpoints by.  Absent: ELoss and DynamicLossScaler."""
import argparse
import csv
import json
import os
import pickle

import numpy as np

COLUMNS = ("npy_data_path:path", "speaker:str", "start_ts:float", "anime_minfi:int", "anime_maxfi:int", "audio_samples:int")


def load_track(data_dir, minfi, maxfi, suffix=""):
    """Frames minfi .. maxfi of one clip, {data_dir}/NNNNNN{suffix}.npy each, as float32 rows."""
    rows = [np.asarray(np.load(os.path.join(str(data_dir), f"{fi:06d}{suffix}.npy")), np.float32).reshape(-1) for fi in range(int(minfi), int(maxfi) + 1)]
    return np.stack(rows)


def read_valid_csv(csv_file, with_lips_dist=False):
    """The clips of an info list, as SaberSpeechDrivenAnimation.validate takes them (dicts; relative paths are taken from the
    csv's directory)."""
    with open(csv_file, newline="") as fp:
        rows = list(csv.DictReader(fp))
    missing = [c for c in COLUMNS if not rows or c not in rows[0]]
    if missing:
        raise ValueError(f"{csv_file}: no column {', '.join(missing)}")
    base = os.path.dirname(os.path.abspath(csv_file))
    clips = []
    for r in rows:
        path = r["npy_data_path:path"] if os.path.isabs(r["npy_data_path:path"]) else os.path.join(base, r["npy_data_path:path"])
        with open(path + "_audio", "rb") as fp:
            data = pickle.load(fp)
        minfi, maxfi, n = int(r["anime_minfi:int"]), int(r["anime_maxfi:int"]), int(r["audio_samples:int"])
        signal = np.asarray(data["audio"], np.float32).reshape(-1)
        if len(signal) != n:
            raise ValueError(f"{path}_audio holds {len(signal)} samples, the info list says {n}")
        clip = dict(signal=signal, sr=int(data["sr"]), speaker=r["speaker:str"], track=load_track(path, minfi, maxfi), start_ts=float(r["start_ts:float"]),
                    minfi=minfi, maxfi=maxfi, path=path)
        if with_lips_dist:
            clip["lips_dist"] = load_track(path, minfi, maxfi, "_lips_dist").reshape(-1)
        clips.append(clip)
    return clips


def validate_model(args):
    from .api import _load_checkpoint, build_model
    from .hparams import configure
    args = args if isinstance(args, dict) else vars(args)
    hparams = configure(args)
    if hparams.get("load_from") is None:
        raise ValueError("--load_from <checkpoint> is required for validation")
    clips = read_valid_csv(args["valid_csv"], with_lips_dist=args.get("anime_loss_weight") is not None)
    for c in clips:
        if c["sr"] != hparams.audio.sample_rate:              # sliding_window.py:103-104
            raise ValueError(f"sample_rate is not same! hparams {hparams.audio.sample_rate}, data {c['sr']}")
    ckpt = _load_checkpoint(os.path.expanduser(hparams.load_from))
    model = build_model(hparams, ckpt["state"])
    res = model.validate(clips, frames=args.get("frames") or "inference", anime_loss_weight=args.get("anime_loss_weight"))
    for c, r in zip(clips, res["clips"]):
        r["path"] = c["path"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m speech_anime.validate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--load_from", required=True)
    ap.add_argument("--custom_hparams", default=None)
    ap.add_argument("--log_dir", default=None)
    ap.add_argument("--valid_csv", required=True, help="the reference's info list of the held-out clips")
    ap.add_argument("--frames", choices=["inference", "dataset"], default="inference")
    ap.add_argument("--anime_loss_weight", choices=["anime_weight"], default=None)
    print(json.dumps(validate_model(ap.parse_args(argv))))


if __name__ == "__main__":
    main()
