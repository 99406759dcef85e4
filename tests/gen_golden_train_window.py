"""Regenerates tests/golden/train_window.npz and tests/golden/META_train_window.json: what the reference's OWN training data path
returns for small seeded inputs.  tests/test_augment_ref64_cpu.py pins tests/augment_ref64.py to it, tests/test_train_batch_cpu.py
pins DatasetSlidingWindow.draw_augment to it, tests/test_gpu_augment.py compares train_batch with it.

    python -B tests/gen_golden_train_window.py          (needs the reference checkout; imported through oracle/ref_import.py)

Part A ("w<sr>_*"): DatasetSlidingWindow._audio_features -> get_features.windowed_features (speech_anime/datasets/
sliding_window.py:380-463, get_features.py:8-223) called directly at both model rates with every argument given (CASES below): each
ex_time extreme, ex_feat +-5 in every flag combination, noise, pre-emphasis, scale, dropout in both modes.
Part B ("b_*"): a two-clip synthetic dataset tree in a temporary directory (csv, `_audio` pickles, numbered .npy rows and
`_lips_dist` files) and DatasetSlidingWindow(hparams, training=True).__getitem__ under np.random.seed(s) for INDICES, with
windowed_features wrapped to record its arguments: the arguments, the features, the targets and the weights.

Third-party code the image lacks is RESTATED, not pinned (as oracle/ref_import.py does for librosa): librosa's mel filters and delta
by oracle/librosa_restate.py, and cv2.resize(INTER_LINEAR) by resize_f32 below -- a float32 restatement of OpenCV's rule for float
images (source coordinate (d + 0.5) scale - 0.5 in double rounded to float32, floor, float32 fraction, ends clamped with fraction 0,
the horizontal pass v[x0] (1 - fx) + v[x1] fx, then the vertical one).  META says so.

To stay small the fixture keeps, of every (64, 128, 3) image, channel 0 at the 16 columns COLS and the delta channels at the 4
columns DCOLS; the audio is not stored (sdfa_amd.synth.make_pcm regenerates it from the seeds in META)."""
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "sdfa-2019_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

COLS = np.array([0, 1, 2, 3, 4, 5, 13, 22, 31, 32, 41, 50, 58, 59, 60, 63])
DCOLS = np.array([0, 4, 31, 63])
SRS = (8000, 16000)
INDICES = (0, 1, 5, 11, 17, 23, 29, 36, 41, 47, 60, 74)       # dataset indices of part B; seed of index i is SEED0 + i
SEED0 = 4100
B_SR = 16000                                                    # hparams.audio.sample_rate of part B: the `_8k` sources take the conversion
B_CLIPS = ((9600, 70, "speechlike", "m0", 37.5, 3, 40), (7200, 74, "uniform", "f1", 0.0, 0, 30))   # samples, seed, kind, speaker, start_ts, minfi, maxfi
B_WIDTH = 18                                                    # two triangles of dgrad rows
SOURCES = ("audio", "audio_denoised", "audio_8k", "audio_denoised_8k")


def geometry(sr):
    win, hop = int(0.064 * sr), int(0.008 * sr)
    return win, hop, hop * 63 + win


def clip_a(sr):
    """(seed, samples, kind) of part A's clip."""
    return 60 + sr // 8000, int(0.9 * sr), "speechlike"


def cases(sr):
    """Part A: name -> dict(start, ex_time, ex_feat, lower_freq, trunck, pad_reflect, preemph, noise (scale or 0), scale (seed or 0),
    mask (row indices), drop_mode)."""
    win, hop, sliding = geometry(sr)
    L = clip_a(sr)[1]
    base = dict(start=1000, ex_time=0, ex_feat=0, lower_freq=False, trunck=False, pad_reflect=False, preemph=0.65, noise=0.0, scale=0,
                mask=[], drop_mode="zero")
    c = {"neutral": dict(base)}
    c["time-4_before_clip"] = dict(base, start=-300, ex_time=-4, preemph=0.3)
    c["time+4_past_end"] = dict(base, start=L - sliding + 200, ex_time=4, preemph=0.0)
    c["feat-5_lower"] = dict(base, ex_feat=-5, lower_freq=True)
    c["feat-5_upper"] = dict(base, ex_feat=-5)
    for lower in (True, False):
        for trunck in (False, True):
            for reflect in ((False,) if lower else (True, False)):
                name = "feat+5_" + ("lower" if lower else "upper") + ("_trunck" if trunck else "") + ("" if lower else ("_reflect" if reflect else "_constant"))
                c[name] = dict(base, ex_feat=5, lower_freq=lower, trunck=trunck, pad_reflect=reflect, start=1000 + 37 * len(c))
    c["all_zero_mode"] = dict(base, start=5 * hop + 3, ex_time=3, ex_feat=-2, lower_freq=True, preemph=0.9, noise=0.01, scale=7,
                              mask=[3, 3, 70, 127], drop_mode="zero")
    c["all_max_mode"] = dict(base, start=2 * hop - 1, ex_time=-2, ex_feat=3, trunck=True, pad_reflect=True, preemph=0.5, noise=0.004, scale=8,
                             mask=[0, 64], drop_mode="max")
    c["odd_base"] = dict(base, start=7 * hop + 11, ex_time=1, ex_feat=1, lower_freq=True, preemph=0.95)
    return c


def scale_curve(seed):
    """A feat_scale column as __getitem__ builds it (sliding_window.py:180-183), float64 (128, 1)."""
    rs = np.random.RandomState(seed)
    s = np.sin(np.linspace(0, np.pi * 2, num=128) * rs.uniform(-np.pi / 2, np.pi / 2) + rs.uniform(0, np.pi)) * 0.15
    return np.expand_dims(np.exp(s), 1)


def case_noise(sr, name, scale):
    """The noise a part-A case adds: float32, the longest cut's length, seeded by the case."""
    win, hop, _ = geometry(sr)
    seed = 9000 + sr // 8000 * 100 + sorted(cases(sr)).index(name)
    return np.random.RandomState(seed).normal(0, scale, 71 * hop + win).astype(np.float32)


def resize_f32(src, dsize, interpolation=None, **k):
    """cv2.resize(src, (width, height), interpolation=INTER_LINEAR) for a float32 (h, w) or (h, w, 1) image, restated in float32."""
    f32 = np.float32
    img = np.asarray(src, f32)
    if img.ndim == 3:
        assert img.shape[2] == 1
        img = img[:, :, 0]
    w_out, h_out = dsize

    def taps(n_in, n_out):
        d = np.arange(n_out, dtype=np.float64)
        f = ((d + 0.5) * (n_in / n_out) - 0.5).astype(f32)
        i0 = np.floor(f).astype(np.int64)
        f = (f - i0.astype(f32)).astype(f32)
        lo, hi = i0 < 0, i0 >= n_in - 1
        f[lo | hi] = 0
        i0[lo] = 0
        i0[hi] = n_in - 1
        return i0, np.minimum(i0 + 1, n_in - 1), f

    x0, x1, fx = taps(img.shape[1], w_out)
    y0, y1, fy = taps(img.shape[0], h_out)
    rows = (img[:, x0] * (f32(1) - fx) + img[:, x1] * fx).astype(f32)
    out = (rows[y0] * (f32(1) - fy)[:, None] + rows[y1] * fy[:, None]).astype(f32)
    assert out.dtype == f32 and out.shape == (h_out, w_out)
    return out


def keep(feat):
    """(64, 128, 3) -> (channel 0 at COLS, channels 1-2 at DCOLS)."""
    return np.ascontiguousarray(feat[COLS, :, 0]), np.ascontiguousarray(feat[DCOLS][:, :, 1:])


def part_a(out):
    import ref_import
    from sdfa_amd import synth
    for sr in SRS:
        hp, _, DSW = ref_import.load_reference("dgrad", sample_rate=sr)
        sys.modules["cv2"].resize = resize_f32
        DSW.hparams = hp
        seed, L, kind = clip_a(sr)
        pcm = synth.make_pcm(seed, L, kind)
        _, _, sliding = geometry(sr)
        for name, c in sorted(cases(sr).items()):
            rargs = dict(trunck=c["trunck"], pad_mode="reflect" if c["pad_reflect"] else "constant", lower_freq=c["lower_freq"],
                         mask_idx=np.asarray(c["mask"], np.int64), drop_mode=c["drop_mode"], mask_thres=0.45, signal_noise_start=0)
            feat, _, wav, _ = DSW._audio_features(
                pcm, c["start"], c["start"] + sliding, force_preemph=c["preemph"],
                signal_noise=case_noise(sr, name, c["noise"]) if c["noise"] else None, feat_extra=(c["ex_feat"], c["ex_time"]),
                feat_scale=scale_curve(c["scale"]) if c["scale"] else None, feat_dropout=0.1 if len(c["mask"]) else None,
                training=True, sample_rate=sr, random_args=rargs)
            assert feat.shape == (64, 128, 3) and feat.dtype == np.float32, (feat.shape, feat.dtype)
            assert len(wav) == sliding + 2 * c["ex_time"] * geometry(sr)[1]
            out[f"w{sr}_{name}.m"], out[f"w{sr}_{name}.d"] = keep(feat)
            print(sr, name, float(feat[..., 0].mean()))


def build_tree(root):
    """The synthetic dataset: train.csv, per clip a directory of numbered rows and lips distances and its `_audio` pickle.
    Returns what the tests need to rebuild the same inputs: per clip (track rows float32 [n][W], lips_dist float32 [n])."""
    from sdfa_amd import synth
    lines = ["npy_data_path:path,speaker:str,emotion:str,audio_samples:int,start_ts:float,anime_minfi:int,anime_maxfi:int"]
    tracks = []
    for ci, (L, seed, kind, spk, start_ts, minfi, maxfi) in enumerate(B_CLIPS):
        d = os.path.join(root, f"clip{ci}")
        os.makedirs(d)
        rs = np.random.RandomState(500 + ci)
        rows = rs.normal(0, 0.3, (maxfi - minfi + 1, B_WIDTH)).astype(np.float32)
        dist = rs.uniform(0.0, 0.03, (maxfi - minfi + 1,)).astype(np.float32)
        for k in range(maxfi - minfi + 1):
            np.save(os.path.join(d, f"{str(minfi + k).zfill(6)}.npy"), rows[k])
            np.save(os.path.join(d, f"{str(minfi + k).zfill(6)}_lips_dist.npy"), dist[k])
        audio = dict(sr=B_SR)
        for si, name in enumerate(SOURCES):
            audio[name] = synth.make_pcm(seed + si, L // 2 if name.endswith("_8k") else L, kind)
        with open(d + "_audio", "wb") as fp:
            pickle.dump(audio, fp)
        lines.append(f"clip{ci},{spk},neutral,{L},{start_ts},{minfi},{maxfi}")
        tracks.append((rows, dist))
    with open(os.path.join(root, "train.csv"), "w") as fp:
        fp.write("\n".join(lines) + "\n")
    return tracks


def part_b(out):
    import ref_import
    from sdfa_amd import synth
    hp, _, DSW = ref_import.load_reference("dgrad", sample_rate=B_SR)
    sys.modules["cv2"].resize = resize_f32
    from speech_anime.datasets import sliding_window as SW
    from speech_anime.datasets.speech_anime import SpeechAnimeDataset
    with tempfile.TemporaryDirectory() as root:
        tracks = build_tree(root)
        hp.dataset_anime.set_key("root", root)
        SpeechAnimeDataset.hparams = None
        DSW.hparams = hp                                        # load_reference left the subclass's own attribute at None
        ds = DSW(hp, training=True)
        assert len(ds) > max(INDICES), len(ds)
        coords = np.array([[c["data_id"], c["range"][0]] for c in ds.coordinates], np.int64)
        calls = []
        orig = SW.get_features.windowed_features

        def recording(**kw):
            given = kw.get("random_args")
            ret = orig(**kw)
            ra = ret[3]
            cfg = kw["audio_config"]
            name = [s for ci in range(len(B_CLIPS)) for s in SOURCES
                    if np.array_equal(kw["signal"], synth.make_pcm(B_CLIPS[ci][1] + SOURCES.index(s), B_CLIPS[ci][0] // 2 if s.endswith("_8k") else B_CLIPS[ci][0], B_CLIPS[ci][2]))]
            assert len(name) == 1, name
            sn = kw["signal_noise"]
            calls.append(dict(
                source=SOURCES.index(name[0]), sr=int(cfg.sample_rate), stt=int(kw["signal_stt"]), end=int(kw["signal_end"]),
                preemph=float(cfg.mel.preemphasis), noise_scale=0.0 if sn is None else float(sn.split("@")[1]),
                ex_feat=int(kw["feat_extra"][0]), ex_time=int(kw["feat_extra"][1]), feat_scale=np.asarray(kw["feat_scale"], np.float64).reshape(128),
                feat_dropout=float(kw["feat_dropout"]), trunck=bool(ra["trunck"]), pad_reflect=str(ra["pad_mode"]) == "reflect",
                lower_freq=bool(ra["lower_freq"]), mask_idx=np.asarray(ra["mask_idx"], np.int64), drop_zero=str(ra["drop_mode"]) == "zero",
                mask_thres=float(ra["mask_thres"]), reused=given is not None))
            return ret
        SW.get_features.windowed_features = recording
        try:
            for i in INDICES:
                np.random.seed(SEED0 + i)
                n0 = len(calls)
                item = ds[i]
                a, b = calls[n0:]
                assert not a["reused"] and b["reused"]
                out[f"b{i}.int"] = np.array([[c["source"], c["sr"], c["stt"], c["end"], c["ex_feat"], c["ex_time"], c["trunck"], c["pad_reflect"],
                                              c["lower_freq"], c["drop_zero"]] for c in (a, b)], np.int64)
                out[f"b{i}.float"] = np.array([[c["preemph"], c["noise_scale"], c["feat_dropout"], c["mask_thres"]] for c in (a, b)], np.float64)
                out[f"b{i}.feat_scale"] = a["feat_scale"]
                out[f"b{i}.mask_idx"] = a["mask_idx"]
                assert np.array_equal(a["mask_idx"], b["mask_idx"]) and np.array_equal(a["feat_scale"], b["feat_scale"])
                for k in (0, 1):
                    out[f"b{i}.m{k}"], out[f"b{i}.d{k}"] = keep(item[f"audio_feat_{k}"])
                    out[f"b{i}.target{k}"] = np.concatenate([item[f"dgrad_3d_scale_{k}"][0], item[f"dgrad_3d_rotat_{k}"][0]], 1).reshape(-1).astype(np.float32)
                    assert item[f"anime_weight_{k}"].dtype == np.float32
                out[f"b{i}.weight"] = np.array([item["anime_weight_0"], item["anime_weight_1"]], np.float32).reshape(2)
                out[f"b{i}.ids"] = np.array([item["frame_id_0"], item["frame_id_1"], item["speaker_id"], item["sr"]], np.int64)
                print("index", i, "source", SOURCES[a["source"]], "ex", a["ex_feat"], a["ex_time"], "noise", a["noise_scale"], "mask", len(a["mask_idx"]))
        finally:
            SW.get_features.windowed_features = orig
    out["b_coords"] = coords
    for ci, (rows, dist) in enumerate(tracks):
        out[f"b_track{ci}"], out[f"b_lips{ci}"] = rows, dist


def main():
    out = {"cols": COLS, "dcols": DCOLS}
    part_a(out)
    part_b(out)
    path = os.path.join(HERE, "golden", "train_window.npz")
    np.savez_compressed(path, **out)
    meta = {
        "file": "train_window.npz",
        "generator": "tests/gen_golden_train_window.py",
        "source": "the reference's DatasetSlidingWindow._audio_features / get_features.windowed_features (part A, keys w<sr>_<case>) and "
                  "DatasetSlidingWindow(hparams, training=True).__getitem__ on a synthetic two-clip tree (part B, keys b<index>)",
        "restated_not_pinned": {
            "cv2.resize": "OpenCV is not installed where the fixture is generated: INTER_LINEAR for float images is restated in float32 "
                          "inside the generator (resize_f32); parity with the real library is not pinned",
            "librosa.filters.mel / librosa.feature.delta": "oracle/librosa_restate.py, as for every other fixture (oracle/ref_import.py)",
        },
        "kept": "channel 0 at columns `cols`, delta channels at columns `dcols` of each (64, 128, 3) image",
        "audio": "not stored: sdfa_amd.synth.make_pcm(seed, samples, kind)",
        "part_a": {str(sr): {"clip": list(clip_a(sr)), "cases": {k: v for k, v in sorted(cases(sr).items())}} for sr in SRS},
        "part_a_noise": "gen_golden_train_window.case_noise(sr, name, scale); scale curve: scale_curve(seed)",
        "part_b": {"sample_rate": B_SR, "clips": [list(c) for c in B_CLIPS], "sources": list(SOURCES), "source_seed": "clip seed + source index",
                   "width": B_WIDTH, "indices": list(INDICES), "seed": f"np.random.seed({SEED0} + index)",
                   "int_columns": ["source", "sr", "stt", "end", "ex_feat", "ex_time", "trunck", "pad_reflect", "lower_freq", "drop_zero"],
                   "float_columns": ["preemph", "noise_scale", "feat_dropout", "mask_thres"],
                   "ids": ["frame_id_0", "frame_id_1", "speaker_id", "sr"]},
    }
    with open(os.path.join(HERE, "golden", "META_train_window.json"), "w") as fp:
        json.dump(meta, fp, indent=1)
        fp.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
