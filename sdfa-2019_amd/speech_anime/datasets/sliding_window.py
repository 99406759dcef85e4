"""DatasetSlidingWindow -- speech_anime/datasets/sliding_window.py on the device.

Inference half: fetch_audio_features and the unit converters of speech_anime/datasets/speech_anime.py:128-164.

Training half: what the reference's data-loader workers do per sample (__getitem__, sliding_window.py:66-284, and collate,
:286-315), as one batch call.  draw_augment() restates __getitem__'s random draws in the reference's order for a
numpy.random.RandomState; TrainSet keeps the clips' audio and animation tracks on the device; train_batch() turns dataset indices
into the collated batch [a; b]: the augmented feature images through sdfa_amd.augment (csrc/frontend.hip
frontend_augment_kernel), the blended targets through sdfa_amd.score.truth_plan and sdfa_seek_rows, the loss weights through
sdfa_amd.score.anime_weights.  Not built: the csv / pickle reader (the caller hands over arrays), phoneme labels, feat_noise,
feat_tremolo, pink noise, and the reverberated / pitch-shifted sources (precomputed audio the reference's configurations leave off).
"""
import weakref

import numpy as np
import torch

from sdfa_amd import engine as _engine

# config/model/dgrad.py:14-23 (offsets.py has the same values): what hparams.audio.feature lacks is taken from here
TRAIN_DEFAULTS = dict(random_noise=0.01, random_reverb=False, random_preemph=0.95, random_pitch_shift=False,
                      random_mel_extra=[5, 4], random_mel_noise=None, random_mel_scale=0.15, random_mel_dropout=0.15,
                      random_mel_tremolo=None)
SOURCES = ("audio", "audio_denoised", "audio_8k", "audio_denoised_8k")        # sliding_window.py:131


class TrainSet:
    """The training clips on the device.  clips: per clip a dict with "sr" (the rate of "audio" / "audio_denoised"; the `_8k`
    sources are 8000 Hz), the four SOURCES as float32 arrays, "speaker_id", "start_ts", "anime_minfi", "anime_maxfi" (the csv's
    columns) and optionally "audio_samples" (default len(audio)).  tracks: per clip (rows float32 [n][W], lips_dist float32 [n]),
    row k being animation frame anime_minfi + k (the reference's numbered .npy files)."""

    def __init__(self, clips, tracks, sr, fps=60, device="cuda"):
        from sdfa_amd import augment, score
        assert len(clips) == len(tracks) and len(clips) > 0
        self.sr, self.fps, self.device = int(sr), int(fps), torch.device(device)
        self.clips = [{k: v for k, v in c.items() if k not in SOURCES} for c in clips]
        self.sliding = score.sliding_samples(self.sr)
        coords = []
        for ci, c in enumerate(clips):
            assert int(c["sr"]) == self.sr, f"sample_rate is not same! hparams {self.sr}, data {c['sr']}"      # sliding_window.py:103
            starts = score.dataset_frame_starts(int(c.get("audio_samples", len(c["audio"]))), self.sr, self.fps, self.sliding)
            coords += [(ci, int(s)) for s in starts]
        self.coordinates = np.asarray(coords, np.int64).reshape(-1, 2)
        # one flat buffer per rate; clip ci's source si is buffer clip ci * len(SOURCES) + si of ITS rate (absent ones stay empty)
        self.pcm = {}
        for rate in sorted({self.sr, 8000}):
            arrs = [np.asarray(c[s], np.float32).reshape(-1) if (8000 if s.endswith("_8k") else self.sr) == rate and s in c else np.zeros(0, np.float32)
                    for c in clips for s in SOURCES]
            self.pcm[rate] = augment.upload_clips(arrs, self.device) + (np.asarray([len(a) for a in arrs], np.int64),)
        rows = [np.asarray(t[0], np.float32).reshape(len(t[0]), -1) for t in tracks]
        self.width = rows[0].shape[1]
        self.track_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        for c, r in zip(clips, rows):
            assert r.shape[1] == self.width and len(r) >= int(c["anime_maxfi"]) - int(c["anime_minfi"]) + 1
        self.rows = torch.from_numpy(np.concatenate(rows)).to(self.device)
        self.lips = np.concatenate([np.asarray(t[1], np.float32).reshape(-1) for t in tracks])
        assert len(self.lips) == self.track_off[-1]

    def __len__(self):
        return len(self.coordinates)


class DatasetSlidingWindow:
    hparams = None
    _engine = None          # a bare front-end engine, created on demand
    _engine_ref = None      # weak reference to the model's engine (set by SaberSpeechDrivenAnimation.load_state_dict): the class must
                            # not keep a dropped model's weights and workspace alive

    # ---- units: same float32 roundings as the reference (speech_anime.py:128-164)
    @classmethod
    def ms_to_sample(cls, ms, sr=None, dtype=np.float32):
        sr = sr or cls.hparams.audio.sample_rate
        return dtype(float(ms * sr) / 1000.0)

    @classmethod
    def sample_to_ms(cls, sample, sr=None, dtype=np.float32):
        sr = sr or cls.hparams.audio.sample_rate
        return dtype(float(sample * 1000.0) / float(sr))

    @classmethod
    def frame_to_sample(cls, idx, sr=None, fps=None, dtype=np.float32):
        sr = sr or cls.hparams.audio.sample_rate
        fps = fps or cls.hparams.anime.fps
        return dtype(float(idx * sr) / float(fps))

    @classmethod
    def sample_to_frame(cls, sample, sr=None, fps=None, dtype=np.float32):
        sr = sr or cls.hparams.audio.sample_rate
        fps = fps or cls.hparams.anime.fps
        return dtype(float(sample * fps) / float(sr))

    @classmethod
    def frame_in_range(cls, frame_idx, sliding_size, start, end):
        return start + cls.frame_to_sample(frame_idx) + sliding_size <= end

    # ---- training half
    @staticmethod
    def convert_window(stt, end, sample_rate, sr):
        """_audio_features' window conversion for a source at another rate (sliding_window.py:413-424), `stt and end is not None`
        with its truthiness: a start of 0 takes the second branch."""
        if sample_rate == sr:
            return int(stt), int(end)
        if stt:
            length = int((end - stt) * sample_rate / sr)
            stt = int(stt * sample_rate / sr)
            return stt, stt + length
        return int(stt * sample_rate / sr), int(end * sample_rate / sr)

    @classmethod
    def draw_augment(cls, rng, n_samples_in_window, hparams=None, noise="numpy"):
        """One sample's random draws, in the order the reference's __getitem__ (sliding_window.py:84-203) and its two
        windowed_features calls (get_features.py:70-75, 114-119, 174-182) make them on np.random; rng is a
        numpy.random.RandomState (np.random's own generator type, so a RandomState seeded like np.random.seed gives the
        reference's values bit for bit).  n_samples_in_window: r - l of a coordinate at hparams.audio.sample_rate.
        noise: "numpy" draws both windows' white noise from rng where the reference does (parity with it); "device" draws
        none -- sdfa_amd.augment.white_noise makes it -- so every draw behind the first noise differs from the reference's
        stream, not from its distribution.  Returns a dict: shift, source, sr (the source's rate), noise_scale (0.0 = none),
        preemph, ex_feat, ex_time, scale (float64 [128]), dropout, trunck, pad_reflect, lower_freq, mask_idx, drop_zero,
        mask_thres, noise (two float32 arrays or None), cut (samples of each window's cut at the source's rate)."""
        hp = hparams if hparams is not None else cls.hparams
        f = lambda k: hp.audio.feature.get(k, TRAIN_DEFAULTS[k])
        sr_set, fps = hp.audio.sample_rate, hp.anime.fps
        for k in ("random_reverb", "random_pitch_shift"):
            if f(k):
                raise NotImplementedError(f"audio.feature.{k}: precomputed sources are not built")
        for k in ("random_mel_noise", "random_mel_tremolo"):
            if f(k) is not None:
                raise NotImplementedError(f"audio.feature.{k} is not built (both model configurations leave it off)")
        d = {}
        shifting = int(0.5 / fps * sr_set)                                       # :42, :85
        d["shift"] = int(rng.randint(-shifting, shifting + 1))
        d["source"] = str(rng.choice(list(SOURCES)))                             # :131-134
        d["sr"] = 8000 if d["source"].find("_8k") >= 0 else sr_set
        d["noise_scale"] = 0.0
        rand_noise = f("random_noise")
        if rand_noise is not None:                                               # :150-155
            assert rand_noise > 0
            if rng.choice(["none", "white"]) == "white":
                # the reference formats the scale into "white@<scale>" and parses it back: repr round-trips a double
                d["noise_scale"] = float(rng.uniform(rand_noise / 5, rand_noise))
        rand_preemph = f("random_preemph")
        d["preemph"] = float(rng.uniform(0, rand_preemph)) if rand_preemph is not None and rand_preemph > 0 else None   # :158-159
        d["ex_feat"] = d["ex_time"] = 0
        extra = f("random_mel_extra")
        if extra is not None:                                                    # :166-174
            d["ex_feat"] = int(rng.randint(-abs(extra[0]), abs(extra[0]) + 1))
            d["ex_time"] = int(rng.randint(-abs(extra[1]), abs(extra[1]) + 1))
        d["scale"] = None
        mel_scale = f("random_mel_scale")
        if mel_scale is not None:                                                # :176-184
            assert 0 <= mel_scale <= 0.2
            a = rng.uniform(-np.pi / 2, np.pi / 2)
            b = rng.uniform(0, np.pi)
            d["scale"] = np.exp(np.sin(np.linspace(0, np.pi * 2, num=hp.audio.mel.n_mels) * a + b) * mel_scale)
        drop = f("random_mel_dropout")
        d["dropout"] = float(rng.uniform(0, drop)) if drop is not None else None    # :192-195
        # ---- inside the first windowed_features call
        hop = int(d["sr"] * hp.audio.mel.hop_size)
        l, r = cls.convert_window(0, int(n_samples_in_window), d["sr"], sr_set)
        d["cut"] = (r - l) + 2 * d["ex_time"] * hop
        white = lambda: rng.normal(0, d["noise_scale"], d["cut"]).astype(np.float32)      # saber/data/audio/noise.py:32-33
        want_noise = noise == "numpy" and d["noise_scale"] > 0
        assert noise in ("numpy", "device"), noise
        n0 = white() if want_noise else None
        d["trunck"] = bool(rng.uniform() < 0.5)                                  # get_features.py:117-119
        d["pad_reflect"] = str(rng.choice(["reflect", "constant"])) == "reflect"
        d["lower_freq"] = bool(rng.uniform() < 0.5)
        d["mask_idx"], d["drop_zero"], d["mask_thres"] = np.zeros(0, np.int64), True, None
        if d["dropout"] is not None and d["dropout"] > 0:                        # get_features.py:173-182
            n_feat = hp.audio.mel.n_mels
            d["mask_idx"] = rng.choice(np.arange(n_feat), max(1, int(d["dropout"] * n_feat)))
            d["drop_zero"] = str(rng.choice(["zero", "max"])) == "zero"
            d["mask_thres"] = float(rng.uniform(0.3, 0.6))
        # ---- the second call reuses random_args and draws fresh noise only
        d["noise"] = (n0, white()) if want_noise else None
        return d

    @classmethod
    def train_batch(cls, clips, tracks, indices, rng, noise="device", hparams=None):
        """The collated training batch [a; b] of the reference's collate (sliding_window.py:286-315) for the dataset indices
        `indices`: sample k contributes row k (its window) and row B + k (the next window of its clip).  clips: a TrainSet (then
        tracks is None), or the lists TrainSet takes (uploaded for this call).  Returns a dict of device tensors: audio_feat
        (2B, 64, 128, 3), face_data (2B, W) -- the blended track rows --, anime_weight (2B,), speaker_id (2B,), frame_id (2B,),
        and the host list `draws` of draw_augment's results.  noise: see draw_augment; "numpy" uploads the reference's noise."""
        from sdfa_amd import augment, score
        from sdfa_amd._lib import lib, check
        from sdfa_amd._packed import ptr, stream
        hp = hparams if hparams is not None else cls.hparams
        ts = clips if isinstance(clips, TrainSet) else TrainSet(clips, tracks, hp.audio.sample_rate, hp.anime.fps, hp.get("device") or "cuda")
        assert ts.sr == hp.audio.sample_rate
        B, n_co = len(indices), len(ts.coordinates)
        win_l = np.zeros(2 * B, np.int64)            # shifted window starts at the dataset's rate, rows in [a; b] order
        clip_of, frame_id = np.zeros(2 * B, np.int64), np.zeros(2 * B, np.int64)
        draws, per_rate = [], {}
        for k, i in enumerate(indices):
            i, j = int(i), int(i) + 1
            if j == n_co or ts.coordinates[i, 0] != ts.coordinates[j, 0]:       # :70-76
                j = i
                i = j - 1
            ci = int(ts.coordinates[i, 0])
            assert ci == ts.coordinates[j, 0]
            d = cls.draw_augment(rng, ts.sliding, hp, noise)
            draws.append(d)
            hop = int(d["sr"] * hp.audio.mel.hop_size)
            for half, fr in ((0, i), (1, j)):
                row = half * B + k
                l = int(ts.coordinates[fr, 1]) + d["shift"]
                win_l[row], clip_of[row], frame_id[row] = l, ci, fr
                stt, end = cls.convert_window(l, l + ts.sliding, d["sr"], ts.sr)
                assert end - stt + 2 * d["ex_time"] * hop == d["cut"], (end - stt, d["cut"])
                per_rate.setdefault(d["sr"], []).append((row, ci * len(SOURCES) + SOURCES.index(d["source"]), stt, d, half))
        dev = ts.device
        feat = torch.empty((2 * B, 64, 128, 3), dtype=torch.float32, device=dev)
        for rate, items in sorted(per_rate.items()):
            pcm, off, ln, host_len = ts.pcm[rate]
            for _, c, _, d, _ in items:
                assert host_len[c] > 0, f"clip {c // len(SOURCES)} has no source {d['source']!r}"
            preemph = [hp.audio.mel.preemphasis if d["preemph"] is None else d["preemph"] for *_, d, _ in items]
            desc = augment.pack_desc([c for _, c, *_ in items], [s for _, _, s, *_ in items], [d["ex_time"] for *_, d, _ in items], preemph,
                                     [d["ex_feat"] for *_, d, _ in items], [d["lower_freq"] for *_, d, _ in items],
                                     [d["trunck"] for *_, d, _ in items], [d["pad_reflect"] for *_, d, _ in items],
                                     [d["mask_idx"] if d["drop_zero"] else [] for *_, d, _ in items])       # "max" does nothing in the reference
            augment.check_desc(desc, host_len)
            scale = None
            if any(d["scale"] is not None for *_, d, _ in items):
                scale = torch.from_numpy(np.stack([np.ones(128) if d["scale"] is None else d["scale"] for *_, d, _ in items]).astype(np.float32)).to(dev)
            nz, stride = None, augment.noise_samples(rate)
            scales = [d["noise_scale"] for *_, d, _ in items]
            if any(s > 0 for s in scales):
                if noise == "numpy":
                    h = np.zeros((len(items), stride), np.float32)
                    for r, (*_, d, half) in enumerate(items):
                        if d["noise"] is not None:
                            h[r, :d["cut"]] = d["noise"][half]
                    nz = torch.from_numpy(h).to(dev)
                else:
                    nz = augment.white_noise(len(items), stride, scales, device=dev)
            rows = torch.as_tensor([r for r, *_ in items], dtype=torch.int64, device=dev)
            feat[rows] = augment.augment_frontend(pcm, off, ln, desc, rate, nz, scale)
        # ---- targets and weights: get_anime (:205-240) per window
        src, w = np.zeros((2 * B, 2), np.int64), np.zeros((2 * B, 2), np.float32)
        for ci in np.unique(clip_of):
            c, sel = ts.clips[int(ci)], clip_of == ci
            s, ww = score.truth_plan(win_l[sel], ts.sr, c["start_ts"], c["anime_minfi"], c["anime_maxfi"], ts.fps, hp.anime.feature.ts_delta, ts.sliding)
            src[sel], w[sel] = s - int(c["anime_minfi"]) + ts.track_off[int(ci)], ww
        weight = score.anime_weights(ts.lips, src, w)
        d_src, d_w = torch.from_numpy(src).to(dev), torch.from_numpy(w).to(dev)
        face = torch.empty((2 * B, ts.width), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.sdfa_seek_rows(ptr(ts.rows), ts.width, ptr(d_src), ptr(d_w), 2 * B, ptr(face), stream()))
        spk = np.asarray([int(ts.clips[int(c)]["speaker_id"]) for c in clip_of], np.int64)
        return dict(audio_feat=feat, face_data=face, anime_weight=torch.from_numpy(weight).to(dev), speaker_id=torch.from_numpy(spk).to(dev),
                    frame_id=torch.from_numpy(frame_id).to(dev), sr=[d["sr"] for d in draws] * 2, draws=draws)

    # ---- hot path
    @classmethod
    def fetch_audio_features(cls, signal, hparams=None, as_numpy=True):
        """sliding_window.py:324-377: dict(tslist, energy (F,1,64), audio_feat (F,64,128,3)).

        `as_numpy=False` keeps audio_feat on the GPU (the reference always returns numpy)."""
        if hparams is not None and cls.hparams is None:
            cls.hparams = hparams
        hp = cls.hparams
        if torch.is_tensor(signal):
            signal = signal.detach().cpu().numpy()
        signal = np.asarray(signal, np.float32).reshape(-1)
        assert -1.0 <= signal.min() and signal.max() <= 1.0                      # :330
        sr = hp.audio.sample_rate
        fe = cls._frontend_engine()
        table = _engine.frame_index(len(signal), sr)                             # ONE enumeration per clip: front end and energy share it
        feat, tslists, _ = fe.mel_frontend([signal], sr, tables=[table])
        energy = cls._energy(signal, sr, table[0])
        return dict(tslist=tslists[0], energy=energy,
                    audio_feat=feat.cpu().numpy() if as_numpy else feat)

    @classmethod
    def use_engine(cls, engine):
        cls._engine_ref = weakref.ref(engine)

    @classmethod
    def _frontend_engine(cls):
        eng = cls._engine_ref() if cls._engine_ref is not None else None
        if eng is not None:
            return eng
        # a bare front end lives on the configured device (hparams.device; api.evaluate_model sets it per rank), else the CURRENT one
        want = (cls.hparams.get("device") if cls.hparams is not None else None) or None
        if cls._engine is None or (want is not None and cls._same_device(cls._engine.device, want) is False):
            cls._engine = _engine.FrontendOnly(device=want)
        return cls._engine

    @staticmethod
    def _same_device(have, want):
        """torch.device comparison with an index-less "cuda" meaning the CURRENT device (FrontendOnly normalises its own the same way):
        'cuda' against 'cuda:0' is the same card, not a reason to build a new front end -- and a new 0.7 GB workspace -- per call."""
        a, b = torch.device(have), torch.device(want)
        if a.type != b.type:
            return False
        if a.type != "cuda":
            return True
        cur = torch.cuda.current_device() if torch.cuda.is_available() else 0
        return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)

    @staticmethod
    def _energy(signal, sr, starts=None):
        """librosa.feature.rms(frame_length=win, hop_length=hop, center=False) per window (sliding_window.py:365).
        Carried in the result for interface parity; no model consumes it (model.py:443,487)."""
        win, hop, sliding = _engine.frame_geometry(sr)
        if starts is None:
            starts, _ = _engine.frame_index(len(signal), sr)
        L = len(signal)
        csum = np.concatenate([[0.0], np.cumsum(signal.astype(np.float64) ** 2)])
        a = starts[:, None] + hop * np.arange(64)[None, :]
        lo, hi = np.clip(a, 0, L), np.clip(a + win, 0, L)
        return np.sqrt((csum[hi] - csum[lo]) / win).astype(np.float32)[:, None, :]
