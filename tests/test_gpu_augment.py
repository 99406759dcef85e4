"""frontend_augment_kernel (csrc/frontend.hip, include/sdfa_augment.h) against the float64 restatement of tests/augment_ref64.py on
every element of every window, at 8 kHz (WIN = 512) and 16 kHz (WIN = 1024), and DatasetSlidingWindow.train_batch against what
the reference's own __getitem__ returned (tests/golden/train_window.npz part B).

Metric: r = max |gpu - ref64| / kappa with the propagated error scale of augment_ref64.py.  Bound: BOUND_R_PER_WINDOW of
tests/test_gpu_frontend_ref64.py (10 at 8 kHz, 16 at 16 kHz) -- the transform is that kernel's, the resize is a convex combination
and the gain one multiply, both charged by kappa: no new number.

Windows (about 50 per rate, windows() below) over three short clips -- 0.9 s, 0.35 s (shorter than a window) and one of length 0:
every ex_time; ex_feat +-5 in every flag combination and every other ex_feat with rotating flags; windows that start before sample
0, end past the end, lie wholly outside, on the short and on the empty clip; both hop-base parities; pre-emphasis 0, 0.65 and 0.95;
empty, single-row, duplicate-index and all-row dropout masks.  The batch runs in four launches: noise and scale present and null.

Exact assertions: neutral descriptors with preemph 0.65f give sdfa_mel_frontend's rows bitwise; dropped rows are 0 in all three
channels; windows with no sample and no noise are 0; everything is finite; batch order and batch size (1, 3, all) do not change a
window's bits; train_batch's targets and weights equal the reference's.  Each perturbation of augment_ref64.py lies above
SENS_MARGIN times the bound against the GPU's output; the control (frequency axis first) stays inside it.

Measured on an MI355X (pytest -s prints every figure): max |gpu - ref64| / kappa 1.15 at 8 kHz and 1.20 at 16 kHz over the four
launches (mel channel; deltas 0.54 at most); the perturbations 1.3e4 / 7.5e3 (preemph_first) to 4.6e6 / 5.2e6 (trunck_wrong_end),
drop_after_deltas infinite, the control 0.81 / 0.87; train_batch against the reference's recorded features 0.49 - 1.12.  The module
takes 5 s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "..", "oracle"), os.path.join(_HERE, "..", "sdfa-2019_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gen_golden_train_window as G                                            # noqa: E402
from augment_ref64 import CONTROL, PERTURBATIONS, AugmentRef64, ratio          # noqa: E402
from test_gpu_frontend_ref64 import BOUND_R_PER_WINDOW, SENS_MARGIN            # noqa: E402

pytestmark = pytest.mark.gpu
assert BOUND_R_PER_WINDOW == {8000: 10.0, 16000: 16.0} and SENS_MARGIN == 100

SRS = (8000, 16000)
CONFIGS = {"noise+scale": (True, True), "noise": (True, False), "scale": (False, True), "plain": (False, False)}
# the launch each perturbation is judged on: noise hides the one sample preemph_first changes and scale_first needs a scale, so
# everything runs without noise except the perturbation that moves the noise
JUDGED_ON = {p: ("noise+scale" if p == "noise_after_preemph" else "scale") for p in PERTURBATIONS}


def clips_of(sr):
    from sdfa_amd import synth
    return [synth.make_pcm(81, int(0.9 * sr), "speechlike"), synth.make_pcm(82, int(0.35 * sr)), np.zeros(0, np.float32)]


def windows(sr):
    """The descriptor fields of every window, as a dict of lists (AugmentRef64 and pack_desc both take it)."""
    win, hop, sliding = G.geometry(sr)
    L = int(0.9 * sr)
    w = []

    def add(start, clip=0, ex_time=0, preemph=0.65, ex_feat=0, flags=0, drop=()):
        w.append(dict(clip=clip, start=int(start), ex_time=ex_time, preemph=np.float32(preemph), ex_feat=ex_feat, lower_freq=bool(flags & 1),
                      trunck=bool(flags & 2), pad_reflect=bool(flags & 4), drop=list(drop)))
    for k, et in enumerate(range(-4, 5)):                                      # every ex_time; hop bases of both parities, off the grid too
        add(600 + k * (hop + 1) * 3, ex_time=et, preemph=(0.0, 0.95)[k & 1], ex_feat=(0, 2, -3)[k % 3], flags=k & 7)
    for ef in (-5, 5):                                                         # +-5 in every flag combination
        for flags in range(8):
            add(400 + 53 * flags, ex_feat=ef, flags=flags, preemph=0.3)
    for k, ef in enumerate((-4, -3, -2, -1, 0, 1, 2, 3, 4)):                   # every other ex_feat, flags rotating
        add(900 + 11 * k, ex_feat=ef, flags=(3 * k + 1) & 7, ex_time=(k % 3) - 1, preemph=0.95)
    add(2 * hop, preemph=0.5)                                                  # even hop base
    add(3 * hop, preemph=0.5)                                                  # odd hop base
    add(-3 * hop, ex_time=1)                                                   # hop base -4 - ... below zero: the floor division
    add(-hop - 1, ex_time=2, ex_feat=3, flags=4)                               # starts before sample 0, off the grid
    add(-sliding // 2, ex_time=-4, preemph=0.0)
    add(L - sliding // 2, ex_time=4, preemph=0.95, ex_feat=-5, flags=1)        # ends past the end
    add(L - sliding + 7, ex_time=3)
    add(-sliding - 5 * hop, ex_time=4)                                         # wholly outside, before
    add(L + 4 * hop, ex_time=4, ex_feat=5, flags=6)                            # wholly outside, behind
    add(L, ex_time=0)                                                          # the first sample behind the clip
    add(-hop * 20, clip=1, ex_time=2, preemph=0.95)                            # the short clip inside the cut
    add(100, clip=1, ex_time=-3, ex_feat=4, flags=5)
    add(0, clip=2, ex_time=1)                                                  # the empty clip
    add(-70, clip=2, ex_time=-4, ex_feat=-1, flags=1, drop=[5])
    add(1500, drop=[])                                                         # dropout masks: empty, one row, duplicates, all rows
    add(1500, drop=[77], ex_time=1)
    add(1500, drop=[3, 3, 70, 127, 70, 0], ex_feat=2, flags=2)
    add(1500, drop=range(128), ex_time=-1)
    return {k: [x[k] for x in w] for k in w[0]}


def empty_windows(sr, desc):
    """Windows whose cut holds no sample."""
    win, hop, sliding = G.geometry(sr)
    lens = np.array([len(c) for c in clips_of(sr)])[np.asarray(desc["clip"])]
    et = np.asarray(desc["ex_time"])
    lo = np.asarray(desc["start"]) - et * hop
    hi = lo + sliding + 2 * et * hop
    return (hi <= 0) | (lo >= lens)


def side_inputs(sr, n):
    from sdfa_amd import augment
    stride = augment.noise_samples(sr) + 3                                     # not the least stride
    rs = np.random.RandomState(sr + 9)
    noise = (rs.normal(0, 1, (n, stride)) * rs.choice([0.002, 0.01], (n, 1))).astype(np.float32)
    scale = np.stack([G.scale_curve(300 + i).reshape(128) for i in range(n)]).astype(np.float32)
    return noise, scale


def launch(sr, desc, noise, scale, rows=None):
    """One sdfa_augment_frontend call on the windows `rows` (default all) -> (len(rows), 64, 128, 3) on the device."""
    from sdfa_amd import augment
    pcm, off, ln = augment.upload_clips(clips_of(sr))
    rows = np.arange(len(desc["start"])) if rows is None else np.asarray(rows)
    d = augment.pack_desc(**{k: [v[i] for i in rows] for k, v in desc.items()})
    nz = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise[rows])).cuda()
    sc = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale[rows])).cuda()
    out = augment.augment_frontend(pcm, off, ln, d, sr, nz, sc)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def measured():
    out = {}
    for sr in SRS:
        desc = windows(sr)
        n = len(desc["start"])
        noise, scale = side_inputs(sr, n)
        ref = AugmentRef64(sr, device="cuda")
        m = dict(desc=desc, n=n, noise=noise, scale=scale, ref=ref, got={}, r={}, feat={}, kappa={})
        for name, (with_noise, with_scale) in CONFIGS.items():
            nz, sc = (noise if with_noise else None), (scale if with_scale else None)
            got = launch(sr, desc, nz, sc)
            feat, kappa = ref(clips_of(sr), desc, nz, sc)
            m["got"][name], m["feat"][name], m["kappa"][name] = got, feat, kappa
            m["r"][name] = ratio(got.double() - feat, kappa).flatten(1).max(1).values.cpu().numpy()
        out[sr] = m
    return out


@pytest.mark.parametrize("sr", SRS)
def test_against_float64(measured, sr):
    m = measured[sr]
    for name, r in m["r"].items():
        ch = ratio(m["got"][name].double() - m["feat"][name], m["kappa"][name]).reshape(-1, 3).max(0).values.tolist()
        print(f"\n{sr} {name}: {m['n']} windows, max |gpu - ref64| / kappa = {r.max():.2f} (window {int(r.argmax())}; channels {ch[0]:.2f} {ch[1]:.2f} {ch[2]:.2f}), "
              f"bound {BOUND_R_PER_WINDOW[sr]}")
    for name, r in m["r"].items():
        assert r.max() <= BOUND_R_PER_WINDOW[sr], (name, int(r.argmax()), r.max())


@pytest.mark.parametrize("sr", SRS)
def test_exact_zeros_and_finite(measured, sr):
    m = measured[sr]
    desc = m["desc"]
    empty = empty_windows(sr, desc)
    assert 4 <= empty.sum() < m["n"]
    dropped = [(i, r) for i, rows in enumerate(desc["drop"]) for r in set(rows)]
    assert len(dropped) >= 128 + 5
    for name, got in m["got"].items():
        assert bool(torch.isfinite(got).all()), name
        for i, r in dropped:
            assert not bool(got[i, :, r, :].any()), (name, i, r)
        if not CONFIGS[name][0]:                                               # no noise: a cut without a sample is silence
            assert not bool(got[torch.from_numpy(empty).cuda()].any()), name
        else:
            assert bool(got[torch.from_numpy(empty).cuda()].any()), name       # and with noise it is not
    some = [i for i, rows in enumerate(desc["drop"]) if 0 < len(set(rows)) < 128 and not empty[i] and desc["clip"][i] == 0]
    assert some and all(bool(m["got"]["plain"][i].any()) for i in some)


@pytest.mark.parametrize("sr", SRS)
def test_neutral_is_mel_frontend_bitwise(sr):
    from sdfa_amd import augment
    from sdfa_amd._lib import lib, check
    win, hop, sliding = G.geometry(sr)
    clips = clips_of(sr)
    L = len(clips[0])
    starts = np.array([0, 1, hop, 2 * hop, 3 * hop + 5, -1, -hop, -3 * hop, -sliding + 1, -sliding, 1234, L - sliding, L - sliding + 1, L - 1, L,
                       -100, 200, 0, -5], np.int64)
    clip = np.array([0] * 15 + [1, 1, 2, 2], np.int32)
    pcm, off, ln = augment.upload_clips(clips)
    want = torch.empty((len(starts), 64, 128, 3), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    d_fc, d_fs = torch.from_numpy(clip).cuda(), torch.from_numpy(starts).cuda()
    check(lib.sdfa_mel_frontend(p(pcm), p(off), p(ln), len(clips), p(d_fc), p(d_fs), len(starts), sr, p(want),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = augment.augment_frontend(pcm, off, ln, augment.pack_desc(clip, starts, preemph=np.float32(0.65), lower_freq=True, trunck=True, pad_reflect=True), sr)
    torch.cuda.synchronize()
    assert bool(want[:15].any())
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("sr", SRS)
def test_batch_order_and_size_do_not_change_a_window(measured, sr):
    m = measured[sr]
    full = m["got"]["noise+scale"]
    n = m["n"]
    perm = np.random.RandomState(sr).permutation(n)
    assert torch.equal(launch(sr, m["desc"], m["noise"], m["scale"], perm), full[torch.from_numpy(perm).cuda()])
    three = [5, n - 1, 17]
    assert torch.equal(launch(sr, m["desc"], m["noise"], m["scale"], three), full[three])
    for i in (0, 20, n - 2):
        assert torch.equal(launch(sr, m["desc"], m["noise"], m["scale"], [i]), full[i:i + 1])


@pytest.mark.parametrize("name", PERTURBATIONS)
def test_bound_catches(measured, name):
    for sr in SRS:
        m = measured[sr]
        cfg = JUDGED_ON[name]
        nz, sc = (m["noise"] if CONFIGS[cfg][0] else None), (m["scale"] if CONFIGS[cfg][1] else None)
        feat, kappa = m["ref"](clips_of(sr), m["desc"], nz, sc, **{name: True})
        bad = float(ratio(m["got"][cfg].double() - feat, kappa).max())
        good = float(m["r"][cfg].max())
        print(f"\n{sr} {name} on {cfg}: {bad:.3g} (unperturbed {good:.2f})")
        assert good <= BOUND_R_PER_WINDOW[sr]
        if name == CONTROL:
            assert bad <= BOUND_R_PER_WINDOW[sr], (sr, bad)
        else:
            assert bad > SENS_MARGIN * BOUND_R_PER_WINDOW[sr], (sr, name, bad)


def test_train_batch_against_the_reference_getitem(golden):
    """The fixture's synthetic tree, one train_batch call per recorded index with the reference's seed and noise="numpy": the
    features within the bound of the window's rate on the kept elements (kappa from ref64 on the same draws), the targets and
    weights bit for bit (the tolerance of the blend in tests/test_gpu_score.py: sdfa_seek_rows is score_ref64.blend32 exactly)."""
    from sdfa_amd import augment, synth
    from speech_anime import hparams as H
    from speech_anime.datasets.sliding_window import SOURCES, DatasetSlidingWindow as DSW, TrainSet
    g = golden["train_window"]
    hp = H.configure({"custom_hparams": "dgrad"})
    hp.audio.set_key("sample_rate", G.B_SR)
    clips, tracks = [], []
    for ci, (L, seed, kind, spk, start_ts, minfi, maxfi) in enumerate(G.B_CLIPS):
        c = dict(sr=G.B_SR, speaker_id=H.DEFAULTS["dataset_anime"]["speakers"][spk], start_ts=start_ts, anime_minfi=minfi, anime_maxfi=maxfi)
        for si, s in enumerate(SOURCES):
            c[s] = synth.make_pcm(seed + si, L // 2 if s.endswith("_8k") else L, kind)
        clips.append(c)
        tracks.append((g[f"b_track{ci}"], g[f"b_lips{ci}"]))
    ts = TrainSet(clips, tracks, G.B_SR)
    assert np.array_equal(ts.coordinates, g["b_coords"])
    refs = {sr: AugmentRef64(sr, device="cuda") for sr in SRS}
    cols, dcols = g["cols"], g["dcols"]
    rates = set()
    for index in G.INDICES:
        b = DSW.train_batch(ts, None, [index], np.random.RandomState(G.SEED0 + index), noise="numpy", hparams=hp)
        torch.cuda.synchronize()
        d = b["draws"][0]
        rates.add(d["sr"])
        assert tuple(b["audio_feat"].shape) == (2, 64, 128, 3) and b["frame_id"].tolist() == g[f"b{index}.ids"][:2].tolist()
        assert b["speaker_id"].tolist() == [int(g[f"b{index}.ids"][2])] * 2
        ci = int(g["b_coords"][g[f"b{index}.ids"][0], 0])
        src_clip = clips[ci][d["source"]]
        for k in (0, 1):
            stt = int(g[f"b{index}.int"][k][2])
            desc = dict(clip=[0], start=[stt], ex_time=[d["ex_time"]], preemph=[np.float32(d["preemph"])], ex_feat=[d["ex_feat"]], lower_freq=[d["lower_freq"]],
                        trunck=[d["trunck"]], pad_reflect=[d["pad_reflect"]], drop=[d["mask_idx"] if d["drop_zero"] else []])
            nz = None if d["noise"] is None else d["noise"][k][None]
            _, kappa = refs[d["sr"]]([src_clip], desc, nz, d["scale"].astype(np.float32)[None])
            got = b["audio_feat"][k].cpu().numpy()
            rm = float(ratio(got[cols][:, :, 0] - g[f"b{index}.m{k}"], kappa[0].cpu()[cols][:, :, 0]).max())
            rd = float(ratio(got[dcols][:, :, 1:] - g[f"b{index}.d{k}"], kappa[0].cpu()[dcols][:, :, 1:]).max())
            print(f"\nindex {index} window {k} ({d['source']}, ex {d['ex_feat']} {d['ex_time']}): |gpu - reference| / kappa = {rm:.2f} (mel) {rd:.2f} (deltas)")
            assert max(rm, rd) <= BOUND_R_PER_WINDOW[d["sr"]], (index, k, rm, rd)
            assert np.array_equal(b["face_data"][k].cpu().numpy(), g[f"b{index}.target{k}"]), (index, k)
        assert np.array_equal(b["anime_weight"].cpu().numpy(), g[f"b{index}.weight"]), index
    assert rates == {8000, 16000}
    # one batch of several samples is the same rows in [a; b] order
    idx = list(G.INDICES[:5])
    rng = np.random.RandomState(7)
    many = DSW.train_batch(ts, None, idx, rng, noise="numpy", hparams=hp)
    rng = np.random.RandomState(7)
    for k, i in enumerate(idx):
        one = DSW.train_batch(ts, None, [i], rng, noise="numpy", hparams=hp)
        for key in ("audio_feat", "face_data", "anime_weight", "speaker_id", "frame_id"):
            assert torch.equal(one[key][0], many[key][k]) and torch.equal(one[key][1], many[key][len(idx) + k]), (key, i)
    dev = DSW.train_batch(ts, None, idx, np.random.RandomState(7), hparams=hp)                     # device noise: same shapes, finite
    assert tuple(dev["audio_feat"].shape) == (10, 64, 128, 3) and bool(torch.isfinite(dev["audio_feat"]).all())
    assert augment.white_noise(3, 16, [0.0, 1.0, 2.0])[0].abs().max() == 0
