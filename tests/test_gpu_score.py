"""GPU checks of the validation losses (sdfa_amd.score, include/sdfa_score.h) against the float64 restatement
tests/score_ref64.py -- the reference, never the code under test.  Every record of every case is held to the model within
the model's own per-frame bound, which follows from the float32 operations the terms are formed with (score_ref64.records):
no measured constant enters an assertion.  `_held` prints the largest |gpu - model| / bound of a case before it asserts.

Shapes are named by the kernel's tiling (score.COLS columns per slab = 1024 triangles, score.RUN frames per run): one short
of, equal to and one past a slab in both alignments (T % 4 == 0 takes the float4 path), three slabs, FLAME's T = 9,976;
clips of 2, RUN, RUN + 1 and 2 RUN + 1 frames, alone and three in one call."""
import numpy as np
import pytest
import torch

import score_ref64 as R
from test_score_ref64_cpu import refusals, call_refused

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make_case(layout, W, clip_lens, seed, clamp=()):
    """Seeded rows, a hand-made plan and the float32 truth.  Track rows run at the frame rate (60 fps against 60 fps): frame f of
    a clip blends rows f and f + 1 of its clip's stretch with weights (1 - a, a).  Frames listed in `clamp` take one row twice
    with weights (1, 0), as a clamped plan entry does."""
    rs = np.random.RandomState(seed)
    F = int(sum(clip_lens))
    off = np.concatenate(([0], np.cumsum(clip_lens))).astype(np.int64)
    n_track = F + len(clip_lens)
    track = R.tracks(n_track, W, seed, 0.3)
    src = np.zeros((F, 2), np.int64)
    for c, n in enumerate(clip_lens):
        src[off[c]:off[c + 1], 0] = off[c] + c + np.arange(n)
    src[:, 1] = src[:, 0] + 1
    a = rs.uniform(0, 1, F).astype(np.float32)
    a[::5] = 0
    w = np.stack(((1.0 - a.astype(np.float64)).astype(np.float32), a), 1)
    for f in clamp:
        src[f, 1] = src[f, 0]
        w[f] = (1, 0)
    truth = R.blend32(track, src, w)
    pred = (truth + R.tracks(F, W, seed + 1000, 0.1)).astype(np.float32)
    return dict(layout=layout, W=W, off=off, track=track, src=src, w=w, truth=truth, pred=pred)


def gpu_records(case, pred=None):
    from sdfa_amd import score
    lay = score.LAYOUT_DGRAD if case["layout"] == "dgrad" else score.LAYOUT_PLAIN
    p = torch.from_numpy(case["pred"] if pred is None else pred).to(DEV)
    rec = score.score_rows(p, torch.from_numpy(case["track"]).to(DEV), case["src"], case["w"], case["off"], lay)
    return rec.cpu().numpy()


def _held(name, got, case):
    rec, bound = R.records(case["pred"], case["truth"], case["off"], case["layout"])
    err = np.abs(got - rec)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"{name}: F {got.shape[0]} W {case['W']}: max |gpu - model| / bound = {ratio.max():.3g}, max relative error = "
          f"{(err / np.maximum(rec, 1e-300)).max():.3g}, max bound / record = {(bound / np.maximum(rec, 1e-300)).max():.3g}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (name, np.argwhere(err > bound)[:5], ratio.max())
    first = case["off"][:-1]
    assert (got[first, 2:] == 0).all(), "motion crossed a clip boundary"
    if case["layout"] == "plain":
        assert (got[:, 1] == 0).all() and (got[:, 3] == 0).all()
    else:
        assert (got[:, :2] > 0).all()
    return rec


def _slab_t():
    from sdfa_amd import score
    return score.COLS // 9


@pytest.mark.parametrize("T", ["1", "3", "4", "slab-1", "slab", "slab+1", "slab+4", "3*slab", "9976"])
def test_dgrad_widths(T):
    t = {"slab-1": _slab_t() - 1, "slab": _slab_t(), "slab+1": _slab_t() + 1, "slab+4": _slab_t() + 4, "3*slab": 3 * _slab_t()}.get(T) or int(T)
    case = make_case("dgrad", 9 * t, [5], 100 + t % 97, clamp=(3,))
    _held(f"dgrad T={t}", gpu_records(case), case)


@pytest.mark.parametrize("W", ["1", "15069", "slab+1"])
def test_plain_widths(W):
    from sdfa_amd import score
    w = score.COLS + 1 if W == "slab+1" else int(W)
    case = make_case("plain", w, [5], 200 + w % 89, clamp=(0, 4))
    _held(f"plain W={w}", gpu_records(case), case)


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("n", ["2", "run", "run+1", "2*run+1"])
def test_clip_lengths(n, T):
    from sdfa_amd import score
    fc = {"2": 2, "run": score.RUN, "run+1": score.RUN + 1, "2*run+1": 2 * score.RUN + 1}[n]
    case = make_case("dgrad", 9 * T, [fc], 300 + fc, clamp=(fc - 1,))
    _held(f"clip of {fc}, T={T}", gpu_records(case), case)
    plain = make_case("plain", 300, [fc], 400 + fc)
    _held(f"plain clip of {fc}", gpu_records(plain), plain)


@pytest.mark.parametrize("layout,W", [("dgrad", 36), ("dgrad", 45), ("plain", 77)])
def test_three_clips_in_one_call_equal_three_calls(layout, W):
    from sdfa_amd import score
    lens = [score.RUN + 1, 2, 2 * score.RUN + 1]                 # clips start inside runs, one run holds three clip starts
    case = make_case(layout, W, lens, 500 + W, clamp=(0, score.RUN, score.RUN + 2))
    got = gpu_records(case)
    _held(f"three clips {layout} W={W}", got, case)
    off = case["off"]
    for c in range(3):                                          # a clip's records do not depend on its neighbours
        f0, f1 = int(off[c]), int(off[c + 1])
        alone = dict(case, off=np.asarray([0, f1 - f0]), src=case["src"][f0:f1], w=case["w"][f0:f1], pred=case["pred"][f0:f1], truth=case["truth"][f0:f1])
        assert np.array_equal(gpu_records(alone), got[f0:f1])


@pytest.mark.parametrize("layout,W", [("dgrad", 9 * 1028), ("dgrad", 9 * 7), ("plain", 15069)])
def test_prediction_equal_to_truth_gives_exact_zeros(layout, W):
    case = make_case(layout, W, [3, 40], 600 + W % 50, clamp=(2,))
    got = gpu_records(case, pred=case["truth"])
    assert got.shape == (43, 4) and not got.any()


@pytest.mark.parametrize("layout,W", [("dgrad", 9 * 9976), ("dgrad", 45), ("plain", 15069)])
def test_same_call_twice_is_bitwise_equal(layout, W):
    case = make_case(layout, W, [4, 3], 700 + W % 50)
    a, b = gpu_records(case), gpu_records(case)
    assert np.array_equal(a, b) and a[:, 0].all()


@pytest.mark.parametrize("layout,W", [("dgrad", 72), ("dgrad", 45), ("plain", 50)])
def test_bad_plan_index_is_never_read_and_gives_nan(layout, W):
    case = make_case(layout, W, [6, 4], 800 + W)
    good = gpu_records(case)
    n_track = case["track"].shape[0]
    src = case["src"].copy()
    src[2, 1] = n_track                     # one past the track
    src[7, 0] = -1
    got = gpu_records(dict(case, src=src))
    assert np.isnan(got[[2, 7]]).all()
    motion = [2, 3] if layout == "dgrad" else [2]
    assert np.isnan(got[[3, 8]][:, motion]).all()                # their successors have no predecessor truth
    keep = np.ones_like(got, bool)
    keep[[2, 7]] = False
    keep[3, 2:] = keep[8, 2:] = False
    assert np.array_equal(got[keep], good[keep])


@pytest.mark.parametrize("name,a", refusals(), ids=[k for k, _ in refusals()])
def test_refusals_launch_nothing(name, a):
    from sdfa_amd import _lib
    out = torch.full((8, 4), -7.0, dtype=torch.float64, device=DEV)
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    # real device memory behind every pointer, the output among them: a launch would overwrite the sentinel
    rc = call_refused(_lib.lib, a, buf.data_ptr(), out.data_ptr())
    assert rc == _lib.EINVAL and _lib.lib.sdfa_last_error().decode().startswith("score_rows:"), name
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def _model(sd, head):
    from speech_anime.hparams import configure
    from speech_anime.model import SaberSpeechDrivenAnimation
    hp = configure(dict(mode="evaluate", custom_hparams=head))
    hp.audio.set_key("sample_rate", 8000)
    from speech_anime.datasets import DatasetSlidingWindow
    DatasetSlidingWindow.hparams = None
    m = SaberSpeechDrivenAnimation(hp, None, None, load_pca=False)
    m.load_state_dict(sd)
    return m


@pytest.mark.parametrize("head", ["dgrad", "offsets"])
def test_validate_end_to_end(synth_sd, head):
    """validate() on the synthetic head: one 2 s clip and one clip of the minimum length at 8 kHz.  The rows the engine wrote
    (keep_rows taps them) are scored by the model; the scalars agree within the model's bound carried through clip_scalars."""
    from sdfa_amd import score, synth
    from sdfa_amd.engine import frame_index
    model = _model(synth_sd[head], head)
    W = model._model._engine.out_dim
    layout = "dgrad" if head == "dgrad" else "plain"
    lens = (16000, 4544)
    clips = []
    for i, n in enumerate(lens):
        minfi, maxfi = (5, 60) if i == 0 else (0, 9)            # both clamps of the 2 s clip are met, the short clip clamps above
        track = (R.tracks(maxfi - minfi + 1, W, 40 + i, 0.01) if layout == "dgrad" else R.tracks(maxfi - minfi + 1, W, 40 + i, 0.001))
        clips.append(dict(signal=synth.make_pcm(60 + i, n), speaker=2 + i, track=track, start_ts=12.5 * i, minfi=minfi, maxfi=maxfi))
    res = model.validate(clips, keep_rows=True)
    counts = [len(frame_index(n, 8000)[0]) for n in lens]
    assert [c["frames"] for c in res["clips"]] == counts and res["clip_frame_off"].tolist() == [0, counts[0], sum(counts)]
    rows = res["rows"].cpu().numpy()
    src, w = res["plan"]
    assert (src[:, 0] == src[:, 1]).any() and (src[:, 0] != src[:, 1]).any()
    truth = R.blend32(res["track"].cpu().numpy(), src, w)
    rec, bound = R.records(rows, truth, res["clip_frame_off"], layout)
    got = res["records"].cpu().numpy()
    assert (np.abs(got - rec) <= bound).all()
    n = W // 9 if layout == "dgrad" else W
    want = score.clip_scalars(rec, res["clip_frame_off"], n)
    slack = score.clip_scalars(bound, res["clip_frame_off"], n)          # the scalars are non-negative combinations of the records
    for c, (a, b, s) in enumerate(zip(res["clips"], want["clips"], slack["clips"])):
        f0, f1 = res["clip_frame_off"][c:c + 2]
        model64 = R.criterion64(rows[f0:f1], truth[f0:f1], None, layout)
        for k in score.SCALAR_KEYS:
            print(head, c, k, a[k], b[k], s[k])
            assert abs(a[k] - b[k]) <= s[k] + 1e-15 * b[k]
            assert abs(b[k] - model64[k]) <= 1e-12 * max(model64[k], 1e-300)
        assert a["scalar_ploss"] > 0 and a["scalar_mloss"] > 0
    for k in score.SCALAR_KEYS:
        assert res["corpus"][k] == pytest.approx(sum(c[k] * c["frames"] for c in res["clips"]) / sum(counts), rel=1e-14)
    ds = model.validate(clips, frames="dataset")
    assert [c["frames"] for c in ds["clips"]] == [len(score.dataset_frame_starts(n, 8000)) for n in lens] == [126, 40]
