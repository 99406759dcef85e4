"""CPU checks of the validation losses' contract (include/sdfa_score.h): the float64 restatement tests/score_ref64.py is what
the reference's PLoss / MLoss return (against tests/golden/score_criterion.npz, made by the reference's own criterion); the
host arithmetic of sdfa_amd.score -- truth_plan, dataset_frame_starts, clip_scalars, anime_weights -- restates the
reference's loops; the info list is parsed from a data root; the ABI of the header is bound and exported and every
host-side refusal is made before a launch."""
import ctypes as C
import math
import os
import pickle
import re

import numpy as np
import pytest

import score_ref64 as R
from gen_golden_score import CASES, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The largest relative gap, over every scalar of every case of the fixture, between the reference's float32 result and the
# float64 model: measured 1.418e-06 (dgrad_weighted.scalar_mr -- differences of exponentials of nearby values, formed and
# summed in float32 there).  The test allows 4 x that, the margin covering the reference's float32 summation.
MEASURED_GAP = 1.418e-06


def _n(layout, W):
    return W // 9 if layout == "dgrad" else W


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_the_references_criterion(golden, name):
    """Measured: largest |model / reference - 1| over the fixture = 1.418e-06; asserted: 4 x that."""
    from sdfa_amd import score
    g = golden["score_criterion"]
    layout, pred, truth, weights = inputs(name)
    assert np.array_equal(pred, g[name + ".pred"]) and np.array_equal(truth, g[name + ".truth"]) and np.array_equal(weights, g[name + ".weights"])
    want = {k: float(g[f"{name}.{k}"]) for k in score.SCALAR_KEYS if f"{name}.{k}" in g.files}
    assert set(want) == (set(score.SCALAR_KEYS) if layout == "dgrad" else {"scalar_ploss", "scalar_mloss"})
    model = R.criterion64(pred, truth, weights, layout)
    rec, _ = R.records(pred, truth, [0, len(pred)], layout)
    ours = score.clip_scalars(rec, [0, len(pred)], _n(layout, pred.shape[1]), weights)["clips"][0]
    for k, ref in want.items():
        print(name, k, ref, model[k] / ref - 1, ours[k] / model[k] - 1)
        assert abs(model[k] / ref - 1) <= 4 * MEASURED_GAP, (k, model[k], ref)
        assert abs(ours[k] / model[k] - 1) <= 1e-13, (k, ours[k], model[k])      # records + clip_scalars = the criterion on [a; b]
    if layout == "plain":
        assert ours["scalar_pr"] == ours["scalar_mr"] == 0.0


def _get_anime_indices(l, r, sr, start_ts, minfi, maxfi, fps, ts_delta):
    """datasets/sliding_window.py:205-227 and speech_anime.py:135-138, line by line (NumPy >= 2 scalar promotion: a float32
    scalar stays float32 against Python numbers)."""
    ms = float((l + r) / 2 * 1000.0) / float(sr)
    ts = np.float32(ms)
    ts = ts - ts_delta + start_ts
    pos = ts * fps / 1000.0
    pos_lower = int(math.floor(pos))
    pos_upper = pos_lower + 1
    if pos_lower < minfi:
        pos_lower = minfi
        pos_upper = minfi
    elif pos_upper > maxfi:
        pos_lower = maxfi
        pos_upper = maxfi
    a = float(pos - pos_lower)
    return pos_lower, pos_upper, np.float32(1.0 - a), np.float32(a)


@pytest.mark.parametrize("sr,start_ts,minfi,maxfi", [(16000, 0.0, -10 ** 6, 10 ** 6), (16000, 1234.5, 80, 300), (8000, -50.25, 3, 150), (22050, 16.6666, 0, 200)])
def test_truth_plan_is_get_anime(sr, start_ts, minfi, maxfi):
    from sdfa_amd import score
    assert int(np.__version__.split(".")[0]) >= 2, "the transcription above relies on NumPy 2 scalar promotion"
    starts = score.dataset_frame_starts(5 * sr, sr)
    # frames on exact track frames (a = 0): pos = k  <=>  mid sample = (k * 1000 / fps + ts_delta - start_ts) * sr / 1000
    sliding = score.sliding_samples(sr)
    exact = np.asarray([int(round((k * 1000 / 60 + 100) * sr / 1000 - sliding / 2)) for k in range(0, 120, 6)], np.int64)
    starts = np.concatenate((starts, exact, np.arange(-3000, 3000, 7)))
    assert len(starts) > 1000
    src, w = score.truth_plan(starts, sr, start_ts, minfi, maxfi)
    assert src.dtype == np.int64 and w.dtype == np.float32 and src.shape == w.shape == (len(starts), 2)
    for i, s in enumerate(starts.tolist()):
        lo, up, w0, w1 = _get_anime_indices(s, s + sliding, sr, start_ts, minfi, maxfi, 60, 100)
        assert (lo, up) == tuple(src[i]) and w0 == w[i, 0] and w1 == w[i, 1], (i, s, lo, up, w0, w1, src[i], w[i])
    clamped = minfi > -10 ** 6
    assert (src[:, 0] == src[:, 1]).any() == clamped                                 # both clamps are met where they exist
    if clamped:
        assert (src[:, 0] == minfi).any() and (src[:, 1] == maxfi).any()
    if start_ts == 0.0:
        assert (w[:, 1] == 0).any() and (w[w[:, 1] == 0, 0] == 1).all()                # a = 0 happens


@pytest.mark.parametrize("L,sr,fps", [(16000, 16000, 60), (12345, 8000, 60), (50001, 22050, 25), (9088, 16000, 60), (1, 16000, 60)])
def test_dataset_frame_starts_is_the_references_loop(L, sr, fps):
    from sdfa_amd import score
    win_size, hop_size, feat_frames = 0.064, 0.008, 64                               # sliding_window.py:24-61
    sliding_size = int(sr * (hop_size * (feat_frames - 1) + win_size))
    coordinates = []
    extra_samples = sr // 3
    delta_samples = float(sr) / float(fps)
    stt_sp = 0 - extra_samples
    end_sp = L + extra_samples
    left = stt_sp
    while left + sliding_size <= end_sp:
        s = math.ceil(left)
        coordinates.append((s, s + sliding_size))
        left += delta_samples
    got = score.dataset_frame_starts(L, sr, fps)
    assert got.dtype == np.int64 and got.tolist() == [s for s, _ in coordinates]
    assert score.sliding_samples(sr) == sliding_size


def test_clip_scalars_on_hand_made_records():
    from sdfa_amd import score
    rec = np.zeros((5, 4))
    rec[:, 0] = [1, 2, 3, 40, 50]
    rec[:, 1] = [0.5, 0.5, 0.5, 1, 1]
    rec[:, 2] = [0, 6, 8, 0, 10]
    rec[:, 3] = [0, 1, 2, 0, 3]
    res = score.clip_scalars(rec, [0, 3, 5], 2)
    c0, c1 = res["clips"]
    # clip 0, frames 0 1 2: a = [0 1 1], b = [1 2 2]
    assert c0["scalar_ps"] == pytest.approx((1 + 2 + 2 + 2 + 3 + 3) / 2 / 6) and c0["scalar_ms"] == pytest.approx(2 * (6 + 8 + 8) / 2 / 3)
    assert c0["scalar_pr"] == pytest.approx(0.25) and c0["scalar_mr"] == pytest.approx(2 * (1 + 2 + 2) / 2 / 3)
    # clip 1, frames 3 4: a = [3 3], b = [4 4]
    assert c1["scalar_ps"] == pytest.approx((40 + 40 + 50 + 50) / 2 / 4) and c1["scalar_ms"] == pytest.approx(2 * (10 + 10) / 2 / 2)
    assert c0["scalar_ploss"] == c0["scalar_ps"] + c0["scalar_pr"] and c1["scalar_mloss"] == c1["scalar_ms"] + c1["scalar_mr"]
    for k in score.SCALAR_KEYS:
        assert res["corpus"][k] == pytest.approx((3 * c0[k] + 2 * c1[k]) / 5)
    wt = np.asarray([1, 2, 3, 1, 0.5])
    cw = score.clip_scalars(rec, [0, 3, 5], 2, wt)["clips"][0]
    assert cw["scalar_ps"] == pytest.approx((1 * 1 + 2 * 2 + 2 * 2 + 2 * 2 + 3 * 3 + 3 * 3) / 2 / 6)
    assert cw["scalar_ms"] == pytest.approx(((1 + 2) * 6 + (2 + 3) * 8 + (2 + 3) * 8) / 2 / 3)
    with pytest.raises(AssertionError):
        score.clip_scalars(rec, [0, 4, 5], 2)


def test_anime_weights_blend_like_the_rows():
    from sdfa_amd import score
    d = np.asarray([0.001, 0.004, 0.02], np.float32)
    src = np.asarray([[0, 1], [1, 2], [2, 2]], np.int64)
    w = np.asarray([[0.25, 0.75], [1, 0], [0.5, 0.5]], np.float32)
    got = score.anime_weights(d, src, w)
    for i in range(3):
        lower, upper, a = d[src[i, 0]], d[src[i, 1]], float(w[i, 1])
        dist = lower * np.float32(1.0 - a) + upper * np.float32(a)
        assert got[i] == np.float32(np.exp((0.002 - dist) * 50) * 2)


def test_valid_csv_is_parsed_from_a_data_root(tmp_path):
    from speech_anime import validate as V
    rs = np.random.RandomState(0)
    root = tmp_path / "root"
    rows = []
    for i, (n, minfi, maxfi) in enumerate(((4000, 2, 9), (6000, 0, 5))):
        d = root / "data" / f"clip{i}"
        d.mkdir(parents=True)
        for fi in range(minfi, maxfi + 1):
            np.save(d / f"{fi:06d}.npy", np.full((5, 9), fi + 10 * i, np.float32))
            np.save(d / f"{fi:06d}_lips_dist.npy", np.float32(0.001 * fi))
        audio = rs.uniform(-0.5, 0.5, n).astype(np.float32)
        with open(str(d) + "_audio", "wb") as fp:
            pickle.dump({"sr": 8000, "audio": audio}, fp)
        rows.append((f"data/clip{i}" if i == 0 else str(d), f"m{i}", 12.5 * i, minfi, maxfi, n))
    with open(root / "valid.csv", "w") as fp:
        fp.write("npy_data_path:path,speaker:str,emotion:str,start_ts:float,anime_minfi:int,anime_maxfi:int,audio_samples:int\n")
        for r in rows:
            fp.write(f"{r[0]},{r[1]},neutral,{r[2]},{r[3]},{r[4]},{r[5]}\n")
    clips = V.read_valid_csv(str(root / "valid.csv"), with_lips_dist=True)
    assert len(clips) == 2
    for i, c in enumerate(clips):
        n, minfi, maxfi = ((4000, 2, 9), (6000, 0, 5))[i]
        assert c["speaker"] == f"m{i}" and c["start_ts"] == 12.5 * i and (c["minfi"], c["maxfi"]) == (minfi, maxfi)
        assert c["signal"].dtype == np.float32 and c["signal"].shape == (n,) and c["sr"] == 8000
        assert c["track"].shape == (maxfi - minfi + 1, 45) and c["track"].dtype == np.float32
        assert np.array_equal(c["track"][:, 0], np.arange(minfi, maxfi + 1) + 10 * i)
        assert np.allclose(c["lips_dist"], 0.001 * np.arange(minfi, maxfi + 1))
    with open(root / "bad.csv", "w") as fp:
        fp.write("speaker:str\nm0\n")
    with pytest.raises(ValueError):
        V.read_valid_csv(str(root / "bad.csv"))


def test_score_abi_is_bound_and_exported():
    from sdfa_amd import _lib, score, pca
    hdr = open(os.path.join(ROOT, "include", "sdfa_score.h")).read()
    declared = set(re.findall(r"\b(sdfa_score_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(score.SYMBOLS), declared ^ set(score.SYMBOLS)
    assert _lib.lib.sdfa_score_abi_version() == score.ABI_VERSION == int(re.search(r"#define SDFA_SCORE_ABI_VERSION\s+(\d+)", hdr).group(1))
    for other in (_lib, pca):
        assert not declared & set(other.SYMBOLS), "score symbols belong to their own header"
    for name, const in (("COLS", score.COLS), ("RUN", score.RUN), ("PARTS", score.PARTS), ("LAYOUT_DGRAD", score.LAYOUT_DGRAD), ("LAYOUT_PLAIN", score.LAYOUT_PLAIN)):
        assert int(re.search(rf"#define SDFA_SCORE_{name}\s+(\d+)", hdr).group(1)) == const
    assert score.COLS % 36 == 0


def refusals():
    """(name, arguments of sdfa_score_rows after the pointers are filled in) that only the host checks can answer: F, W, layout,
    n_track, offsets, workspace bytes given (None = exactly enough), which pointer to null."""
    ok = dict(F=6, W=45, layout=0, n_track=4, off=[0, 3, 6], ws=None, null=None)
    cases = {"short clip": dict(off=[0, 5, 6]), "empty clip": dict(off=[0, 0, 6]), "offsets not from 0": dict(off=[1, 3, 6]),
             "offsets not to F": dict(off=[0, 3, 5]), "dgrad width": dict(W=44), "unknown layout": dict(layout=2), "no track": dict(n_track=0),
             "short workspace": dict(ws=-1), "one frame": dict(F=1, off=[0, 1]), "no clips": dict(off=[0])}
    for p in ("pred", "track", "src", "w", "off", "out", "ws"):
        cases["null " + p] = dict(null=p)
    return [(k, {**ok, **v}) for k, v in cases.items()]


def call_refused(lib, a, ptr, out_ptr=None):
    """Calls sdfa_score_rows with `ptr` (a dummy address when there is no device: a refusal never touches it) for every pointer."""
    off = (C.c_int64 * len(a["off"]))(*a["off"])
    need = lib.sdfa_score_workspace_bytes(max(a["F"], 2), 45 if a["W"] % 9 else a["W"], 0)
    ws = need + (a["ws"] or 0)
    p = {k: ptr for k in ("pred", "track", "src", "w", "out", "ws")}
    p["off"] = C.cast(off, C.c_void_p).value
    if out_ptr is not None:
        p["out"] = out_ptr
    if a["null"]:
        p[a["null"]] = None
    return lib.sdfa_score_rows(p["pred"], a["F"], a["W"], a["layout"], p["track"], a["n_track"], p["src"], p["w"], p["off"], len(a["off"]) - 1,
                               p["out"], p["ws"], ws, None)


@pytest.mark.parametrize("name,a", refusals(), ids=[k for k, _ in refusals()])
def test_refusals_are_made_on_the_host(name, a):
    from sdfa_amd import _lib, score  # noqa: F401
    rc = call_refused(_lib.lib, a, 256)                      # 256: aligned and never to be dereferenced
    assert rc == _lib.EINVAL, name
    assert _lib.lib.sdfa_last_error().decode().startswith("score_rows:")


def test_workspace_bytes():
    from sdfa_amd import _lib, score
    lib = _lib.lib
    small = lib.sdfa_score_workspace_bytes(10, 45, 0)
    assert small > 0 and small % 256 == 0
    assert lib.sdfa_score_workspace_bytes(10, score.COLS, 0) == small < lib.sdfa_score_workspace_bytes(10, score.COLS + 9, 0)
    assert lib.sdfa_score_workspace_bytes(10, 44, 0) == _lib.EINVAL and lib.sdfa_score_workspace_bytes(10, 44, 1) > 0
    assert lib.sdfa_score_workspace_bytes(1, 45, 0) == _lib.EINVAL and lib.sdfa_score_workspace_bytes(10, 45, 3) == _lib.EINVAL
    assert lib.sdfa_score_workspace_bytes(20352, 89784, 0) >= 20352 * 10 * 4 * 32


def test_model_bound_covers_float32_terms():
    """The bound is what float32 terms can move: a float32 evaluation of the same sums stays inside it."""
    for layout, W in (("dgrad", 90), ("plain", 31)):
        t = R.tracks(12, W, 3, 0.4)
        p = (t + R.tracks(12, W, 4, 0.1)).astype(np.float32)
        rec0, b0 = R.records(t, t, [0, 5, 12], layout)
        assert not rec0.any() and not b0[:, 0].any()          # (the exp and motion bounds do not know that equal inputs round equally)
        rec, bound = R.records(p, t, [0, 5, 12], layout)
        assert (rec[[0, 5], 2:] == 0).all() and (rec[1:5, 2] > 0).all() and (bound[:, 0] > 0).all() and (bound[:, 0] < 1e-5 * rec[:, 0]).all()
        rot = R.rotat_mask(W, layout)
        ep, et = np.where(rot, np.exp(p), p).astype(np.float32), np.where(rot, np.exp(t), t).astype(np.float32)
        d = (ep - et).astype(np.float64)
        assert (np.abs((d * d)[:, ~rot].sum(1) - rec[:, 0]) <= bound[:, 0]).all()
        m = ((ep[1:] - ep[:-1]) - (et[1:] - et[:-1])).astype(np.float64)
        got = (m * m)[:, ~rot].sum(1)
        keep = np.asarray([f for f in range(1, 12) if f != 5])
        assert (np.abs(got[keep - 1] - rec[keep, 2]) <= bound[keep, 2]).all()
        if layout == "dgrad":
            assert (np.abs((d * d)[:, rot].sum(1) - rec[:, 1]) <= bound[:, 1]).all()
