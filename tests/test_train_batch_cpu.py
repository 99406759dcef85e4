"""The host side of the training batches (speech_anime/datasets/sliding_window.py draw_augment / convert_window, sdfa_amd/augment.py
pack_desc and the library's sdfa_augment_check) against what the reference's own DatasetSlidingWindow.__getitem__ did under the
same seeds (tests/golden/train_window.npz part B, tests/gen_golden_train_window.py).  CPU only: nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

import gen_golden_train_window as G
from sdfa_amd import _lib, augment, score
from score_ref64 import blend32
from speech_anime import hparams as H
from speech_anime.datasets.sliding_window import SOURCES, DatasetSlidingWindow as DSW


@pytest.fixture(scope="module")
def hp():
    h = H.configure({"custom_hparams": "dgrad"})
    h.audio.set_key("sample_rate", G.B_SR)
    return h


def coordinates():
    return np.concatenate([np.stack([np.full(len(s), ci), s], 1) for ci, s in
                           enumerate(score.dataset_frame_starts(c[0], G.B_SR) for c in G.B_CLIPS)])


def test_coordinates_are_the_reference_datasets(golden):
    assert np.array_equal(coordinates(), golden["train_window"]["b_coords"])
    assert tuple(SOURCES) == tuple(G.SOURCES)


@pytest.mark.parametrize("index", G.INDICES)
def test_draw_augment_reproduces_getitem(golden, hp, index):
    g = golden["train_window"]
    co = g["b_coords"]
    sliding = score.sliding_samples(G.B_SR)
    d = DSW.draw_augment(np.random.RandomState(G.SEED0 + index), sliding, hp)
    i, j = index, index + 1
    if j == len(co) or co[i, 0] != co[j, 0]:
        i, j = index - 1, index
    assert [i, j] == g[f"b{index}.ids"][:2].tolist()
    ints, floats = g[f"b{index}.int"], g[f"b{index}.float"]
    for half, fr in ((0, i), (1, j)):
        l = int(co[fr, 1]) + d["shift"]
        stt, end = DSW.convert_window(l, l + sliding, d["sr"], G.B_SR)
        got = [SOURCES.index(d["source"]), d["sr"], stt, end, d["ex_feat"], d["ex_time"], d["trunck"], d["pad_reflect"], d["lower_freq"], d["drop_zero"]]
        assert got == ints[half].tolist(), (half, got, ints[half])
        want = np.array([d["preemph"], d["noise_scale"], d["dropout"], d["mask_thres"]], np.float64)
        assert want.tobytes() == floats[half].tobytes(), (half, want, floats[half])          # bit for bit
    assert d["scale"].dtype == np.float64 and d["scale"].tobytes() == g[f"b{index}.feat_scale"].tobytes()
    assert np.array_equal(d["mask_idx"], g[f"b{index}.mask_idx"])
    assert g[f"b{index}.ids"][3] == d["sr"]
    if d["noise_scale"] > 0:
        assert d["noise"][0].dtype == np.float32 and len(d["noise"][0]) == len(d["noise"][1]) == d["cut"]
    else:
        assert d["noise"] is None


def test_device_noise_mode_draws_no_noise_from_the_generator(hp):
    a = DSW.draw_augment(np.random.RandomState(G.SEED0), 9088, hp, noise="device")
    b = DSW.draw_augment(np.random.RandomState(G.SEED0), 9088, hp, noise="numpy")
    assert a["noise"] is None and b["noise"] is not None and a["noise_scale"] == b["noise_scale"] > 0
    assert a["preemph"] == b["preemph"] and a["scale"].tobytes() == b["scale"].tobytes()


@pytest.mark.parametrize("index", G.INDICES)
def test_targets_and_weights_are_get_animes(golden, hp, index):
    """truth_plan + the three-rounding blend of sdfa_seek_rows (restated by score_ref64.blend32) + anime_weights on the recorded
    windows give the reference's targets and weights bit for bit."""
    g = golden["train_window"]
    co, ints = g["b_coords"], g[f"b{index}.int"]
    ci = int(co[g[f"b{index}.ids"][0], 0])
    L, _, _, spk, start_ts, minfi, maxfi = G.B_CLIPS[ci]
    sliding = score.sliding_samples(G.B_SR)
    d = DSW.draw_augment(np.random.RandomState(G.SEED0 + index), sliding, hp)
    ls = np.array([co[g[f"b{index}.ids"][k], 1] + d["shift"] for k in (0, 1)], np.int64)
    src, w = score.truth_plan(ls, G.B_SR, start_ts, minfi, maxfi)
    rows = blend32(g[f"b_track{ci}"], src - minfi, w)
    for k in (0, 1):
        assert np.array_equal(rows[k], g[f"b{index}.target{k}"]), np.abs(rows[k] - g[f"b{index}.target{k}"]).max()
    wt = score.anime_weights(g[f"b_lips{ci}"], src - minfi, w)
    assert wt.dtype == np.float32 and np.array_equal(wt, g[f"b{index}.weight"]), (wt, g[f"b{index}.weight"])
    assert g[f"b{index}.ids"][2] == H.DEFAULTS["dataset_anime"]["speakers"][spk]
    assert ints[0][1] == ints[1][1]


def test_convert_window():
    f = DSW.convert_window
    assert f(-5333, 3755, 16000, 16000) == (-5333, 3755)
    assert f(-5333, 3755, 8000, 16000) == (-2666, -2666 + 4544)            # int() truncates towards zero
    assert f(-5332, 3756, 8000, 16000) == (-2666, 1878)
    assert f(0, 9088, 8000, 16000) == (0, 4544)                            # a start of 0 is falsy: the other branch
    assert f(1, 9089, 8000, 16000) == (0, 4544)
    assert f(101, 9189, 8000, 16000) == (50, 4594)
    assert f(100, 4644, 16000, 8000) == (200, 9288)


def test_pack_desc_round_trip():
    rs = np.random.RandomState(5)
    n = 40
    want = dict(clip=rs.randint(0, 7, n).astype(np.int32), start=rs.randint(-2 ** 40, 2 ** 40, n), ex_time=rs.randint(-4, 5, n).astype(np.int32),
                preemph=rs.uniform(0, 0.95, n).astype(np.float32), ex_feat=rs.randint(-5, 6, n).astype(np.int32), lower_freq=rs.rand(n) < 0.5,
                trunck=rs.rand(n) < 0.5, pad_reflect=rs.rand(n) < 0.5, drop=[sorted(set(rs.randint(0, 128, rs.randint(0, 20)).tolist())) for _ in range(n)])
    want["drop"][0], want["drop"][1] = [], list(range(128))
    d = augment.pack_desc(**want)
    assert d.dtype == augment.DESC and d.itemsize == 48 and d.shape == (n,)
    got = augment.unpack_desc(d)
    for k, v in want.items():
        assert (got[k] == v) if k == "drop" else np.array_equal(got[k], v), k
    assert np.array_equal(augment.drop_words([3, 3, 70, 127]), augment.drop_words([127, 70, 3]))          # duplicates, as np.random.choice draws them
    assert augment.drop_words([0, 31, 32, 127]).tolist() == [0x80000001, 1, 0, 0x80000000]
    augment.check_desc(d, np.full(7, 1000))
    one = augment.pack_desc(2, 17)                                          # scalars
    assert one.shape == (1,) and one["clip"][0] == 2 and one["start"][0] == 17 and one["preemph"][0] == np.float32(0.65)
    assert C.sizeof(C.c_char * 48) == d.itemsize and d["drop"].shape == (n, 4)


def refused(fn, *a):
    with pytest.raises(_lib.SdfaError) as e:
        fn(*a)
    return str(e.value)


def test_check_refuses_each_bad_field():
    good = augment.pack_desc([0, 1], [5, -9000], [4, -4], [0.0, 0.95], [5, -5], True, True, True, [[0], [127]])
    augment.check_desc(good)
    augment.check_desc(good, [10, 2 ** 29 - 1])
    augment.check_desc(good[:0])
    for field, value, word in (("ex_time", 5, "ex_time"), ("ex_time", -5, "ex_time"), ("ex_feat", 6, "ex_feat"), ("ex_feat", -6, "ex_feat"),
                               ("flags", 8, "flag"), ("reserved", 1, "reserved"), ("preemph", np.nan, "preemph"), ("preemph", np.inf, "preemph"),
                               ("clip", -1, "clip")):
        bad = good.copy()
        bad[field][1] = value
        assert word in refused(augment.check_desc, bad), (field, value)
    assert "clip" in refused(augment.check_desc, good, [10])                # clip 1 of a one-clip batch
    assert "2^29" in refused(augment.check_desc, good, [10, 2 ** 29])       # a clip the 32-bit sample arithmetic does not cover
    assert "samples" in refused(augment.check_desc, good, [10, -1])


def test_frontend_refusals_come_before_any_launch():
    """Arguments the host refuses without touching the device (this test runs without one)."""
    lib = _lib.lib
    p = C.c_void_p(256)            # never dereferenced: every call below is refused first
    call = lambda sr, n, noise, stride: _lib.check(lib.sdfa_augment_frontend(p, p, p, 1, p, n, sr, noise, stride, None, p, None))
    assert "sample_rate" in refused(call, 44100, 1, None, 0)
    assert "sample_rate" in refused(call, 0, 1, None, 0)
    assert "windows" in refused(call, 8000, -1, None, 0)
    assert "windows" in refused(call, 8000, 2 ** 31, None, 0)
    assert augment.noise_samples(8000) == 71 * 64 + 512 and augment.noise_samples(16000) == 71 * 128 + 1024
    assert "noise_stride" in refused(call, 8000, 1, p, 71 * 64 + 511)
    assert "noise_stride" in refused(call, 16000, 1, p, 71 * 128 + 1023)
    assert "sample_rate" in refused(augment.noise_samples, 22050)
    assert int(lib.sdfa_augment_abi_version()) == augment.ABI_VERSION == 1
    assert _lib.check(lib.sdfa_augment_frontend(p, p, p, 1, p, 0, 8000, None, 0, None, p, None)) == 0      # no window: nothing to do
