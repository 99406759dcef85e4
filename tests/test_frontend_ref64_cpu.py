"""Pins the float64 front-end reference (tests/frontend_ref64.py) before it judges a kernel: against the reference project's own fp32
front end (tests/golden/frontend.npz) and the fp32 oracle (oracle/sdfa_oracle.py) within a small multiple of its error scale kappa,
its DFT against numpy's FFT, and each of its perturbations changing only what it names.  CPU only."""
import numpy as np
import pytest
import torch

import sdfa_oracle as O
from frontend_ref64 import FrontendRef64, dft_matrices, frame_table
from sdfa_amd import synth

# max |err| / kappa.  The fixture is the reference's own fp32 output on its 7 (or 3) pinned frames per clip: 0.81 - 1.27 measured
# (mel channel; deltas 0.16 - 0.68).  The fp32 oracle on every frame: up to 1.70.
K_FIXTURE = 2.0
K_ORACLE = 3.0
K_SUM = 0.05         # |frame sum - fixture's| / (sum of kappa over the frame): 0.003 - 0.010 measured


@pytest.fixture(scope="module")
def refs():
    return {sr: FrontendRef64(sr) for sr in (8000, 16000)}


def ratio(feat, kappa, other):
    return (np.abs(feat.numpy() - other) / kappa.numpy()).reshape(-1, 3).max(0)


@pytest.mark.parametrize("sr", [8000, 16000])
@pytest.mark.parametrize("kind,clip", [("uniform", 0), ("zeros", 1), ("sweep", 2), ("speechlike", 3)])
def test_reference_fixture(golden, refs, sr, kind, clip):
    g = golden["frontend"]
    pre = f"sr{sr}_{kind}_"
    pcm = synth.make_pcm(clip, 2 * sr, kind)
    fc, fs = frame_table([pcm], sr)
    feat, kappa = refs[sr]([pcm], fc, fs)
    assert feat.dtype == kappa.dtype == torch.float64
    assert list(feat.shape) == list(g[pre + "shape"])
    keep = g[pre + "frames"]
    r = ratio(feat[keep], kappa[keep], g[pre + "audio_feat"])
    assert r.max() <= K_FIXTURE, r
    ds = np.abs(feat.sum((1, 2, 3)).numpy() - g[pre + "frame_sum"])
    assert (ds <= K_SUM * kappa.sum((1, 2, 3)).numpy()).all(), ds.max()


@pytest.mark.parametrize("sr", [8000, 16000])
def test_fp32_oracle_on_every_frame(refs, sr):
    """The clips of tests/test_gpu_parity.py::test_frontend_multi_clip_ragged_vs_oracle, every frame, at both rates, as one
    multi-clip table (each clip's frames cut from its own samples)."""
    clips = [synth.make_pcm(10, 9088), synth.make_pcm(11, 20011, "speechlike"), synth.make_pcm(12, 16000, "sweep")]
    fc, fs = frame_table(clips, sr)
    feat, kappa = refs[sr](clips, fc, fs)
    want = np.concatenate([O.fetch_audio_features(c, sr)["audio_feat"] for c in clips])
    assert feat.shape == want.shape
    r = ratio(feat, kappa, want)
    assert r.max() <= K_ORACLE, r


@pytest.mark.parametrize("win", [512, 1024])
def test_dft_matmul_is_rfft(win):
    x = np.random.RandomState(win).uniform(-1, 1, (6, win))
    c, s = dft_matrices(win)
    xt = torch.from_numpy(x)
    want = np.fft.rfft(x, axis=-1)
    got = (xt @ c).numpy() - 1j * (xt @ s).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    ref = FrontendRef64(win * 125 // 8)
    assert np.abs(ref.spectrum(xt).numpy() - np.abs(want) ** 2).max() <= 1e-12 * (np.abs(want) ** 2).max()


def test_zero_clip_is_exactly_zero(refs):
    for sr, ref in refs.items():
        pcm = np.zeros(sr, np.float32)
        fc, fs = frame_table([pcm], sr)
        feat, kappa = ref([pcm], fc, fs)
        assert not bool(feat.any())
        assert bool(torch.isfinite(kappa).all()) and float(kappa.max()) <= 1e-7 and float(kappa.min()) > 0


def test_chunking_does_not_change_the_reference(refs):
    pcm = synth.make_pcm(8, 8000, "speechlike")
    fc, fs = frame_table([pcm], 8000)
    a, ka = refs[8000]([pcm], fc, fs)
    b, kb = refs[8000]([pcm], fc, fs, chunk=7)
    assert (a - b).abs().max() <= 1e-13 and ((ka - kb).abs() / ka).max() <= 1e-12


# --------------------------------------------------------------------------------------------------------- perturbations
@pytest.fixture(scope="module")
def base(refs):
    """One 8 kHz clip of 1.2 s at 60 fps: its first frames start before the clip."""
    sr = 8000
    pcm = synth.make_pcm(4, int(1.2 * sr), "speechlike")
    fc, fs = frame_table([pcm], sr)
    assert (fs < 0).sum() >= 3
    feat, _ = refs[sr]([pcm], fc, fs)
    return refs[sr], pcm, fc, fs, feat


def changed(base, **kw):
    ref, pcm, fc, fs, feat = base
    bad, _ = ref([pcm], fc, fs, **kw)
    return (bad - feat).abs() > 1e-12                  # (F, 64 T, 128 bands, 3 channels)


def test_preemph_col0_changes_column_0_only(base):
    d = changed(base, preemph_col0=True)
    assert d[:, 0, :, 0].any()
    assert not d[:, 1:, :, 0].any() and not d[:, 5:, :, 1:].any()


def test_stale_col_changes_one_column_of_one_frame(base):
    d = changed(base, stale_col=(30, 20))
    assert d[30, 20, :, 0].any()
    d[30, 20, :, 0] = False
    assert not d[:, :, :, 0].any()
    assert d[30, 16:25, :, 1:].any() and not d[30, :16, :, 1:].any() and not d[30, 25:, :, 1:].any()
    assert not d[:30].any() and not d[31:].any()


def test_mel_shift_changes_one_band(base):
    d = changed(base, mel_shift=50)
    assert d[:, :, 50].any()
    assert not d[:, :, :50].any() and not d[:, :, 51:].any()


def test_delta_edge_zero_changes_only_delta_edges(base):
    d = changed(base, delta_edge_zero=True)
    assert not d[..., 0].any()
    assert d[:, :4, :, 1:].any() and d[:, 60:, :, 1:].any()
    assert not d[:, 4:60].any()


def test_pad_off_by_one_changes_frames_before_the_clip_only(base):
    _, _, _, fs, _ = base
    d = changed(base, pad_off_by_one=True).flatten(1).any(1).numpy()
    assert d[fs < 0].any() and not d[fs >= 0].any()


def test_periodic_hamming_changes_every_frame(base):
    """Every frame that is not zero throughout (the enumeration's last frames start past the clip's end)."""
    *_, feat = base
    d = changed(base, periodic_hamming=True).flatten(1).any(1).numpy()
    live = feat.flatten(1).any(1).numpy()
    assert live.sum() >= 80 and d[live].all()
