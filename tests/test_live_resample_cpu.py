"""CPU checks of capture-rate live streams (include/sdfa_stream.h "Capture-rate streams", sdfa_amd/live.py): the final-output count
against a restatement of the rule and against the resampler oracle's prefix behaviour, the carried time register, the gain
arithmetic against rms_normalize, and the argument checks that must fire before any device work."""
import numpy as np
import pytest

import resample_oracle as RO
from sdfa_amd import engine, live, synth
from sdfa_amd._lib import SdfaError
from speech_anime import audio

PAIRS = [(44100, 16000), (48000, 8000), (22050, 16000), (11025, 8000), (8000, 16000)]
NWIN, NUM_TABLE = 64 * 512 + 1, 512


def _registers(n, a, sr):
    """Time registers of outputs 0 .. n: the sequential float64 sum (np.cumsum of a 1-D float64 array adds in order)."""
    inc = 1.0 / (float(sr) / a)
    return np.concatenate([[0.0], np.cumsum(np.full(n, inc))])


def _needed(treg, a, sr):
    """n(t) + 1 + room_R(t): input samples that must have arrived before output t's right wing is complete (resample_kernel's
    wing 1, the oracle's `(nwin - offset) // step`)."""
    ratio = float(sr) / a
    scale = min(1.0, ratio)
    step = int(scale * NUM_TABLE)
    n = treg.astype(np.int64)
    frac = scale - scale * (treg - n)
    offset = (frac * NUM_TABLE).astype(np.int64)
    return n + 1 + (NWIN - offset) // step


def _final_table(n_in_max, a, sr):
    """Non-decreasing M with final(n_in) = #{t : M[t] <= n_in}: output t is final when every t' <= t has needed(t') <= n_in."""
    treg = _registers(int(n_in_max * float(sr) / a) + 8, a, sr)
    return np.maximum.accumulate(_needed(treg, a, sr))


def test_cumsum_is_the_sequential_register():
    inc = 1.0 / (16000.0 / 44100)
    tr, seq = 0.0, []
    for _ in range(5000):
        seq.append(tr)
        tr += inc
    assert np.array_equal(_registers(4999, 44100, 16000), np.array(seq))


@pytest.mark.parametrize("a,sr", PAIRS)
def test_final_output_count(a, sr):
    M = _final_table(10 ** 6, a, sr)
    first = int(M[0])                                           # input samples at which output 0 becomes final
    rs = np.random.RandomState(a + sr)
    ns = sorted(set([0, 1, 10 ** 6] + list(range(max(first - 40, 0), first + 60)) + list(rs.randint(0, 10 ** 6, 3000))))
    want = np.searchsorted(M, ns, side="right")
    got = [live.resample_final(n, a, sr) for n in ns]
    assert got == list(want)
    assert got[0] == 0 and live.resample_final(first - 1, a, sr) == 0 and live.resample_final(first, a, sr) >= 1
    assert all(x <= y for x, y in zip(got, got[1:]))            # non-decreasing in n_in
    ratio = float(sr) / a
    held = [int(n * ratio) - g for n, g in zip(ns, got) if n >= first]
    assert min(held) >= 0 and max(held) <= (126 if ratio > 1 else 64), (min(held), max(held))
    # in any order too: the count is a function of n_in alone
    for n in rs.permutation(ns)[:200]:
        assert live.resample_final(int(n), a, sr) == int(np.searchsorted(M, n, side="right"))


def test_final_count_of_equal_rates_and_refusals():
    assert [live.resample_final(n, 16000, 16000) for n in (0, 1, 12345)] == [0, 1, 12345]
    with pytest.raises(SdfaError, match="too small for the filter table"):
        live.resample_final(100, 16000 * 600, 16000)
    with pytest.raises(SdfaError, match="bad argument"):
        live.resample_final(-1, 44100, 16000)
    with pytest.raises(SdfaError, match="bad argument"):
        live.resample_final(5, 0, 16000)


@pytest.mark.parametrize("a,sr", PAIRS)
def test_prefix_property_against_the_oracle(a, sr):
    """What the rule promises: the first final(n') outputs of the prefix x[:n'] are those of the whole signal, bit for bit."""
    x = synth.make_pcm(a // 100 + sr // 1000, int(0.12 * a))
    whole = RO.resampy_resample(x, a, sr)
    ratio = float(sr) / a
    rs = np.random.RandomState(a)
    first = int(_final_table(len(x), a, sr)[0])
    prefixes = [first, first + 1, len(x) - 1] + list(rs.randint(first, len(x), 5))
    nonzero = 0
    for n1 in prefixes:
        T = live.resample_final(n1, a, sr)
        assert 1 <= T <= int(n1 * ratio)
        part = RO.resampy_resample(x[:n1], a, sr)
        assert np.array_equal(part[:T], whole[:T]), (n1, T)
        nonzero += int(np.count_nonzero(whole[:T]))
        if T < len(part) and n1 < len(x) - 500:
            assert not np.array_equal(part, whole[:len(part)])   # and the outputs held back do still change
    assert nonzero > 0


@pytest.mark.parametrize("a,sr", [(44100, 16000), (8000, 16000), (48000, 8000)])
def test_time_register_is_carried(a, sr):
    n = 10 ** 6 + 5000
    want = _registers(n, a, sr)
    reg, state = live.resample_register(0.0, 1, a, sr)                      # t0 = 0
    assert reg[0] == 0.0 and state == want[1]
    reg, state = live.resample_register(state, 999, a, sr)                  # t0 = 1
    assert np.array_equal(reg, want[1:1000]) and state == want[1000]
    rs = np.random.RandomState(sr)
    t = 1000
    while t < 10 ** 6:                                                      # ... carried to t0 = 10^6 in pieces of any size
        c = min(int(rs.randint(0, 70000)), 10 ** 6 - t)
        reg, state = live.resample_register(state, c, a, sr)
        assert np.array_equal(reg, want[t:t + c])
        t += c
    reg, state = live.resample_register(state, 5000, a, sr)
    assert np.array_equal(reg, want[10 ** 6:10 ** 6 + 5000]) and state == want[10 ** 6 + 5000]
    if a == 44100:                                                          # (the increments 0.5 and 6 are exact either way)
        assert not np.array_equal(reg, np.arange(10 ** 6, 10 ** 6 + 5000) * (1.0 / (float(sr) / a)))     # t * inc rounds differently


def test_rms_gain_and_clamp_equal_rms_normalize():
    rs = np.random.RandomState(2)
    lo, hi = np.float32(-0.999), np.float32(0.999)
    clipped = 0
    for i, db in enumerate((-24.5, -20, -6, -1)):
        for wav in (rs.uniform(-1, 1, 20000).astype(np.float32) * np.float32(0.3), synth.make_pcm(40 + i, 30011, "speechlike")):
            g = audio.rms_gain(wav, db)
            assert isinstance(g, np.float32)
            want = audio.rms_normalize(wav, db)
            got = np.clip(wav * g, lo, hi)
            assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want), db
            clipped += int((np.abs(want) == hi).sum())
    assert clipped > 0                                           # the clamp took part
    wav = synth.make_pcm(1, 5000)
    assert np.array_equal(np.clip(wav * audio.rms_gain(wav, -20, threshold=-30.0), lo, hi), audio.rms_normalize(wav, -20, threshold=-30.0))
    assert audio.rms_gain(wav, -20, threshold=10.0) == np.float32(1.0)     # empty selection: rms_normalize returns its input


def test_close_lengths_and_offline_refusals():
    for a, sr, n in ((44100, 16000, 57343), (48000, 8000, 62413), (8000, 16000, 10413), (16000, 16000, 777)):
        ratio = float(sr) / a
        n_out, n_res = live.resample_close(n, a, sr)
        assert n_out == int(np.ceil(n * ratio)) == len(RO.librosa_resample(np.zeros(n, np.float32), a, sr))
        assert n_res == int(n * ratio) and live.resample_final(n, a, sr) <= n_res
    with pytest.raises(SdfaError, match="input signal length=2 is too small to resample from 44100->16000"):
        live.resample_close(2, 44100, 16000)
    with pytest.raises(ValueError, match="Input signal length=2 is too small to resample from 44100->16000"):
        RO.resampy_resample(np.zeros(2, np.float32), 44100, 16000)


class _HostEngine:
    """What LiveSession reads of an Engine before its first step."""
    device = "cuda:0"
    max_frames = 4096
    out_dim, coef_dim = 89784, 265
    check_speaker_ids = staticmethod(engine.Engine.check_speaker_ids)


def test_bad_arguments_raise_before_device_work():
    sr = 16000
    s = live.LiveSession(_HostEngine(), 4, sample_rate=sr)
    for rate in (0, -44100, 44100.5):
        with pytest.raises(ValueError, match="input_rate"):
            s.open(0, input_rate=rate)
    with pytest.raises(ValueError, match="max_input_rate"):
        s.open(0, input_rate=96000)
    with pytest.raises(SdfaError, match="too small for the filter table"):      # a rate pair the offline call refuses, its message
        live.LiveSession(_HostEngine(), 1, sample_rate=sr, push_budget=16, max_input_rate=sr * 600)
    for gain in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="gain"):
            s.open(0, input_rate=44100, gain=gain)
    with pytest.raises(ValueError, match="gain needs input_rate"):
        s.open(0, gain=0.5)
    assert not s._streams and len(s._free) == 4                  # a refused open takes no ring
    sid = s.open(2, ensembling_ms=20, input_rate=44100, gain=0.7)
    with pytest.raises(ValueError, match="\\[-1, 1\\]"):
        s.push(sid, np.array([0.0, 1.5], np.float32))
    with pytest.raises(ValueError, match="\\[-1, 1\\]"):
        s.push(sid, np.array([np.nan], np.float32))
    s.push(sid, np.zeros(30000, np.float32))                     # fits both rings: no step, no device
    st = s._streams[sid]
    assert st.in_total == 30000 and st.n_total == live.resample_final(30000, 44100, sr) and st.n_dev == 0
    tiny = s.open(1, input_rate=44100)
    s.push(tiny, np.zeros(2, np.float32))
    with pytest.raises(SdfaError, match="too small to resample"):
        s.close(tiny)
    with pytest.raises(KeyError):
        s.push(tiny, np.zeros(1, np.float32))                    # dropped at close
    short = s.open(1, input_rate=48000)
    s.push(short, np.zeros(9000, np.float32))
    with pytest.raises(AssertionError, match="signal length"):
        s.close(short)
    assert len(s._free) == 3
    assert s.stream is None and s.rings is None and s.in_rings is None


def test_input_ring_size():
    """R_in >= left wing + right wing + push budget in input samples + 1; a wing reaches nwin / step (+ the sample at n) inputs."""
    assert live.resample_wing(44100, 16000) == 177 and live.resample_wing(48000, 8000) == 385 and live.resample_wing(16000, 16000) == 0
    s = live.LiveSession(_HostEngine(), 1, sample_rate=16000, max_input_rate=44100)
    assert s.R_in == 1 << 16 and 2 * 178 + 44100 + 1 <= s.R_in < 2 * (2 * 178 + 44100 + 1)
    s = live.LiveSession(_HostEngine(), 1, sample_rate=16000, push_budget=1000, max_input_rate=44100)
    assert s.R_in == 1 << 12 and 2 * 178 + 2757 + 1 <= s.R_in         # ceil(1000 * 44100 / 16000) = 2757
    s = live.LiveSession(_HostEngine(), 1, sample_rate=8000, push_budget=400, max_input_rate=48000)
    assert s.R_in == 1 << 12 and 2 * 386 + 2400 + 1 <= s.R_in
    assert live.LiveSession(_HostEngine(), 1, sample_rate=8000).max_input_rate == 48000
