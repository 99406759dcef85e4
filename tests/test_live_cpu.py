"""CPU checks of live streaming (include/sdfa_stream.h, sdfa_amd/live.py): frame positions and final-frame counts against the
offline enumeration and the oracle, the delayed ensembling view against np.pad, the header against the binding, and the
argument checks that must fire before any device work."""
import os
import re

import numpy as np
import pytest

import sdfa_oracle as O
from sdfa_amd import _lib, engine, live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sr", [8000, 16000])
def test_frame_positions_equal_frame_index(sr):
    rs = np.random.RandomState(5)
    _, _, sliding = engine.frame_geometry(sr)
    lengths = [sliding, sliding + 1, 10 * sr, 10 * sr + 1, 60 * sr + 7, 600 * sr + 13] + list(rs.randint(sliding, 40 * sr, 40))
    for L in lengths:
        s_c, t_c = engine.frame_index(int(L), sr)
        s_o, t_o = O.frame_index(int(L), sr)
        s_l, t_l = live.frame_positions(0, len(s_c), sr)
        assert np.array_equal(s_l, s_c) and np.array_equal(t_l, t_c), L
        assert np.array_equal(s_l, s_o) and np.array_equal(t_l, t_o), L
        k0 = int(rs.randint(0, len(s_c)))                      # any k0: a function of k alone
        s_k, t_k = live.frame_positions(k0, len(s_c) - k0, sr)
        assert np.array_equal(s_k, s_c[k0:]) and np.array_equal(t_k, t_c[k0:]), (L, k0)


@pytest.mark.parametrize("sr", [8000, 16000])
def test_final_frame_count(sr):
    win, hop, sliding = engine.frame_geometry(sr)
    s_all, _ = engine.frame_index(30 * sr, sr)
    e_all = s_all + sliding
    ns = sorted(set([0, 1, sliding - 1, sliding, sliding + 1, 2 * sliding] + list(range(sliding - 700, sliding + 3000, 7))
                    + list(np.random.RandomState(1).randint(1, 25 * sr, 300))))
    for n in ns:
        want = 0 if n - 1 < sliding else int((e_all < n).sum())
        assert live.final_frames(n, sr) == want, n
    # at close: sdfa_frame_index(n) frames; short streams raise the offline short-clip error
    for n in (sliding, sliding + 1, 3 * sr + 5, 10 * sr):
        assert live.close_frames(n, sr) == len(engine.frame_index(n, sr)[0]) == len(O.frame_index(n, sr)[0])
        assert live.close_frames(n, sr) >= live.final_frames(n, sr)
    # below one window the offline call's assert fires for most lengths (not all: the windows sit at discrete positions);
    # close raises exactly where it does
    raised = 0
    for n in [1, sliding // 2] + list(range(sliding - 400, sliding)):
        try:
            want = len(engine.frame_index(n, sr)[0])
        except AssertionError as e:
            raised += 1
            with pytest.raises(AssertionError, match=re.escape(str(e))):
                live.close_frames(n, sr)
        else:
            assert live.close_frames(n, sr) == want and live.final_frames(n, sr) == 0
    assert raised >= 2


def test_length_limit_message():
    from sdfa_amd._lib import SdfaError
    with pytest.raises(SdfaError, match="2\\^29"):
        live.final_frames(0x1fffffff + 1, 16000)
    assert live.final_frames(0x1fffffff, 16000) > 0


def _ring_view(signal, pad, R, start, n_win):
    """Window [start, start + n_win) of the delayed view cut from a numpy model of the ring: signal written at p & (R - 1),
    read at (g - pad) & (R - 1), zero outside [0, max(len - pad, 0)) in the ring's coordinates."""
    ring = np.zeros(R, np.float32)
    L = len(signal)
    lo = max(0, L - R)
    for p in range(lo, L):
        ring[p & (R - 1)] = signal[p]
    g = np.arange(start, start + n_win) - pad
    hi = max(L - pad, 0)
    ok = (g >= 0) & (g < hi)
    assert (g[ok] >= lo).all(), "window no longer in the ring"
    return np.where(ok, ring[g & (R - 1)], 0.0).astype(np.float32)


@pytest.mark.parametrize("sr", [8000, 16000])
def test_delayed_view_equals_np_pad(sr):
    rs = np.random.RandomState(3)
    _, _, sliding = engine.frame_geometry(sr)
    R = 1 << int(np.ceil(np.log2(3 * sliding)))
    for L, ms in ((sliding + 5, 20), (3 * sliding, 20), (2 * sliding + 17, 7), (50, 20), (160, 20), (161, 10)):
        pad = ms * sr // 1000
        sig = rs.uniform(-1, 1, L).astype(np.float32)
        ref = np.pad(sig[:-pad], [[pad, 0]], "constant")     # model.py:373-384
        for start in list(range(-sliding, L + 1, max(1, L // 9))) + [L - sliding - 1, -pad]:
            want = np.array([ref[g] if 0 <= g < len(ref) else 0.0 for g in range(start, start + sliding)], np.float32)
            if min(start - pad, L) < L - R + sliding:             # the ring model only holds the newest R samples
                continue
            got = _ring_view(sig, pad, R, start, sliding)
            assert np.array_equal(got, want), (L, pad, start)


def test_stream_header_symbols_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sdfa_stream.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(live.SYMBOLS), declared ^ set(live.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.sdfa_stream_abi_version() == live.ABI_VERSION == 1
    assert not declared & set(_lib.SYMBOLS), "stream symbols belong to their own header, not the core ABI"
    assert _lib.lib.sdfa_abi_version() == 5


class _HostEngine:
    """What LiveSession reads of an Engine before its first step."""
    device = "cuda:0"
    max_frames = 4096
    out_dim, coef_dim = 89784, 265
    check_speaker_ids = staticmethod(engine.Engine.check_speaker_ids)


def test_bad_arguments_raise_before_device_work():
    sr = 16000
    _, _, sliding = engine.frame_geometry(sr)
    s = live.LiveSession(_HostEngine(), 4, sample_rate=sr)
    with pytest.raises(RuntimeError, match="out of bounds"):
        s.open(8)
    with pytest.raises(RuntimeError, match="out of bounds"):
        s.open(-1)
    sid = s.open(2)
    with pytest.raises(ValueError, match="\\[-1, 1\\]"):
        s.push(sid, np.array([0.0, 1.5], np.float32))
    with pytest.raises(ValueError, match="\\[-1, 1\\]"):
        s.push(sid, np.array([np.nan], np.float32))
    s.push(sid, np.zeros(sliding + 100, np.float32))     # fits the ring: no step, no device
    s.close(sid)
    with pytest.raises(ValueError, match="closed"):
        s.push(sid, np.zeros(10, np.float32))
    short = s.open(1)
    s.push(short, np.zeros(sliding // 2, np.float32))
    with pytest.raises(AssertionError, match="signal length"):
        s.close(short)
    with pytest.raises(KeyError):
        s.push(short, np.zeros(10, np.float32))               # a short stream is dropped at close
    c = live.LiveSession(_HostEngine(), 2, sample_rate=sr, outputs="coef")
    with pytest.raises(ValueError, match="coefficients"):
        c.open(0, ensembling_ms=20)
    assert s.stream is None and s.rings is None and c.stream is None     # nothing above touched the device


def test_large_delay_with_small_budget_needs_no_early_step():
    """Positions below -pad are never read, so the room before the first final frame is R - pad - n: at 16 kHz with a 200 ms delay
    and a 1,000-sample budget (R = 2^14) a 13,000-sample push fits without a step.  (Counting from the first window's start, the
    room ran out at 8,372 samples, before any frame was final, and the forced step could free nothing.)"""
    s = live.LiveSession(_HostEngine(), 1, sample_rate=16000, push_budget=1000, max_ensembling_ms=200)
    assert s.R == 1 << 14
    sid = s.open(0, ensembling_ms=200)
    s.push(sid, np.zeros(13000, np.float32))
    assert s.stream is None and s._streams[sid].n_total == 13000


def test_ring_front_end_refuses_the_radix4_switch():
    """With "mel_fft_radix4" on, offline 16 kHz features take another column transform: the live front end refuses the call
    (before any device work) instead of returning frames that differ from offline."""
    import ctypes as C
    fake = C.c_void_p(1 << 20)                      # never dereferenced: the switch is checked before anything is read
    _lib.set_option("mel_fft_radix4", 1)
    try:
        with pytest.raises(_lib.SdfaError, match="mel_fft_radix4"):
            _lib.check(_lib.lib.sdfa_mel_frontend_ring(fake, 14, 1, fake, fake, 1, fake, fake, 1, 16000, fake, fake, 1 << 30, None))
    finally:
        _lib.set_option("mel_fft_radix4", 0)
