"""Capture-rate live streams on the MI355X (include/sdfa_stream.h "Capture-rate streams", sdfa_amd/live.py): the ring resampler
against the offline kernel position by position, and streams at 44.1 / 48 / 22.05 / 8 kHz against the offline chain
generate_animation(clip(resample(x, a, sr) * gain, -0.999, 0.999)) bit for bit, whatever the chunking and the mix of streams."""
import ctypes as C

import numpy as np
import pytest
import torch

from speech_anime.hparams import configure
from speech_anime.api import build_model
from speech_anime.datasets import DatasetSlidingWindow
from sdfa_amd import synth, live
from sdfa_amd._lib import lib, check, SdfaError
from sdfa_amd.engine import frame_geometry
from sdfa_amd.resample import resample

pytestmark = pytest.mark.gpu

LO, HI = np.float32(-0.999), np.float32(0.999)


def _model(sd, sr, head):
    hp = configure(dict(mode="evaluate", custom_hparams=head))
    hp.audio.set_key("sample_rate", sr)
    DatasetSlidingWindow.hparams = None
    return build_model(hp, sd)


def _offline_signal(x, a, sr, gain):
    """The contract's model-rate signal: the library's offline kernel on the whole signal, one float32 multiply, the clamp."""
    y = resample(x, a, sr).cpu().numpy()
    return np.clip(y * np.float32(gain), LO, HI)


def _first_final(a, sr):
    """Fewest input samples after which output 0 is final."""
    n = 0
    while live.resample_final(n, a, sr) == 0:
        n += 1
    return n


def _pieces(n, how, a, sr, rs):
    if how == "whole":
        return [n]
    if how == "one":                   # 1-sample pieces across the first final output, then the rest
        k = _first_final(a, sr) + 40
        return [1] * k + [n - k]
    if how == "441":
        return [441] * (n // 441) + ([n % 441] if n % 441 else [])
    sizes, left = [], n                # random 1 .. 5000
    while left:
        sizes.append(min(left, int(rs.randint(1, 5001))))
        left -= sizes[-1]
    return sizes


class _RingDriver:
    """One stream fed through the C calls alone: input ring 1 of 2 (2^r_in samples), model ring 1 of 2 (2^r samples)."""
    SENTINEL = 7.0

    def __init__(self, a, sr, r_in, r, gain, pad):
        self.a, self.sr, self.r_in, self.r, self.gain, self.pad = a, sr, r_in, r, gain, pad
        self.R_in, self.R = 1 << r_in, 1 << r
        self.in_rings = torch.zeros(2 * (self.R_in + live.RING_MIRROR), dtype=torch.float32, device="cuda")
        self.rings = torch.full((2 * (self.R + live.RING_MIRROR),), self.SENTINEL, dtype=torch.float32, device="cuda")
        self.wing = live.resample_wing(a, sr) + 1
        self.n_fed = self.n_out = 0
        self.treg = 0.0
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.steps = 0

    def room(self):
        oldest = self.n_out if self.a == self.sr else int(self.treg) - self.wing
        return oldest + self.R_in - self.n_fed

    def _resample(self, upto, t_zero):
        """Outputs n_out .. upto - 1 (and the zeros at -pad .. -1 ahead of the first)."""
        lead = self.pad if self.n_out == 0 else 0
        count = upto - self.n_out
        if count + lead == 0:
            return
        n_reg = 0 if self.a == self.sr else max(min(upto, t_zero) - self.n_out, 0)
        reg, self.treg = live.resample_register(self.treg, n_reg, self.a, self.sr)
        bits = int(np.float32(self.gain).view(np.uint32))
        seg = torch.tensor([1, 1, self.n_out - lead, count + lead, self.n_fed, t_zero, 0, 0 | (bits << 32)], dtype=torch.int64, device="cuda")
        d_reg = torch.from_numpy(reg).cuda() if n_reg else torch.zeros(1, dtype=torch.float64, device="cuda")
        rates = (C.c_int32 * 1)(self.a)
        check(lib.sdfa_stream_resample(C.c_void_p(self.in_rings.data_ptr()), self.r_in, 2, C.c_void_p(self.rings.data_ptr()), self.r, 2,
                                       C.c_void_p(seg.data_ptr()), 1, count + lead, C.c_void_p(d_reg.data_ptr()), n_reg, rates, 1, self.sr,
                                       self.stream))
        self.n_out = upto

    def feed(self, piece):
        """Appends `piece` in as many steps as the input ring needs; after each, the outputs that became final are resampled.
        Yields (first new output, one past the last) per step."""
        pos = 0
        while pos < len(piece):
            take = min(self.room(), len(piece) - pos)
            assert take > 0, "the input ring is too small for this schedule"
            src = torch.from_numpy(np.ascontiguousarray(piece[pos:pos + take])).cuda()
            seg = torch.tensor([1, self.n_fed, take, 0], dtype=torch.int64, device="cuda")
            check(lib.sdfa_stream_ring_append(C.c_void_p(self.in_rings.data_ptr()), self.r_in, 2, C.c_void_p(seg.data_ptr()), 1,
                                              C.c_void_p(src.data_ptr()), take, self.stream))
            self.n_fed += take
            pos += take
            t0 = self.n_out
            self._resample(live.resample_final(self.n_fed, self.a, self.sr), live.T_OPEN)
            self.steps += 1
            yield t0, self.n_out

    def close(self):
        n_out, n_res = live.resample_close(self.n_fed, self.a, self.sr)
        t0 = self.n_out
        self._resample(n_out, n_res)
        return t0, n_out, n_res

    def model_ring(self):
        S = self.R + live.RING_MIRROR
        return self.rings[S:2 * S].cpu().numpy()


@pytest.mark.parametrize("a,sr,r_in", [(44100, 16000, 12), (48000, 8000, 12), (8000, 16000, 9), (16000, 16000, 10)])
def test_ring_kernel_equals_offline_kernel(a, sr, r_in):
    gain, r, pad = 0.7, 13, 320
    R = 1 << r
    n_in = int(1.3 * a) + 13
    x = synth.make_pcm(a // 1000, n_in)
    want = _offline_signal(x, a, sr, gain)
    ratio = float(sr) / a
    assert n_in > 10 * (1 << r_in)                                            # the input ring wraps more than ten times
    if a in (44100, 48000):
        assert len(want) > int(n_in * ratio)                                  # n_out > n_res: the zero tail exists
    rs = np.random.RandomState(a)
    for how in ("whole", "one", "441", "random"):
        d = _RingDriver(a, sr, r_in, r, gain, pad if how == "whole" else 0)
        fed = 0
        for size in _pieces(n_in, how, a, sr, rs):
            for t0, t1 in d.feed(x[fed:fed + size]):
                assert t1 == live.resample_final(d.n_fed, a, sr)
                ring = d.model_ring()
                t = np.arange(t0, t1)
                assert np.array_equal(ring[t & (R - 1)], want[t]), (how, t0, t1)
                # exactly t1 positions are written: the next ones still hold what they held (never written, or one lap back)
                nxt = np.arange(t1, t1 + 32)
                old = np.array([d.SENTINEL if (p < R - d.pad or (p < R and d.n_out == 0)) else (0.0 if p < R else want[p - R]) for p in nxt], np.float32)
                assert np.array_equal(ring[nxt & (R - 1)], old), (how, t1)
                assert np.array_equal(ring[R:], ring[:live.RING_MIRROR]), (how, t1)      # the mirror behind the ring
            fed += size
        assert d.n_out <= int(n_in * ratio) and int(n_in * ratio) - d.n_out <= (126 if ratio > 1 else 64)
        t0, n_out, n_res = d.close()
        assert n_out == len(want) and n_res == int(n_in * ratio)
        ring = d.model_ring()
        t = np.arange(max(n_out - R, 0), n_out)              # everything the ring still holds, the zero tail included
        assert np.array_equal(ring[t & (R - 1)], want[t]), how
        assert np.array_equal(ring[R:], ring[:live.RING_MIRROR]), how
        if how == "whole":
            assert d.steps >= 10                               # the input ring forced the steps
        assert np.all(d.rings[:R + live.RING_MIRROR].cpu().numpy() == d.SENTINEL)     # ring 0 is not this stream's
    # the zeros ahead of an ensembling stream: written with the first outputs (here: before the model ring wrapped over them)
    d = _RingDriver(a, sr, r_in, r, gain, pad)
    k = _first_final(a, sr) + 100
    for _ in d.feed(x[:k]):
        pass
    ring = d.model_ring()
    assert d.n_out > 0 and np.all(ring[R - pad:R] == 0.0) and ring[R - pad - 1] == d.SENTINEL
    assert np.array_equal(ring[:d.n_out], want[:d.n_out])


def test_kernel_skips_segments_outside_their_arrays():
    """A segment naming a ring, a rate, a count or registers outside its array writes nothing (and faults nothing)."""
    a, sr = 44100, 16000
    d = _RingDriver(a, sr, 12, 13, 1.0, 0)
    x = synth.make_pcm(1, 3000)
    for _ in d.feed(x):
        pass
    before = d.rings.clone()
    reg, _ = live.resample_register(d.treg, 16, a, sr)
    d_reg = torch.from_numpy(reg).cuda()
    one = int(np.float32(1.0).view(np.uint32)) << 32
    bad = [[2, 1, d.n_out, 16, d.n_fed, live.T_OPEN, 0, one], [1, 2, d.n_out, 16, d.n_fed, live.T_OPEN, 0, one],
           [1, -1, d.n_out, 16, d.n_fed, live.T_OPEN, 0, one], [1, 1, d.n_out, 16, d.n_fed, live.T_OPEN, 1, one],
           [1, 1, d.n_out, 16, d.n_fed, live.T_OPEN, -1, one], [1, 1, d.n_out, 16, d.n_fed, live.T_OPEN, 0, one | 1],
           [1, 1, d.n_out, (1 << 13) + 1, d.n_fed, live.T_OPEN, 0, one], [1, 1, d.n_out, 16, -5, live.T_OPEN, 0, one]]
    seg = torch.tensor(bad, dtype=torch.int64, device="cuda")
    rates = (C.c_int32 * 1)(a)
    check(lib.sdfa_stream_resample(C.c_void_p(d.in_rings.data_ptr()), 12, 2, C.c_void_p(d.rings.data_ptr()), 13, 2, C.c_void_p(seg.data_ptr()),
                                   len(bad), 16, C.c_void_p(d_reg.data_ptr()), 16, rates, 1, sr, d.stream))
    torch.cuda.synchronize()
    assert torch.equal(d.rings, before)
    with pytest.raises(SdfaError, match="input rates"):
        check(lib.sdfa_stream_resample(C.c_void_p(d.in_rings.data_ptr()), 12, 2, C.c_void_p(d.rings.data_ptr()), 13, 2, C.c_void_p(seg.data_ptr()),
                                       1, 16, C.c_void_p(d_reg.data_ptr()), 16, rates, 0, sr, d.stream))


def _chunks(n, how, a, sr, rs):
    """(chunk sizes in input samples, push indices after which to step)."""
    if how == "whole":
        return [n], set()
    if how == "one":        # 1-sample pushes across the first final output with a step after each, then 1 s pieces
        k = _first_final(a, sr) + 30
        sizes = [1] * k + [a] * ((n - k) // a) + ([(n - k) % a] if (n - k) % a else [])
        return sizes, set(range(k - 60, k + 2))
    if how == "441":
        sizes = [441] * (n // 441) + ([n % 441] if n % 441 else [])
        return sizes, set(range(len(sizes)))
    sizes, left = [], n                                            # random 1 .. 5000, a step after every few pushes
    while left:
        sizes.append(min(left, int(rs.randint(1, 5001))))
        left -= sizes[-1]
    return sizes, set(i for i in range(len(sizes)) if rs.rand() < 0.3)


def _stream_through(session, sid, pcm, how, a, sr, rs):
    sizes, steps = _chunks(len(pcm), how, a, sr, rs)
    ts, rows, o = [], [], 0
    for i, c in enumerate(sizes):
        session.push(sid, pcm[o:o + c])
        o += c
        if i in steps:
            for s, (t, r) in session.step().items():
                assert s == sid
                ts.append(t); rows.append(r)
    session.close(sid)
    for s, (t, r) in session.step().items():
        ts.append(t); rows.append(r)
    return np.concatenate(ts), torch.cat(rows)


def _offline(model, y, speaker, ens):
    ts, rows, _ = model.generate_animation(y, speaker, 0, 0, ensembling_ms=ens, want_inputs=False)
    return list(ts), torch.from_numpy(np.ascontiguousarray(rows).reshape(len(ts), -1))


CASES = [(44100, 16000, "dgrad", 0, "fp32", 0.7), (48000, 8000, "offsets", 20, "fp32", 4.0), (8000, 16000, "dgrad", 20, "bf16x3", 1.0)]


@pytest.mark.parametrize("a,sr,head,ens,prec,gain", CASES)
def test_one_stream_equals_offline_chain(synth_sd, a, sr, head, ens, prec, gain):
    model = _model(synth_sd[head], sr, head)
    eng = model._model._engine
    eng.set_precision(prec)
    model.clear_signal_cache()
    x = synth.make_pcm(3 + a // 1000, int(1.3 * a) + 13)
    y = _offline_signal(x, a, sr, gain)
    assert gain < 4 or (np.abs(y) == HI).any()                  # the large gain drives the clamp
    want_ts, want = _offline(model, y, 3, ens)
    rs = np.random.RandomState(a + ens)
    for how in ("whole", "one", "441", "random"):
        # a small budget: both rings wrap, and the whole-clip push forces steps
        s = live.LiveSession(eng, 2, sample_rate=sr, max_ensembling_ms=20, push_budget=sr // 8, max_input_rate=a)
        assert s.R_in < len(x) // 4
        sid = s.open(3, ensembling_ms=ens, input_rate=a, gain=gain)
        ts, rows = _stream_through(s, sid, x, how, a, sr, rs)
        assert ts.dtype == np.int32 and list(ts) == want_ts, how
        assert torch.equal(rows.cpu(), want), (how, float((rows.cpu() - want).abs().max()))
        h = s.health()
        assert h["frontend_repairs"] == 0 and h["open_streams"] == 0
    st = model.animation_stream(3, ensembling_ms=ens, input_rate=a, gain=gain)
    parts = [st.push(x[o:o + 3001]) for o in range(0, len(x), 3001)] + [st.finish()]
    got_ts = [t for p in parts for t in p[0]]
    got = np.concatenate([p[1] for p in parts])
    assert got_ts == want_ts and np.array_equal(got.reshape(len(got_ts), -1), want.numpy())


def test_input_rate_equal_to_the_model_rate(synth_sd):
    """input_rate == sr: the offline call's copy, then gain and clamp -- unlike a stream without input_rate, which is taken as it is."""
    sr = 16000
    model = _model(synth_sd["dgrad"], sr, "dgrad")
    eng = model._model._engine
    x = synth.make_pcm(9, int(1.1 * sr) + 5)
    want_ts, want = _offline(model, _offline_signal(x, sr, sr, 2.5), 1, 0)
    s = live.LiveSession(eng, 1, sample_rate=sr, push_budget=2000, max_input_rate=sr)
    sid = s.open(1, input_rate=sr, gain=2.5)
    ts, rows = _stream_through(s, sid, x, "random", sr, sr, np.random.RandomState(4))
    assert list(ts) == want_ts and torch.equal(rows.cpu(), want)
    plain_ts, plain = _offline(model, x, 1, 0)
    assert plain_ts == want_ts and not torch.equal(plain, want)


def test_mixed_session(synth_sd):
    """Six streams of one session: 44.1, 48 and 22.05 kHz beside three at the model rate, different speakers, one ensembling, pushes
    interleaved, two closing early.  Every stream equals its own offline result, and a step costs the same calls and one copy
    whether one capture-rate stream has new audio or all of them."""
    sr = 16000
    model = _model(synth_sd["dgrad"], sr, "dgrad")
    eng = model._model._engine
    rates = [44100, 48000, 22050, None, None, None]
    secs = [1.3, 0.9, 1.3, 1.3, 0.8, 1.2]
    gains = [0.7, 1.9, 1.0, 1.0, 1.0, 1.0]
    ens = [20, 0, 0, 0, 0, 20]
    spk = [0, 1, 2, 3, 4, 5]
    xs = [synth.make_pcm(60 + i, int(secs[i] * (rates[i] or sr)) + 7 * i) for i in range(6)]
    wants = [_offline(model, x if a is None else _offline_signal(x, a, sr, g), p, e) for x, a, g, p, e in zip(xs, rates, gains, spk, ens)]
    s = live.LiveSession(eng, 6, sample_rate=sr, max_ensembling_ms=20, push_budget=4000)
    sids = [s.open(spk[i], ensembling_ms=ens[i], **({} if rates[i] is None else dict(input_rate=rates[i], gain=gains[i]))) for i in range(6)]
    pos = [0] * 6
    got = {sid: ([], []) for sid in sids}
    open_ = set(range(6))

    def tick(who, seconds):
        for i in who:
            if i in open_:
                c = int(seconds * (rates[i] or sr))
                s.push(sids[i], xs[i][pos[i]:pos[i] + c])
                pos[i] = min(len(xs[i]), pos[i] + c)
        for i in list(open_):
            if pos[i] >= len(xs[i]):
                s.close(sids[i])
                open_.discard(i)
        for sid, (t, r) in s.step().items():
            got[sid][0].append(t); got[sid][1].append(r.cpu())
        return dict(s.last_calls)

    everyone = range(6)
    tick(everyone, 0.65)                                        # past the first window: frames flow from here on
    one = tick([0, 3, 4, 5], 0.05)                              # one capture-rate stream (the ensembling one) and the model-rate ones
    full = tick(everyone, 0.05)                                 # all of them
    assert one == full and one["h2d_copy"] == 1 and one["resample"] == 1 and one["ring_append"] == 2 and one["frontend_ring"] == 1
    rs = np.random.RandomState(8)
    while open_:                                                # streams 4 and 1 end first; the others go on
        tick([i for i in everyone if rs.rand() < 0.8], float(rs.choice([0.013, 0.05, 0.21])))
    for i, sid in enumerate(sids):
        ts = np.concatenate(got[sid][0])
        assert list(ts) == wants[i][0], i
        assert torch.equal(torch.cat(got[sid][1]), wants[i][1]), i
    h = s.health()
    assert h["frontend_repairs"] == 0 and h["open_streams"] == 0


def test_ends_raise_the_offline_errors(synth_sd):
    sr, a = 16000, 44100
    model = _model(synth_sd["dgrad"], sr, "dgrad")
    eng = model._model._engine
    _, _, sliding = frame_geometry(sr)
    x = synth.make_pcm(70, int(1.0 * a))
    want_ts, want = _offline(model, _offline_signal(x, a, sr, 1.0), 2, 0)
    s = live.LiveSession(eng, 3, sample_rate=sr)
    keep = s.open(2, input_rate=a)
    s.push(keep, x[:30000])
    got = [s.step()]
    tiny = s.open(0, input_rate=a)
    s.push(tiny, x[:2])
    with pytest.raises(SdfaError, match="input signal length=2 is too small to resample from 44100->16000"):
        s.close(tiny)
    with pytest.raises(SdfaError, match="too small to resample"):
        resample(x[:2], a, sr)                                  # the offline text
    short = s.open(1, input_rate=a)
    n_short = int(0.5 * sliding * a / sr)
    s.push(short, x[:n_short])
    s.push(keep, x[30000:])
    got.append(s.step())                                        # the short stream's samples are resampled like any other's
    with pytest.raises(AssertionError) as live_err:
        s.close(short)
    with pytest.raises(AssertionError) as offline_err:
        model.generate_animation(_offline_signal(x[:n_short], a, sr, 1.0), 1, 0, 0, ensembling_ms=0, want_inputs=False)
    assert str(live_err.value) == str(offline_err.value)
    s.close(keep)
    got.append(s.step())
    assert all(set(g) <= {keep} for g in got)
    ts = np.concatenate([g[keep][0] for g in got if keep in g])
    rows = torch.cat([g[keep][1] for g in got if keep in g])
    assert list(ts) == want_ts and torch.equal(rows.cpu(), want)
    assert s.health()["open_streams"] == 0
