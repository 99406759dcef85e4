"""Live streaming on the MI355X (sdfa_amd/live.py, include/sdfa_stream.h): every streamed frame is bit-identical to the same frame
of the offline call on the whole signal, whatever the chunking, the mix of streams, the ring wraps and a concurrent offline call."""
import threading

import numpy as np
import pytest
import torch

from speech_anime.hparams import configure
from speech_anime.api import build_model
from speech_anime.datasets import DatasetSlidingWindow
from sdfa_amd import synth, live
from sdfa_amd.engine import FrontendOnly, frame_geometry

pytestmark = pytest.mark.gpu


def _model(sd, sr, head):
    hp = configure(dict(mode="evaluate", custom_hparams=head))
    hp.audio.set_key("sample_rate", sr)
    DatasetSlidingWindow.hparams = None
    return build_model(hp, sd)


def _chunks(n, how, sr, rs):
    """(chunk sizes, push indices after which to step)."""
    _, _, sliding = frame_geometry(sr)
    if how == "whole":
        return [n], set()
    if how == "one":        # 1-sample pushes across the first window, a step around its end, then 1 s pieces
        k = sliding + 40
        sizes = [1] * k + [sr] * ((n - k) // sr) + ([(n - k) % sr] if (n - k) % sr else [])
        return sizes, set(range(sliding - 4, sliding + 4)) | {sliding // 2, k - 1, k + 1}
    if how == "17":
        sizes = [17] * (n // 17) + ([n % 17] if n % 17 else [])
        return sizes, set(range(0, len(sizes), 53))
    if how == "1s":
        sizes = [sr] * (n // sr) + ([n % sr] if n % sr else [])
        return sizes, set(range(len(sizes)))
    sizes, left = [], n                                            # random 1 .. 5000, a step after every few pushes
    while left:
        sizes.append(min(left, int(rs.randint(1, 5001))))
        left -= sizes[-1]
    return sizes, set(i for i in range(len(sizes)) if rs.rand() < 0.3)


def _stream_through(session, sid, pcm, how, sr, rs):
    sizes, steps = _chunks(len(pcm), how, sr, rs)
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


CASES = [(16000, "dgrad", 0, "fp32"), (8000, "dgrad", 20, "fp32"), (16000, "offsets", 20, "fp32"), (8000, "offsets", 0, "fp32"),
         (16000, "dgrad", 20, "bf16x3"), (8000, "offsets", 20, "bf16x3")]


@pytest.mark.parametrize("sr,head,ens,prec", CASES)
def test_one_stream_equals_generate_animation(synth_sd, sr, head, ens, prec):
    model = _model(synth_sd[head], sr, head)
    eng = model._model._engine
    eng.set_precision(prec)
    model.clear_signal_cache()
    pcm = synth.make_pcm(7 + sr // 1000, int(2.3 * sr) + 11)
    want_ts, want, _ = model.generate_animation(pcm, 3, 0, 0, ensembling_ms=ens, want_inputs=False)
    want = torch.from_numpy(np.ascontiguousarray(want).reshape(len(want_ts), -1))
    rs = np.random.RandomState(sr + ens)
    for how in ("whole", "one", "17", "1s", "random"):
        s = live.LiveSession(eng, 2, sample_rate=sr, max_ensembling_ms=20)
        sid = s.open(3, ensembling_ms=ens)
        ts, rows = _stream_through(s, sid, pcm, how, sr, rs)
        assert ts.dtype == np.int32 and list(ts) == list(want_ts), how
        assert torch.equal(rows.cpu(), want), (how, float((rows.cpu() - want).abs().max()))
        h = s.health()
        assert h["frontend_repairs"] == 0 and h["open_streams"] == 0
    # the public wrapper: push / finish concatenate to generate_animation[:2]
    st = model.animation_stream(3, ensembling_ms=ens)
    parts = [st.push(pcm[a:a + 3001]) for a in range(0, len(pcm), 3001)] + [st.finish()]
    got_ts = [t for p in parts for t in p[0]]
    got = np.concatenate([p[1] for p in parts])
    assert got_ts == list(want_ts) and np.array_equal(got.reshape(len(got_ts), -1), want.numpy())


def test_coefficients_expand_to_the_rows(synth_sd):
    sr = 16000
    model = _model(synth_sd["dgrad"], sr, "dgrad")
    eng = model._model._engine
    pcm = synth.make_pcm(3, int(1.7 * sr))
    want_ts, want, _ = model.generate_animation(pcm, 5, 0, 0, ensembling_ms=0, want_inputs=False)
    s = live.LiveSession(eng, 1, sample_rate=sr, outputs="coef")
    sid = s.open(5)
    ts, coef = _stream_through(s, sid, pcm, "random", sr, np.random.RandomState(0))
    assert coef.shape == (len(want_ts), eng.coef_dim) and list(ts) == list(want_ts)
    rows = eng.expand_coef(coef.contiguous())
    assert torch.equal(rows.cpu(), torch.from_numpy(np.ascontiguousarray(want).reshape(len(want_ts), -1)))


def test_many_interleaved_streams(synth_sd):
    """64 streams with mixed speakers, lengths, ensembling and push patterns, some closing while others go on; one 16 s stream
    wraps its 2^14-sample ring about fifteen times (compared on every 5th frame)."""
    sr = 16000
    model = _model(synth_sd["dgrad"], sr, "dgrad")
    eng = model._model._engine
    rs = np.random.RandomState(11)
    S = 64
    lens = [int(rs.uniform(0.6, 2.5) * sr) for _ in range(S - 1)] + [16 * sr + 5]
    pcms = [synth.make_pcm(100 + i, n) for i, n in enumerate(lens)]
    spk = [int(rs.randint(0, 8)) for _ in range(S)]
    ens = [20 if i % 3 == 0 else 0 for i in range(S)]
    s = live.LiveSession(eng, S, sample_rate=sr, push_budget=4000, max_ensembling_ms=20)
    assert s.R == 1 << 14 or s.R == 1 << 15
    sids = [s.open(spk[i], ensembling_ms=ens[i]) for i in range(S)]
    pos = [0] * S
    got = {i: ([], []) for i in range(S)}
    sid_to_i = {sid: i for i, sid in enumerate(sids)}
    open_ = set(range(S))
    tick = 0
    while open_:
        for i in list(open_):
            if pos[i] < lens[i]:
                c = int(rs.choice([1, 17, 267, 533, 3999, 11000]))
                s.push(sids[i], pcms[i][pos[i]:pos[i] + c])
                pos[i] = min(lens[i], pos[i] + c)
            elif rs.rand() < 0.5:
                s.close(sids[i])
                open_.discard(i)
        tick += 1
        if tick % 2 == 0 or not open_:
            for sid, (t, r) in s.step().items():
                i = sid_to_i[sid]
                got[i][0].append(t)
                got[i][1].append(r[::5].cpu() if i == S - 1 else r.cpu())
    for e in (0, 20):
        idx = [i for i in range(S) if ens[i] == e]
        outs = model.generate_animation_batch([pcms[i] for i in idx], [spk[i] for i in idx], ensembling_ms=e)
        for i, (wts, wrows, _) in zip(idx, outs):
            ts = np.concatenate(got[i][0])
            assert list(ts) == list(wts), i
            w = torch.from_numpy(np.ascontiguousarray(wrows).reshape(len(wts), -1))
            if i == S - 1:
                # the rows of each step were subsampled from its own start: rebuild the frame indices
                k, keep = 0, []
                for t in got[i][0]:
                    keep += list(range(k, k + len(t), 5))
                    k += len(t)
                w = w[keep]
            assert torch.equal(torch.cat(got[i][1]), w), i
    assert s.health()["frontend_repairs"] == 0


def test_frontend_ring_equals_gather():
    """sdfa_mel_frontend_ring against sdfa_mel_frontend_gather of the same frames: windows across the ring's wrap point, a
    valid_hi that cuts a column in the middle, a delayed view."""
    import ctypes as C
    from sdfa_amd._lib import lib, check
    fe = FrontendOnly("cuda:0")
    for sr in (8000, 16000):
        win, hop, sliding = frame_geometry(sr)
        r = int(np.ceil(np.log2(sliding + 1)))
        R = 1 << r
        L = 3 * R + 1234
        sig = synth.make_pcm(sr, L)
        hi = L - 37                                      # not a multiple of the hop: a column is cut inside
        pad = 20 * sr // 1000
        lo = L - R + 1                                   # the ring holds [L - R, L); a frame may start at lo (reads lo - 1)
        starts = list(range(lo, hi - 40, hop * 7)) + list(range(hi - sliding - 3 * hop, hi + 9, hop)) + [3 * R - 500, 3 * R - sliding // 2]
        starts = np.array(sorted(set(s for s in starts if s >= lo)), np.int64)
        S = R + live.RING_MIRROR
        rings = torch.zeros(2 * S, dtype=torch.float32, device="cuda")
        buf = np.zeros(S, np.float32)
        for p in range(L - R, L):
            buf[p & (R - 1)] = sig[p]
        buf[R:] = buf[:live.RING_MIRROR]                                 # the mirror behind the ring
        rings[S:] = torch.from_numpy(buf).cuda()                         # the stream lives in ring 1
        dstarts = starts[starts - pad >= lo]                             # delayed view: starts s, samples s - pad
        fs = np.concatenate([starts, dstarts - pad])
        fv = np.concatenate([np.zeros(len(starts), np.int32), np.ones(len(dstarts), np.int32)])
        vring = torch.tensor([1, 1 | (pad << 32)], dtype=torch.int64, device="cuda")
        vhi = torch.tensor([hi, hi - pad], dtype=torch.int64, device="cuda")
        d_fs = torch.from_numpy(fs).cuda()
        d_fv = torch.from_numpy(fv).cuda()
        n = len(fs)
        out = torch.empty((n, 64, 128, 3), dtype=torch.float32, device="cuda")
        ws = torch.empty(int(check(lib.sdfa_frontend_workspace_bytes(n))), dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.sdfa_mel_frontend_ring(C.c_void_p(rings.data_ptr()), r, 2, C.c_void_p(vring.data_ptr()), C.c_void_p(vhi.data_ptr()), 2,
                                         C.c_void_p(d_fv.data_ptr()), C.c_void_p(d_fs.data_ptr()), n, sr, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(ws.data_ptr()), ws.numel(), st))
        # offline: clip 0 = sig[:hi], clip 1 = np.pad(sig[:hi][:-pad], [[pad, 0]]) with the main starts
        c0 = sig[:hi]
        c1 = np.pad(c0[:-pad], [[pad, 0]], "constant")
        pcm = torch.from_numpy(np.concatenate([c0, c1])).cuda()
        off = torch.tensor([0, hi], dtype=torch.int64, device="cuda")
        ln = torch.tensor([hi, hi], dtype=torch.int64, device="cuda")
        ofs = torch.from_numpy(np.concatenate([starts, dstarts])).cuda()
        ref = fe.mel_frontend_device(pcm, off, ln, d_fv, ofs, sr)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), (sr, int((out != ref).any(dim=(1, 2, 3)).sum()))
        assert int(check(lib.sdfa_debug_frontend_status(C.c_void_p(ws.data_ptr()), st))) == 0
        wrap = (starts // R) != ((starts + sliding - 1) // R)
        assert wrap.any() and (starts + sliding > hi).any()


def test_session_beside_offline_call(synth_sd):
    """A session stepping on its own stream in one thread while generate_animation runs on another stream: both stay bitwise."""
    sr = 16000
    model = _model(synth_sd["dgrad"], sr, "dgrad")
    other = _model(synth_sd["dgrad"], sr, "dgrad")
    eng = model._model._engine
    pcm = synth.make_pcm(21, 3 * sr)
    big = synth.make_pcm(22, 10 * sr)
    want_ts, want, _ = model.generate_animation(pcm, 1, 0, 0, ensembling_ms=0, want_inputs=False)
    want = torch.from_numpy(np.ascontiguousarray(want).reshape(len(want_ts), -1))
    big_ts, big_want, _ = other.generate_animation(big, 2, 0, 0, ensembling_ms=0, want_inputs=False)
    big_want = big_want.copy()
    other.clear_signal_cache()
    torch.cuda.synchronize()
    res, errs = {}, []

    def live_thread():
        try:
            s = live.LiveSession(eng, 4, sample_rate=sr)
            sid = s.open(1)
            res["live"] = _stream_through(s, sid, pcm, "1s", sr, np.random.RandomState(0))
            torch.cuda.synchronize()
        except Exception as ex:                                             # noqa: BLE001 -- reported below
            errs.append(ex)

    t = threading.Thread(target=live_thread)
    t.start()
    stream = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(stream):
        for _ in range(3):
            other.clear_signal_cache()
            outs.append(other.generate_animation(big, 2, 0, 0, ensembling_ms=0, want_inputs=False)[1].copy())
    stream.synchronize()
    t.join()
    assert not errs, errs
    ts, rows = res["live"]
    assert list(ts) == list(want_ts) and torch.equal(rows.cpu(), want)
    for o in outs:
        assert np.array_equal(o, big_want)
