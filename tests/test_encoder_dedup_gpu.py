"""The table-less encoder call (sdfa_encoder_forward, Engine.encoder(feat)) finds the identical columns of audio_feat itself
(csrc/share.hip: hash -> match -> full compare -> owner walk) and evaluates each distinct column once.  Reference side of every
comparison here: the same call with "encoder_dedup_off" = 1, the every-column arithmetic -- never the scan itself.  All comparisons
are bitwise (torch.equal) on z and align."""
import numpy as np
import pytest
import torch

from sdfa_amd import synth, _lib
from sdfa_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _every_column(e, feat, **kw):
    try:
        _lib.set_option("encoder_dedup_off", 1)
        return e.encoder(feat, **kw)
    finally:
        _lib.set_option("encoder_dedup_off", 0)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _last_chunk(n, max_frames):
    return n - (n - 1) // max_frames * max_frames


@pytest.fixture(scope="module")
def eng(synth_sd):
    return Engine(synth_sd["dgrad"])


@pytest.mark.parametrize("sr,seconds,max_frames", [
    (16000, [2.0], 8192),                        # 156 frames               (the sizes of tests/test_share_gx0_gpu.py: one per
    (16000, [10.0, 3.1], 8192),                  # 844 frames, two clips     time-LSTM kernel form)
    (16000, [10.0, 10.0, 4.0], 8192),            # 1,528 frames
    (16000, [10.0] * 5 + [1.3], 8192),           # 3,290 frames
    (16000, [10.0] * 14, 16384),                 # 8,904 frames in one chunk
    (16000, [10.0] * 4, 1024),                   # several workspace chunks per call: links never cross a chunk
    (8000, [10.0, 3.1], 8192),                   # the other sample rate (hop 64)
    (16000, [2.37, 0.613, 5.003, 1.0], 8192),    # ragged batch: clip lengths that are multiples of nothing
])
def test_frontend_features_default_equals_every_column_equals_table(synth_sd, sr, seconds, max_frames):
    """default == switch off == table path, and the scan finds at least what the table finds: distinct_columns(default) <=
    distinct_columns(table) for the same (last) chunk.  The table path's count is the reference (tests/test_gpu_parity.py recounts it on
    the host); a column without a link is a distinct column, and the table's own (prev, shift) is one of the scan's candidates."""
    e = Engine(synth_sd["dgrad"], max_frames=max_frames)
    clips = [synth.make_pcm(70 + i, int(s * sr), "speechlike" if i % 2 else "uniform") for i, s in enumerate(seconds)]
    feat, _, _ = e.mel_frontend(clips, sr)
    fc, fs, hop = e.last_frame_table
    n = feat.shape[0]
    last = _last_chunk(n, max_frames)
    r_scan = e.encoder(feat)
    d_scan = e.distinct_columns(last)
    r_off = _every_column(e, feat)
    r_table = e.encoder(feat, frame_clip=fc, frame_start=fs, hop=hop)
    d_table = e.distinct_columns(last)
    print(f"sr {sr} frames {n} last chunk {last}: distinct columns scan {d_scan} table {d_table} of {64 * last}")
    assert _same(r_scan, r_off) and _same(r_table, r_off)
    assert d_scan <= d_table < 64 * last
    assert e.time_lstm_repairs() == 0


def test_random_features_share_nothing(eng):
    """torch.rand features have no two equal columns: every column is its own owner (no false link), same bits."""
    n = 300
    feat = torch.rand((n, 64, 128, 3), generator=torch.Generator().manual_seed(11)).cuda()
    r = eng.encoder(feat)
    d = eng.distinct_columns(n)
    assert _same(r, _every_column(eng, feat))
    assert d == 64 * n


def _shared_pair(fc, fs, hop, n, t):
    """(p, t + d): the column the frame table says column (n, t) is a copy of (share_prev_kernel's rule, interior columns 6..58)."""
    fc, fs = fc.cpu().numpy(), fs.cpu().numpy()
    for p in range(n - 1, max(n - 65, -1), -1):
        diff = int(fs[n] - fs[p])
        if fc[p] != fc[n] or diff <= 0 or diff > 52 * hop:
            break
        if diff % hop == 0:
            d = diff // hop
            assert 6 <= t and t + d <= 58
            return p, t + d
    raise AssertionError("frame has no hop-aligned predecessor")


def test_near_copies_are_not_shared(eng):
    """A column that differs from its copy in the lowest mantissa bit of its LAST float, or in the sign of a zero, is a distinct column:
    the result is the every-column result for the edited input, and the count of distinct columns goes up by exactly the one column
    that lost its link (a proposal accepted without the full bit-pattern compare fails here)."""
    sr = 16000
    feat, _, _ = eng.mel_frontend([synth.make_pcm(41, 10 * sr, "speechlike")], sr)
    fc, fs, hop = eng.last_frame_table
    n = feat.shape[0]
    cols = feat.view(n, 64, 384)
    f, t = 20, 10
    p, tp = _shared_pair(fc, fs, hop, f, t)
    assert torch.equal(cols[f, t], cols[p, tp])                  # the front end's copies are exact
    eng.encoder(feat, frame_clip=fc, frame_start=fs, hop=hop)
    d_table = eng.distinct_columns(n)
    eng.encoder(feat)
    d0 = eng.distinct_columns(n)
    assert d0 <= d_table

    a = feat.clone()
    bits = a.view(n, 64, 384).view(torch.int32)
    bits[f, t, 383] ^= 1                                         # one ulp in the last of the 384 floats
    assert _same(eng.encoder(a), _every_column(eng, a))
    assert eng.distinct_columns(n) == d0 + 1

    b = feat.clone()
    bc = b.view(n, 64, 384)
    bc[f, t, 100] = 0.0
    bc[p, tp, 100] = 0.0                                         # still copies of each other
    assert _same(eng.encoder(b), _every_column(eng, b))
    assert eng.distinct_columns(n) == d0
    bc[f, t, 100] = -0.0                                         # equal as floats, not as bits
    assert bool((bc[f, t] == bc[p, tp]).all()) and not torch.equal(bc[f, t].view(torch.int32), bc[p, tp].view(torch.int32))
    assert _same(eng.encoder(b), _every_column(eng, b))
    assert eng.distinct_columns(n) == d0 + 1


def test_chunks_of_equal_columns_terminate(eng):
    """Every column equal to every other (all-zero features), and one frame repeated 256 times: the owner walk is bounded whatever the
    data (each step goes to an earlier frame and a later time step), the call returns, same bits, no time-LSTM repair."""
    zeros = torch.zeros((700, 64, 128, 3), device="cuda")
    assert _same(eng.encoder(zeros), _every_column(eng, zeros))
    print("all-zero features, 700 frames: distinct columns", eng.distinct_columns(700), "of", 64 * 700)
    one = torch.rand((1, 64, 128, 3), generator=torch.Generator().manual_seed(5)).cuda()
    rep = one.expand(256, 64, 128, 3).contiguous()
    assert _same(eng.encoder(rep), _every_column(eng, rep))
    sr = 16000
    feat, _, _ = eng.mel_frontend([synth.make_pcm(42, 2 * sr)], sr)
    rep = feat[17:18].expand(256, 64, 128, 3).contiguous()
    assert _same(eng.encoder(rep), _every_column(eng, rep))
    assert eng.time_lstm_repairs() == 0


def test_shuffled_frames_and_repeated_clip(eng):
    """The scan assumes nothing about the order of the frames or about who made them: frames in shuffled order, and two copies of one
    clip in one batch (copies further than 64 frames apart are simply not found)."""
    sr = 16000
    clip = synth.make_pcm(43, int(3.3 * sr), "speechlike")
    feat, _, _ = eng.mel_frontend([clip, synth.make_pcm(44, 2 * sr)], sr)
    perm = torch.randperm(feat.shape[0], generator=torch.Generator().manual_seed(7)).cuda()
    shuffled = feat[perm].contiguous()
    assert _same(eng.encoder(shuffled), _every_column(eng, shuffled))
    twice, _, _ = eng.mel_frontend([clip, clip], sr)
    twice = twice.clone()
    r = eng.encoder(twice)
    assert _same(r, _every_column(eng, twice))
    h = twice.shape[0] // 2
    assert torch.equal(r[0][:h], r[0][h:])


def test_split_bf16_default_equals_every_column(synth_sd):
    """bf16x3: the scan feeds the same share_expand path the table feeds in the bf16 modes."""
    sr = 16000
    e = Engine(synth_sd["dgrad"], precision="bf16x3")
    feat, _, _ = e.mel_frontend([synth.make_pcm(45, 10 * sr), synth.make_pcm(46, int(3.1 * sr), "speechlike")], sr)
    r = e.encoder(feat)
    d = e.distinct_columns(feat.shape[0])
    assert _same(r, _every_column(e, feat))
    assert d < 64 * feat.shape[0]


def test_kept_intermediates_run_every_column(synth_sd):
    """A keep-intermediates model is never deduplicated (the debug taps read the every-column layout): taps and outputs do not depend on
    the switch."""
    sr = 16000
    e = Engine(synth_sd["dgrad"], debug_keep=True)
    feat, _, _ = e.mel_frontend([synth.make_pcm(47, 2 * sr)], sr)
    n = feat.shape[0]
    r1 = e.encoder(feat)
    taps1 = [e.tap(k, n).clone() for k in range(4)]
    try:
        _lib.set_option("encoder_dedup_off", 1)
        r0 = e.encoder(feat)
        taps0 = [e.tap(k, n).clone() for k in range(4)]
    finally:
        _lib.set_option("encoder_dedup_off", 0)
    assert _same(r1, r0) and all(torch.equal(x, y) for x, y in zip(taps1, taps0))
    ship = Engine(synth_sd["dgrad"])
    assert _same(ship.encoder(feat), r0)
