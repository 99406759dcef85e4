"""The table-less encoder call groups ALL bit-equal columns of a workspace chunk under one owner (csrc/share.hip: hash + table insert ->
look-up + full compare), wherever in the chunk the copies are.  Reference side of every comparison: the same call with
"encoder_dedup_off" = 1 (the every-column arithmetic) for the bits, and a recount on the host -- np.unique over the chunk's columns as
384-word bit patterns -- for the number of distinct columns.  Never the scan itself.  All comparisons are bitwise."""
import numpy as np
import pytest
import torch

from sdfa_amd import synth, _lib
from sdfa_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _with(e, feat, **opts):
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        r = e.encoder(feat)
        d = None if opts.get("encoder_dedup_off") else e.distinct_columns(_last_chunk(feat.shape[0], e.max_frames))
        return r, d
    finally:
        for k in opts:
            _lib.set_option(k, 0)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _last_chunk(n, max_frames):
    return n - (n - 1) // max_frames * max_frames


def _host_distinct(feat, last):
    """Distinct columns of the last `last` frames: a column is its 384 words as a bit pattern (-0.0 != +0.0)."""
    cols = np.ascontiguousarray(feat[feat.shape[0] - last:].cpu().numpy()).reshape(-1, 384).view(np.uint32)
    return len(np.unique(cols.view(np.dtype((np.void, 384 * 4)))))


@pytest.fixture(scope="module")
def engines(synth_sd):
    return {mf: Engine(synth_sd["dgrad"], max_frames=mf) for mf in (8192, 128)}


@pytest.fixture(scope="module")
def inputs(engines):
    """name -> (features, the every-column result): computed once, never modified."""
    e = engines[8192]
    clip = synth.make_pcm(43, int(3.3 * 16000), "speechlike")
    pcm = {
        "two_clips_16k": ([synth.make_pcm(70, 2 * 16000, "uniform"), synth.make_pcm(71, int(1.3 * 16000), "speechlike")], 16000),
        "one_clip_8k": ([synth.make_pcm(72, 2 * 8000, "uniform")], 8000),
        "clip_twice": ([clip, clip], 16000),
    }
    out = {}
    for name, (clips, sr) in pcm.items():
        feat = e.mel_frontend(clips, sr)[0].clone()
        out[name] = (feat, _with(e, feat, encoder_dedup_off=1)[0])
    return out


@pytest.mark.parametrize("max_frames", [8192, 128])
@pytest.mark.parametrize("name", ["two_clips_16k", "one_clip_8k"])
def test_count_equals_host_recount(engines, inputs, name, max_frames):
    """Exactly the distinct bit patterns of the (last) chunk are evaluated, and the rows are those of evaluating every column.  At 128
    frames per chunk the call takes several chunks: a group never crosses a chunk, so the recount is over the last chunk alone."""
    e = engines[max_frames]
    feat, ref = inputs[name]
    n = feat.shape[0]
    last = _last_chunk(n, max_frames)
    r, d = _with(e, feat)
    host = _host_distinct(feat, last)
    print(f"{name} max_frames {max_frames}: {n} frames, last chunk {last}: distinct columns {d}, host recount {host} of {64 * last}")
    assert d == host < 64 * last
    assert _same(r, ref)
    assert e.time_lstm_repairs() == 0


def test_distant_copies_are_grouped(engines, inputs):
    """Two copies of a 3.3 s clip in one batch: the copies are more than 64 frames apart and are found all the same."""
    e = engines[8192]
    feat, ref = inputs["clip_twice"]
    n = feat.shape[0]
    h = n // 2
    assert h > 64 and torch.equal(feat[:h], feat[h:])
    r, d = _with(e, feat)
    host = _host_distinct(feat, n)
    print(f"clip twice, {n} frames: distinct columns {d}, host recount {host}, of the first copy alone {_host_distinct(feat[:h], h)}")
    assert d == host == _host_distinct(feat[:h], h)
    assert _same(r, ref)
    assert torch.equal(r[0][:h], r[0][h:])


def test_chunks_of_equal_columns(engines):
    """Every column on one slot of the table: all-zero features are 1 distinct column, one random frame repeated 256 times is 64."""
    e = engines[8192]
    zeros = torch.zeros((300, 64, 128, 3), device="cuda")
    r, d = _with(e, zeros)
    assert d == 1
    assert _same(r, _with(e, zeros, encoder_dedup_off=1)[0])
    one = torch.rand((1, 64, 128, 3), generator=torch.Generator().manual_seed(5)).cuda()
    rep = one.expand(256, 64, 128, 3).contiguous()
    r, d = _with(e, rep)
    assert d == 64
    assert _same(r, _with(e, rep, encoder_dedup_off=1)[0])
    assert e.time_lstm_repairs() == 0


@pytest.mark.parametrize("bits", [6, 1])
def test_colliding_hashes_cost_columns_not_bits(engines, inputs, bits):
    """"share_hash_bits" keeps only the low bits of the hash (32 different values at 6, a single one at 1), so that nearly every look-up
    names a column of other content: the full compare refuses those, the rows stay those of evaluating every column, and a refused
    column is evaluated on its own -- the count lies between the host recount and every column."""
    e = engines[8192]
    feat, ref = inputs["two_clips_16k"]
    n = feat.shape[0]
    host = _host_distinct(feat, n)
    r, d = _with(e, feat, share_hash_bits=bits)
    print(f"share_hash_bits {bits}: distinct columns {d}, host recount {host}, columns {64 * n}")
    assert _same(r, ref)
    assert host <= d <= 64 * n
    r, d = _with(e, feat)                                            # the option was reset: the exact count again
    assert d == host and _same(r, ref)


def test_colliding_hashes_link_no_random_columns(engines):
    """torch.rand features have no two equal columns; with 32 hash values for 19,200 columns every column but 32 is compared with
    another in full, and every one stays distinct."""
    e = engines[8192]
    n = 300
    feat = torch.rand((n, 64, 128, 3), generator=torch.Generator().manual_seed(11)).cuda()
    r, d = _with(e, feat, share_hash_bits=6)
    assert d == 64 * n
    assert _same(r, _with(e, feat, encoder_dedup_off=1)[0])


def test_two_calls_agree(engines, inputs):
    """The owner of a group is its smallest column index, whatever order the table's atomics land in: same count, same bits."""
    e = engines[8192]
    feat, ref = inputs["clip_twice"]
    r1, d1 = _with(e, feat)
    r2, d2 = _with(e, feat)
    assert d1 == d2 and _same(r1, r2) and _same(r1, ref)
