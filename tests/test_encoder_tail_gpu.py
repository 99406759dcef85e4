"""The shared-column encoder's frequency projection in two launches leaves every bit where it was (csrc/share.hip, csrc/gemm_tail.hip):
"freq_proj_tail": the column tiles behind the last whole round of the persistent projection GEMM go to a fine-tile kernel (0 = device-side
rule, 1 = never, 2 = always).
Reference side of every comparison: the same call with "encoder_dedup_off" = 1, the every-column arithmetic -- never the code under
test.  All comparisons are bitwise (torch.equal) on z and align."""
import contextlib

import pytest
import torch

from sdfa_amd import synth, _lib
from sdfa_amd.engine import Engine

pytestmark = pytest.mark.gpu

OPTIONS = ("encoder_dedup_off", "freq_proj_tail")


@contextlib.contextmanager
def _options(**kw):
    assert set(kw) <= set(OPTIONS)
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k in kw:
            _lib.set_option(k, 0)


def _run(e, feat, table=None, **opts):
    """(z, align), distinct columns of the call's last chunk"""
    with _options(**opts):
        r = e.encoder(feat) if table is None else e.encoder(feat, frame_clip=table[0], frame_start=table[1], hop=table[2])
        n = feat.shape[0]
        last = n - (n - 1) // e.max_frames * e.max_frames
        d = None if opts.get("encoder_dedup_off") else e.distinct_columns(last)
    return r, d


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture(scope="module")
def eng(synth_sd):
    return Engine(synth_sd["dgrad"])


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rand_frames(g):
    """frame counts whose 256-column tiles (n / 4 of them: torch.rand columns are all distinct) are whole rounds of a grid of g
    workgroups, and whole rounds + about g / 8, g / 2 and 7 g / 8 tiles; at least 2,048 frames, where the fat kernel starts"""
    k = max(2, -(-512 // g))
    return [4 * (k * g + r) for r in (0, g // 8, g // 2, 7 * g // 8)]


def test_rand_frame_counts_on_256_cus():
    assert _rand_frames(256) == [2048, 2176, 2560, 2944]


@pytest.mark.parametrize("which", range(4))
def test_random_features_every_tail_size_and_mode(synth_sd, which):
    """torch.rand features: the identity map, so the tail is known exactly -- none, g / 8, g / 2 and 7 g / 8 tiles.  Rule, never and
    always give the every-column bits, and every column stays distinct."""
    n = _rand_frames(_cus())[which]
    e = Engine(synth_sd["dgrad"], max_frames=n)
    feat = torch.rand((n, 64, 128, 3), generator=torch.Generator().manual_seed(100 + which)).cuda()
    ref, _ = _run(e, feat, encoder_dedup_off=1)
    for mode in (0, 1, 2):
        r, d = _run(e, feat, freq_proj_tail=mode)
        assert _same(r, ref), (n, mode)
        assert d == 64 * n, (n, mode, d)
    assert e.time_lstm_repairs() == 0


def test_reserved_cus_change_the_grid(synth_sd):
    """sdfa_model_set_reserved_cus(16): the persistent grid, and with it the split point, is 16 workgroups smaller."""
    g = _cus() - 16
    n = 4 * (max(2, -(-512 // g)) * g + g // 2)
    e = Engine(synth_sd["dgrad"], max_frames=n)
    feat = torch.rand((n, 64, 128, 3), generator=torch.Generator().manual_seed(7)).cuda()
    ref, _ = _run(e, feat, encoder_dedup_off=1)
    e.set_reserved_cus(16)
    for mode in (2, 0, 1):
        r, d = _run(e, feat, freq_proj_tail=mode)
        assert _same(r, ref), mode
        assert d == 64 * n
    n2 = _rand_frames(_cus())[1]                       # a tail for the full grid, another one for the smaller grid
    r, d = _run(e, feat[:n2], freq_proj_tail=2)
    e.set_reserved_cus(0)
    assert _same(r, _run(e, feat[:n2], encoder_dedup_off=1)[0]) and d == 64 * n2


VARIANTS = [dict(freq_proj_tail=1), dict(freq_proj_tail=2)]


@pytest.mark.parametrize("sr,seconds,max_frames", [
    (16000, [2.0], 8192),                        # the sizes of tests/test_encoder_dedup_gpu.py
    (16000, [10.0, 3.1], 8192),
    (16000, [10.0, 10.0, 4.0], 8192),
    (16000, [10.0] * 5 + [1.3], 8192),
    (16000, [10.0] * 14, 16384),
    (16000, [10.0] * 4, 1024),                   # several workspace chunks per call
    (8000, [10.0, 3.1], 8192),                   # hop 64
    (16000, [2.37, 0.613, 5.003, 1.0], 8192),    # ragged batch
    (16000, [10.0] * 32, 8192),                  # the headline batch: chunks of 8,192, 8,192 and 3,968 frames
])
def test_frontend_features_every_option_same_bits_same_count(synth_sd, sr, seconds, max_frames):
    """Front-end features through the scan and through the frame table: default == every column, and the tail never / always
    changes neither a bit nor the number of distinct columns."""
    e = Engine(synth_sd["dgrad"], max_frames=max_frames)
    clips = [synth.make_pcm(70 + i, int(s * sr), "speechlike" if i % 2 else "uniform") for i, s in enumerate(seconds)]
    feat, _, _ = e.mel_frontend(clips, sr)
    table = e.last_frame_table
    ref, _ = _run(e, feat, encoder_dedup_off=1)
    r0, d0 = _run(e, feat)
    rt, dt = _run(e, feat, table=table)
    print(f"sr {sr} frames {feat.shape[0]} chunk {max_frames}: distinct columns of the last chunk, scan {d0} table {dt}")
    assert _same(r0, ref) and _same(rt, ref)
    assert d0 <= dt
    for v in VARIANTS:
        r, d = _run(e, feat, **v)
        assert _same(r, ref), v
        assert d == d0, (v, d, d0)
        r, d = _run(e, feat, table=table, **v)
        assert _same(r, ref), ("table", v)
        assert d == dt, ("table", v, d, dt)
    assert e.time_lstm_repairs() == 0


def test_adversarial_inputs_below_the_fat_kernel(eng):
    """All-zero features, one frame repeated 256 times, shuffled frames (chunks too small for the fat kernel): forcing the tail changes
    neither a bit nor the count."""
    sr = 16000
    zeros = torch.zeros((700, 64, 128, 3), device="cuda")
    one = torch.rand((1, 64, 128, 3), generator=torch.Generator().manual_seed(5)).cuda()
    feat, _, _ = eng.mel_frontend([synth.make_pcm(42, 2 * sr)], sr)
    two, _, _ = eng.mel_frontend([synth.make_pcm(43, int(3.3 * sr), "speechlike"), synth.make_pcm(44, 2 * sr)], sr)
    perm = torch.randperm(two.shape[0], generator=torch.Generator().manual_seed(7)).cuda()
    cases = {"zeros": zeros, "rand frame x 256": one.expand(256, 64, 128, 3).contiguous(),
             "front-end frame x 256": feat[17:18].expand(256, 64, 128, 3).contiguous(), "shuffled": two[perm].contiguous()}
    for name, x in cases.items():
        ref, _ = _run(eng, x, encoder_dedup_off=1)
        r0, d0 = _run(eng, x)
        r1, d1 = _run(eng, x, freq_proj_tail=2)
        print(f"{name}: {x.shape[0]} frames, distinct columns {d0}")
        assert _same(r0, ref) and _same(r1, ref), name
        assert d0 == d1, (name, d0, d1)
    assert eng.time_lstm_repairs() == 0


def test_other_configurations_take_the_path_they_took(synth_sd):
    """A bf16x3 engine and a keep-intermediates engine never take the tail path: forcing it changes nothing."""
    sr = 16000
    clips = [synth.make_pcm(45 + i, 10 * sr, "speechlike" if i % 2 else "uniform") for i in range(4)]
    e = Engine(synth_sd["dgrad"], precision="bf16x3")
    feat, _, _ = e.mel_frontend(clips, sr)
    assert feat.shape[0] >= 2048
    ref, _ = _run(e, feat, encoder_dedup_off=1)
    r0, d0 = _run(e, feat)
    r2, d2 = _run(e, feat, freq_proj_tail=2)
    r3, d3 = _run(e, feat, freq_proj_tail=1)
    assert _same(r0, ref) and _same(r2, ref) and _same(r3, ref)
    assert d0 == d2 == d3 < 64 * feat.shape[0]
    k = Engine(synth_sd["dgrad"], debug_keep=True)
    small = feat[:2048].contiguous()             # large enough for the fat kernel, whose grid a split would cut short
    rk = k.encoder(small)
    with _options(freq_proj_tail=2):
        assert _same(k.encoder(small), rk)
        fc, fs, hop = e.last_frame_table
        assert _same(k.encoder(small, frame_clip=fc[:2048], frame_start=fs[:2048], hop=hop), rk)
