"""The temporal track filters on the MI355X (sdfa_track_fir / sdfa_track_bilateral through sdfa_amd.tfilter) against the
float64 restatements of tests/tfilter_ref64.py: the FIR bit for bit, in both forms, at every width and clip length at which
the kernel takes another path; gaussian_filter1d against scipy itself; the bilateral filter within one float32 ulp of the
rounded double model; batch independence, NaN confinement and untouched memory around the output."""
import numpy as np
import pytest
import torch

import tfilter_ref64 as R
from sdfa_amd import tfilter

pytestmark = pytest.mark.gpu

# 1 .. 257: within one slab, the dword form; 1028: a slab and one float4 quad; 1029: a slab + 5 columns, dword form; 2056: three slabs, float4
WIDTHS = (1, 3, 255, 256, 257, 1028, 1029, tfilter.COLS + 5, 2 * tfilter.COLS + 8)
CLIPS = (1, 2, 3, 4, 5, 8, 9, 10, 31, 32, 33, 64, 65, 97)            # clip starts inside runs, clips shorter than the radius, run edges +- 1
OFF = np.concatenate(([0], np.cumsum(CLIPS))).astype(np.int64)
F = int(OFF[-1])
FIR_RADII = (0, 1, 4, 8, 9, 32)
BIL_RADII = (0, 1, 5, 10, 32)
SENTINEL = 0x7FC0BEEF


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_distance(a, b):
    """Distance in float32 steps between equal-shaped finite arrays."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def signal(W, amp, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(F)[:, None]
    x = np.sin(0.3 * t + rs.uniform(0, 6.28, (1, W))) + 0.3 * rs.normal(0, 1, (F, W))
    return (amp * x).astype(np.float32)


def taps_of(r, seed):
    w = np.random.RandomState(seed).uniform(0.1, 1.0, 2 * r + 1)
    w = (w + w[::-1]) / 2
    w = w / w.sum()
    w = (w + w[::-1]) / 2
    assert w.tobytes() == w[::-1].tobytes()
    return w


@pytest.mark.parametrize("W", WIDTHS)
def test_fir_is_bitwise_in_both_forms(W):
    x = signal(W, 1e-3, W)
    d = torch.from_numpy(x).cuda()
    for r in FIR_RADII:
        taps = taps_of(r, 100 + r)
        want = bits(R.fir_ref(x, taps, OFF))
        win = tfilter.correlate_symmetric(d, taps, OFF)
        gen = tfilter.correlate_symmetric(d, taps, OFF, generic=True)
        assert win.shape == d.shape and win.dtype == torch.float32
        assert np.array_equal(bits(win), want), (W, r, "window form")
        assert np.array_equal(bits(gen), want), (W, r, "generic form")


def test_fir_misaligned_rows_take_the_dword_form():
    W = 1028
    x = signal(W, 1e-3, 5)
    buf = torch.zeros(F * W + 8, device="cuda")
    obuf = torch.zeros(F * W + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    d = buf[1:1 + F * W].view(F, W)                                   # 4 bytes past a 16-byte boundary
    d.copy_(torch.from_numpy(x))
    for r in (4, 9):
        taps = taps_of(r, r)
        want = bits(R.fir_ref(x, taps, OFF))
        for o in (obuf[3:3 + F * W].view(F, W), obuf[4:4 + F * W].view(F, W)):       # misaligned and aligned outputs
            for generic in (False, True):
                got = tfilter.correlate_symmetric(d, taps, OFF, out=o, generic=generic)
                assert got.data_ptr() == o.data_ptr()
                assert np.array_equal(bits(got), want), (r, generic)


def test_gaussian_filter1d_is_scipy_on_an_offsets_clip():
    from scipy.ndimage import gaussian_filter1d
    x = np.random.RandomState(2).normal(0, 2e-3, (600, 15069)).astype(np.float32)
    want = gaussian_filter1d(x, sigma=1, axis=0)
    d = torch.from_numpy(x).cuda()
    got = tfilter.gaussian_filter1d(d, 1)
    assert np.array_equal(bits(got), bits(want))
    assert torch.equal(tfilter.gaussian_filter1d(d, 1, generic=True).view(torch.int32), got.view(torch.int32))
    assert np.array_equal(bits(tfilter.gaussian_filter1d(d.reshape(600, 5023, 3), 1)), bits(want).reshape(600, 5023, 3))


def test_more_clips_than_one_launch_carries():
    rs = np.random.RandomState(9)
    lens = rs.randint(1, 4, 2 * tfilter.CLIPS + 77)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    x = rs.normal(0, 1, (int(off[-1]), 37)).astype(np.float32)
    d = torch.from_numpy(x).cuda()
    taps = taps_of(2, 1)
    want = bits(R.fir_ref(x, taps, off))
    for generic in (False, True):
        assert np.array_equal(bits(tfilter.correlate_symmetric(d, taps, off, generic=generic)), want)
    wantb = R.bilateral_ref(x, 1.0, 1.0, 2, clip_frame_off=off)
    gotb = tfilter.bilateral(d, 1.0, 1.0, 2, clip_frame_off=off)
    assert ulp_distance(gotb.cpu().numpy(), wantb).max() <= 1
    assert torch.equal(tfilter.bilateral(d, 1.0, 1.0, 2, clip_frame_off=off, generic=True).view(torch.int32), gotb.view(torch.int32))


@pytest.mark.parametrize("amp", (1.0, 1e-3))
@pytest.mark.parametrize("W", WIDTHS)
def test_bilateral_within_one_ulp_in_both_forms(W, amp):
    x = signal(W, amp, 1000 + W)
    d = torch.from_numpy(x).cuda()
    for r in BIL_RADII:
        ds, rs = (1.0, 1.0) if r <= 5 else (5.0, 2.0)
        rs *= amp                                                      # the range sigma at the signal's scale
        want = R.bilateral_ref(x, ds, rs, r, clip_frame_off=OFF)
        win = tfilter.bilateral(d, ds, rs, r, clip_frame_off=OFF)
        gen = tfilter.bilateral(d, ds, rs, r, clip_frame_off=OFF, generic=True)
        dist = ulp_distance(win.cpu().numpy(), want)
        differ = float((dist > 0).mean())
        print(f"W {W} amp {amp:g} radius {r}: max distance {int(dist.max())} ulp, {differ:.2e} of the elements differ")
        assert dist.max() <= 1, (W, amp, r)
        assert differ <= 1e-4, (W, amp, r, differ)
        assert torch.equal(win.view(torch.int32), gen.view(torch.int32)), (W, amp, r)
        assert torch.equal(tfilter.bilateral(d, ds, rs, r, clip_frame_off=OFF).view(torch.int32), win.view(torch.int32))     # run to run


@pytest.mark.parametrize("W", (257, 1028))
def test_a_batch_is_its_clips_filtered_alone(W):
    x = signal(W, 1e-3, 7)
    d = torch.from_numpy(x).cuda()
    taps = taps_of(4, 3)
    fir = tfilter.correlate_symmetric(d, taps, OFF)
    big = tfilter.correlate_symmetric(d, taps_of(32, 4), OFF, generic=True)
    bil = tfilter.bilateral(d, 1.0, 1e-3, 5, clip_frame_off=OFF)
    for a, b in zip(OFF[:-1], OFF[1:]):
        part = d[a:b].clone()
        assert torch.equal(tfilter.correlate_symmetric(part, taps).view(torch.int32), fir[a:b].view(torch.int32))
        assert torch.equal(tfilter.correlate_symmetric(part, taps_of(32, 4)).view(torch.int32), big[a:b].view(torch.int32))
        assert torch.equal(tfilter.bilateral(part, 1.0, 1e-3, 5).view(torch.int32), bil[a:b].view(torch.int32))


@pytest.mark.parametrize("generic", (False, True))
def test_a_nan_poisons_its_window_and_stays_in_its_clip(generic):
    W = 259
    x = signal(W, 1.0, 11)
    clip = len(CLIPS) - 1                                              # the 97-frame clip, after the 65-frame one
    a, b = int(OFF[clip]), int(OFF[clip + 1])
    for pos, col in ((a + 1, 0), (a + 40, 258), (b - 1, 100)):
        y = x.copy()
        y[pos, col] = np.nan
        d = torch.from_numpy(y).cuda()
        for r in (4, 9):
            want = np.zeros((F, W), bool)
            want[max(a, pos - r):min(b, pos + r + 1), col] = True
            fir = tfilter.correlate_symmetric(d, taps_of(r, r), OFF, generic=generic).cpu().numpy()
            assert np.array_equal(np.isnan(fir), want), (pos, col, r, "fir")
            bil = tfilter.bilateral(d, 2.0, 1.0, r, clip_frame_off=OFF, generic=generic).cpu().numpy()
            assert np.array_equal(np.isnan(bil), want), (pos, col, r, "bilateral")
            clean = ~want
            assert np.array_equal(fir[clean].view(np.uint32), R.fir_ref(x, taps_of(r, r), OFF)[clean].view(np.uint32))


@pytest.mark.parametrize("W", (255, 1028))
def test_memory_around_the_output_is_untouched(W):
    guard = 64
    x = signal(W, 1e-3, 13)
    d = torch.from_numpy(x).cuda()
    for kind in ("fir", "bilateral"):
        for generic in (False, True):
            buf = torch.full((guard + F * W + guard,), SENTINEL, dtype=torch.int32, device="cuda")
            out = buf[guard:guard + F * W].view(torch.float32).view(F, W)
            if kind == "fir":
                tfilter.correlate_symmetric(d, taps_of(4, 1), OFF, out=out, generic=generic)
            else:
                tfilter.bilateral(d, 1.0, 1e-3, 5, clip_frame_off=OFF, out=out, generic=generic)
            assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[-guard:] == SENTINEL).all()), (kind, generic)
            assert not bool((buf[guard:-guard] == SENTINEL).any())


def test_refused_calls_leave_the_output_alone():
    from sdfa_amd._lib import SdfaError
    d = torch.zeros(10, 8, device="cuda")
    out = torch.full((10, 8), 3.0, device="cuda")
    with pytest.raises(SdfaError, match="overlap"):
        tfilter.gaussian_filter1d(d, 1, out=d)
    with pytest.raises(ValueError):
        tfilter.gaussian_filter1d(d, 1, clip_frame_off=[0, 5, 5, 10], out=out)
    assert bool((out == 3.0).all())
