"""Layer 1 of the time BiLSTM as ONE kernel that contracts [x_t | h] itself (csrc/lstm.hip: time_lstm_fused_kernel, option
"time_lstm_fuse_x" = 2 / 3: 32- / 64-frame tiles) against the two-kernel path of the same build (option 1: input-projection GEMM +
time_lstm_kernel).  The fused loop adds an accumulator's products in the GEMM's order and then the recurrent ones as before, so z and
align of Engine.encoder are compared as bit patterns: no tolerance.  "time_lstm_split" = 1 keeps the small-batch cooperating forms out
of the way, so that the single-workgroup recurrence is what runs at these sizes on both sides.

Sizes: 128 frames = two 64-frame tiles per direction (both directions, step 0 without the h part, the slice hand-over of all 8 + 4
trips); 200 frames (256 columns per step) = padding frames in the last tile; 64 frames = the smallest launch."""
import numpy as np
import pytest
import torch

from sdfa_amd import synth, _lib
from sdfa_amd.engine import Engine

pytestmark = pytest.mark.gpu

SIZES = (64, 128, 200)


def _bits(e, feat, **opts):
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        z, align = e.encoder(feat)
        return z.cpu().numpy().view(np.uint32), align.cpu().numpy().view(np.uint32)
    finally:
        for k in opts:
            _lib.set_option(k, 0)


@pytest.fixture(scope="module")
def engine(synth_sd):
    return Engine(synth_sd["dgrad"], max_frames=256)


@pytest.fixture(scope="module")
def cases(engine):
    """(source, frames) -> (features, options of the source, two-kernel result): computed once, never modified."""
    front = engine.mel_frontend([synth.make_pcm(43, int(3.3 * 16000), "speechlike")], 16000)[0].clone()
    assert front.shape[0] >= max(SIZES)
    g = torch.Generator().manual_seed(7)
    rnd = (torch.randn(front[:max(SIZES)].shape, generator=g) * float(front.std()) + float(front.mean())).cuda()   # the front end's range
    out = {}
    for n in SIZES + (156,):
        for src, feat, opts in (("pcm", front, {}), ("randn", rnd, {"encoder_dedup_off": 1})):
            f = feat[:n].contiguous()
            out[src, n] = (f, opts, _bits(engine, f, time_lstm_fuse_x=1, time_lstm_split=1, **opts))
    return out


@pytest.mark.parametrize("form", [2, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("src", ["pcm", "randn"])
def test_fused_is_bitwise_the_two_kernel_path(engine, cases, src, n, form):
    feat, opts, ref = cases[src, n]
    z, align = _bits(engine, feat, time_lstm_fuse_x=form, time_lstm_split=1, **opts)
    dz, da = int((z != ref[0]).sum()), int((align != ref[1]).sum())
    print(f"{src} {n} frames, time_lstm_fuse_x {form}: {dz} of {z.size} z words and {da} of {align.size} align words differ")
    assert np.isfinite(z.view(np.float32)).all()
    assert dz == 0 and da == 0


@pytest.mark.parametrize("src", ["pcm", "randn"])
def test_default_options_single_clip(engine, cases, src):
    """A single clip's 156 frames under default options: the by-size rule leaves the small-batch forms alone, and whatever runs gives the
    bits of the two-kernel path."""
    feat, opts, ref = cases[src, 156]
    z, align = _bits(engine, feat, **opts)
    assert np.array_equal(z, ref[0]) and np.array_equal(align, ref[1])
    assert engine.time_lstm_repairs() == 0
