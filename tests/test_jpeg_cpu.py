"""CPU checks of the GPU JPEG encoder's contract: the ABI of include/sdfa_jpeg.h is bound and exported, and the numpy
restatement of the encoder (tests/jpeg_oracle.py) writes exactly PIL's bytes (speech_anime.video.encode_jpeg) over the
size, quality and content matrix of tests/jpeg_cases.py, within the header's capacity bound."""
import os
import re

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_oracle as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jpeg_header_symbols_bound_and_exported():
    from sdfa_amd import jpeg, render, _lib
    hdr = open(os.path.join(ROOT, "include", "sdfa_jpeg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    declared = set(re.findall(r"\b(sdfa_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(jpeg.SYMBOLS), declared ^ set(jpeg.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.sdfa_jpeg_abi_version() == jpeg.ABI_VERSION == 1
    assert not declared & set(_lib.SYMBOLS), "jpeg symbols belong to their own header, not the core ABI"
    assert not declared & set(render.SYMBOLS), "jpeg symbols belong to their own header, not the render ABI"


def test_header_constants_match_the_oracle():
    hdr = open(os.path.join(ROOT, "include", "sdfa_jpeg.h")).read()
    assert re.search(r"#define SDFA_JPEG_ABI_VERSION 1\b", hdr)
    assert int(re.search(r"#define SDFA_JPEG_MAX_BLOCK_BITS\s+(\d+)", hdr).group(1)) == 1660 == 22 + 63 * 26


@pytest.mark.parametrize("quality", JC.QUALITIES)
@pytest.mark.parametrize("size", JC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_equals_pil(size, quality):
    from speech_anime.video import encode_jpeg
    w, h = size
    for kind in JC.CONTENTS:
        rgb = JC.frame(kind, w, h, seed=w * 7 + h)
        got, want = J.encode(rgb, quality), encode_jpeg(rgb, quality)
        assert got[:len(J.header(w, h, quality))] == want[:len(J.header(w, h, quality))], (kind, "header")
        assert got == want, (kind, len(got), len(want))


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
def test_oracle_equals_pil_on_a_rendered_flame_frame(golden, quality):
    from speech_anime.video import encode_jpeg
    rgb = JC.flame_frame(golden)
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 20            # a face, not a blank frame
    assert J.encode(rgb, quality) == encode_jpeg(rgb, quality)


def test_oracle_stages_against_pil_decoder():
    """The coefficients decode (PIL) to the frame up to JPEG's loss: the stages are not only self-consistent."""
    import io
    from PIL import Image
    rgb = JC.frame("gradient", 64, 48)
    dec = np.asarray(Image.open(io.BytesIO(J.encode(rgb, 95))).convert("RGB")).astype(int)
    assert np.abs(dec - rgb).mean() < 3.0


def test_dummy_blocks_and_fields():
    """Odd block extents make dummy luma blocks (AC zero, DC of the block before); every block's fields fit the bound."""
    rgb = JC.frame("noise", 17, 7, seed=3)                       # 3 x 1 luma blocks in 2 x 1 MCUs
    c = J.coefficients(rgb, 100)
    assert c.shape == (2, 6, 64)
    last = c[1]
    assert not last[1:4, 1:].any()
    assert last[1, 0] == last[0, 0] and last[2, 0] == last[1, 0] and last[3, 0] == last[1, 0]
    assert not c[0, 2:4, 1:].any() and c[0, 2, 0] == c[0, 1, 0] == c[0, 3, 0]
    c = J.coefficients(JC.frame("noise", 17, 9, seed=3), 100)    # 3 x 2 luma blocks: right dummies only
    assert not c[1, [1, 3], 1:].any() and c[1, 1, 0] == c[1, 0, 0] and c[1, 3, 0] == c[1, 2, 0]
    val, nbits = J.fields(c)
    assert nbits.sum(2).max() <= 63 and (val >> np.maximum(nbits, 0)).max() == 0


@pytest.mark.parametrize("size", [(16, 16), (33, 47), (512, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_at_q100_fits_the_capacity_bound(size):
    w, h = size
    rgb = JC.frame("noise", w, h, seed=11)
    out = J.encode(rgb, 100)
    n_blocks = 6 * J.geometry(w, h)[0] * J.geometry(w, h)[1]
    assert J.block_bits(J.coefficients(rgb, 100)).max() <= 1660
    assert len(out) <= J.max_frame_bytes(w, h) == len(J.header(w, h, 100)) + 2 * ((1660 * n_blocks + 7) // 8 + 1) + 2


def test_cli_accepts_jpeg_encoder_and_evaluate_rejects_unknown():
    from speech_anime.__main__ import _parser
    from speech_anime import video
    assert _parser().parse_args(["evaluate"]).jpeg_encoder == "pil"
    assert _parser().parse_args(["evaluate", "--jpeg_encoder", "gpu"]).jpeg_encoder == "gpu"
    with pytest.raises(SystemExit):
        _parser().parse_args(["evaluate", "--jpeg_encoder", "nvjpeg"])
    with pytest.raises(ValueError, match="encoder"):
        video.write_video("/nonexistent/x.avi", 0, None, 8, 8, 60, encoder="nvjpeg")
