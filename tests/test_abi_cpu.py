"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/sdfa_hip.h declares,
and its host-only entry point (frame enumeration) is bit-exact.  No GPU compute calls here."""
import os
import re

import numpy as np
import pytest

import sdfa_oracle as O
from sdfa_amd import _lib, engine, weights, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_all_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sdfa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sdfa_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.sdfa_abi_version() == _lib.ABI_VERSION == 5


def test_frame_index_matches_reference_fixtures(golden):
    ts = golden["tslist"]
    for key in ts.files:
        sr = int(key.split("_")[0][2:]); L = int(key.split("_L")[1])
        starts, tslist = engine.frame_index(L, sr)
        assert np.array_equal(tslist, ts[key]), key
        assert np.array_equal(starts, O.frame_index(L, sr)[0])


@pytest.mark.parametrize("sr", [8000, 16000])
def test_frame_index_matches_oracle_many_lengths(sr):
    rs = np.random.RandomState(5)
    _, _, sliding = engine.frame_geometry(sr)
    lengths = [sliding, sliding + 1, 10 * sr, 10 * sr + 1, 60 * sr + 7, 600 * sr + 13] + list(rs.randint(sliding, 40 * sr, 40))
    for L in lengths:
        s_c, t_c = engine.frame_index(int(L), sr)
        s_o, t_o = O.frame_index(int(L), sr)
        assert np.array_equal(s_c, s_o) and np.array_equal(t_c, t_o), L


def test_frame_count_of_baseline_clip():
    for L, sr in ((160000, 16000), (80000, 8000)):
        s, t = engine.frame_index(L, sr)
        assert len(s) == 636 and t[-1] == 10467     # SURVEY App. A.1 anchor
    s, t = engine.frame_index(32000, 16000)
    assert len(s) == 156 and list(t[:5]) == [-117, -100, -83, -67, -50]


def test_overlong_clip_is_refused_on_the_host():
    """the front-end kernels index samples in 32-bit arithmetic; a clip beyond 2^29 - 1 samples is refused where its
    length is known (sdfa_frame_index) instead of being truncated silently on the device."""
    from sdfa_amd._lib import SdfaError
    with pytest.raises(SdfaError, match="2\\^29"):
        engine.frame_index(2 ** 29, 16000)


def test_option_table_of_the_header_is_what_the_library_accepts():
    """The comment table next to sdfa_debug_set_option in include/sdfa_hip.h is the specification of the A/B options: the library
    accepts every name it documents (and no retired or unknown one) and enforces the documented ranges of the stream options."""
    hdr = open(os.path.join(ROOT, "include", "sdfa_hip.h")).read()
    comment = hdr[:hdr.index("int sdfa_debug_set_option(")].rsplit("/*", 1)[1]
    names = []
    for row in re.findall(r'^ \*   ("[a-z0-9_]+"(?: / "[a-z0-9_]+")*)', comment, flags=re.M):
        names += re.findall(r'"([a-z0-9_]+)"', row)
    assert len(names) == len(set(names)) >= 18, names
    set_option, last_error = _lib.lib.sdfa_debug_set_option, _lib.lib.sdfa_last_error
    try:
        for name in names:
            assert set_option(name.encode(), 0) == _lib.OK, (name, last_error())
        for name in ("pca_unfused", "conv_unfused", "no_such_option"):
            assert set_option(name.encode(), 0) == _lib.EINVAL, name
            assert b"unknown option" in last_error(), (name, last_error())
        refused = [("frontend_stream_block", 257), ("frontend_stream_block", -1), ("frontend_stream_slots", 257),
                   ("frontend_stream_slots", -1), ("frontend_stream_spin_max", -1)]
        for name, value in refused:
            assert name in names
            assert set_option(name.encode(), value) == _lib.EINVAL, (name, value)
            assert last_error().startswith(name.encode() + b": 0 (default) or "), (name, value, last_error())
    finally:
        for name in names:
            set_option(name.encode(), 0)


def test_short_clip_raises_like_reference():
    with pytest.raises(AssertionError):
        engine.frame_index(2400, 8000)
    engine.frame_index(9088, 16000)
    # same verdict as the oracle (which follows sliding_window.py:356-363) on every short length
    for sr in (8000, 16000):
        _, _, sliding = engine.frame_geometry(sr)
        for L in range(sliding - 700, sliding + 5, 3):
            try:
                ref = O.frame_index(L, sr)
            except AssertionError:
                ref = None
            if ref is None:
                with pytest.raises(AssertionError):
                    engine.frame_index(L, sr)
            else:
                got = engine.frame_index(L, sr)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_weight_norm_fold_matches_oracle(synth_sd):
    sd = synth_sd["dgrad"]
    folded = weights.fold_state_dict(sd)
    for key in ("_audio_encoder._layers.3", "_output_module._scale_layers.2"):
        ref = O.fold_weight_norm(sd, "_model." + key)
        assert np.array_equal(folded[key + ".weight"], ref)
    assert not any(k.endswith("weight_g") or k.endswith("weight_v") or "num_batches" in k for k in folded)
    assert weights.head_of(sd) == "dgrad" and weights.head_of(synth_sd["offsets"]) == "offsets"


def test_legacy_checkpoint_renames():
    ck = {"state": {"audio_encoder.layers.0.weight_v": 1, "anime_decoder.proj_scale.compT": 2,
                    "time_aggregator.layers.1.b": 3, "audio_encoder.layers.0._ext_batch_norm.weight": 4, "hamm": 0}}
    st = weights.ckpt_backward_compatible_preprocess(ck)["state"]
    assert set(st) == {"_model._audio_encoder._layers.1.weight_v", "_model._output_module._scale_pca.compT",
                       "_model._audio_encoder._layers.10.b", "_model._audio_encoder._layers.1._ext_post_bn.weight"}


# (frames, sdfa_workspace_bytes keep-intermediates off, on, sdfa_frontend_workspace_bytes), as the library returned them before the
# layouts' share-map tables and scratch offsets were given one definition each: the sizes are part of what callers allocate by
WORKSPACE_BYTES = [
    (1, 404727808, 526362624, 4359424),
    (128, 404727808, 526362624, 4359424),
    (129, 809446400, 1052716032, 8718592),
    (700, 2428320768, 3158129664, 26155520),
    (2048, 6475506944, 8421664000, 69747456),
    (8192, 25902000896, 33686629120, 278989056),
    (20352, 64350270208, 83690205952, 693113088),
]


def test_workspace_sizes_are_pinned_and_cover_the_share_tables():
    """Host code only: sdfa_workspace_bytes reads the model's keep flag and nothing else, so an unfinalised model will do."""
    lib = _lib.lib
    m = lib.sdfa_model_create(_lib.HEAD_DGRAD)
    assert m
    try:
        for n, keep_off, keep_on, frontend in WORKSPACE_BYTES:
            assert lib.sdfa_debug_keep_intermediates(m, 0) == _lib.OK
            assert lib.sdfa_workspace_bytes(m, n) == keep_off, n
            assert lib.sdfa_debug_keep_intermediates(m, 1) == _lib.OK
            assert lib.sdfa_workspace_bytes(m, n) == keep_on, n
            assert lib.sdfa_frontend_workspace_bytes(n) == frontend, n
            # What the share-map tables need (kernels.h: sdfa_share_table_words, written out again here): 16 counter words, prev / shift
            # [Nc], owner / flag / uid / col_src / col_to_u [Mc], one scan word per 1024 columns and one to spare.
            Nc = (n + 127) // 128 * 128
            Mc = 64 * Nc
            need = 16 + 2 * Nc + 5 * Mc + Mc // 1024 + 1
            # front end: the tables, then the mel table of 128 floats per column
            assert frontend % 4 == 0 and frontend // 4 - 128 * Mc >= need, n
            # encoder, nothing kept: every other region is a multiple of 64 words -- status 64, pool1 / conv3 2048 Mc each, the
            # frequency LSTM's hidden states 8192 Mc, query conv / query / context 512 + 128 + 512 Nc, regressor 2560 Nc, control 2048
            assert keep_off % 4 == 0 and keep_off // 4 - (64 + 12288 * Mc + 3712 * Nc + 2048) >= need, n
            # kept: 2048 + 2048 + 8192 + 256 + 2048 + 512 + 512 + 128 Mc, and the distinct-column projection's own 256 Mc
            assert keep_on % 4 == 0 and keep_on // 4 - (64 + 16000 * Mc + 3712 * Nc + 2048) >= need, n
    finally:
        lib.sdfa_model_destroy(m)
