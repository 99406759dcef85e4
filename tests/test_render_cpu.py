"""CPU checks of the evaluate-video feature: the render ABI (include/sdfa_render.h) is bound and exported, the numpy
restatement of the rasterizer (tests/render_oracle.py) obeys its own contract on analytic cases, the AVI writer round-trips,
the video frame count is the reference's loop, and --save_video without a template fails before any device work."""
import os
import re

import numpy as np
import pytest

import render_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- render ABI ----

def test_render_header_symbols_bound_and_exported():
    from sdfa_amd import render, _lib
    hdr = open(os.path.join(ROOT, "include", "sdfa_render.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    declared = set(re.findall(r"\b(sdfa_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(render.SYMBOLS), declared ^ set(render.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.sdfa_render_abi_version() == render.ABI_VERSION == 1
    assert not declared & set(_lib.SYMBOLS), "render symbols belong to their own header, not the core ABI"


def test_default_params_are_the_reference_rig():
    from sdfa_amd import render
    p = render.default_params()
    assert np.array_equal(np.asarray(p.cam_pose[:], np.float32), R.DEFAULT_PARAMS["cam_pose"].reshape(-1))
    for name in ("yfov", "znear", "ambient", "dir_intensity", "point_intensity"):
        assert np.float32(getattr(p, name)) == R.DEFAULT_PARAMS[name], name
    assert np.array_equal(np.asarray(p.albedo[:], np.float32), R.DEFAULT_PARAMS["albedo"])
    assert np.array_equal(np.asarray(p.background[:], np.float32), R.DEFAULT_PARAMS["background"])


# ---- oracle self-checks (screen space in 1/256 pixel) ----

def _scr(points):
    """[(x, y) in pixels] -> (V, 4) screen records with 1/w = 1."""
    s = np.zeros((len(points), 4), np.int32)
    s[:, 0] = np.rint(np.asarray(points)[:, 0] * 256)
    s[:, 1] = np.rint(np.asarray(points)[:, 1] * 256)
    s[:, 2] = np.float32(1.0).view(np.int32)
    s[:, 3] = 1
    return s


def _covered(scr, faces, W, H, samples=1):
    btri, _ = R.raster(scr, faces, W, H, samples)
    return btri != R.INT_MAX, btri


def test_analytic_triangle_covers_expected_pixel_centres():
    scr = _scr([(2.25, 2.25), (2.25, 12.25), (12.25, 2.25)])       # counter-clockwise in NDC (y up)
    cov, _ = _covered(scr, [(0, 1, 2)], 16, 16)
    y, x = np.mgrid[0:16, 0:16]
    expect = (x >= 2) & (y >= 2) & (x + y <= 13)
    assert np.array_equal(cov[:, :, 0], expect)


def test_back_facing_triangle_draws_nothing():
    scr = _scr([(2.25, 2.25), (12.25, 2.25), (2.25, 12.25)])       # the same triangle, clockwise in NDC
    for samples in (1, 4):
        cov, _ = _covered(scr, [(0, 1, 2)], 16, 16, samples)
        assert not cov.any()


def test_degenerate_and_invalid_triangles_are_dropped():
    scr = _scr([(2.5, 2.5), (8.5, 8.5), (14.5, 14.5), (2.5, 12.5)])
    assert not _covered(scr, [(0, 1, 2)], 16, 16)[0].any()         # zero area
    scr[3, 3] = 0                                                   # invalid vertex (behind the near plane, non-finite, ...)
    assert not _covered(scr, [(0, 3, 1)], 16, 16)[0].any()


@pytest.mark.parametrize("samples", [1, 4])
def test_two_triangle_square_covers_every_sample_once(samples):
    # corners on pixel centres: every sample of the diagonal and of the outer edges lies exactly on an edge
    a, b, c, d = (4.5, 4.5), (4.5, 20.5), (20.5, 20.5), (20.5, 4.5)
    scr = _scr([a, b, c, d])
    t0, t1 = (0, 1, 2), (0, 2, 3)
    c0 = _covered(scr, [t0], 24, 24, samples)[0]
    c1 = _covered(scr, [t1], 24, 24, samples)[0]
    assert not (c0 & c1).any(), "a sample on the shared edge is covered twice"
    offs = np.asarray(R.SAMPLES[samples], np.float64) / 16.0
    y, x = np.mgrid[0:24, 0:24]
    sx = x[:, :, None] + 0.5 + offs[None, None, :, 0]
    sy = y[:, :, None] + 0.5 + offs[None, None, :, 1]
    inside = (sx > 4.5) & (sx < 20.5) & (sy > 4.5) & (sy < 20.5)
    assert np.array_equal((c0 | c1) & inside, inside), "a sample inside the square is missed"
    both = _covered(scr, [t0, t1], 24, 24, samples)[0]
    assert np.array_equal(both, c0 | c1)


def test_lattice_grid_covers_every_sample_once():
    # a 6 x 6 grid of quads with vertices on sample positions, each quad split along alternating diagonals:
    # samples on edges and on shared vertices must be covered by exactly one triangle
    n, step, o = 6, 3, 2.5
    pts = [(o + step * i, o + step * j) for j in range(n + 1) for i in range(n + 1)]
    faces = []
    for j in range(n):
        for i in range(n):
            v00, v10, v01, v11 = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            if (i + j) % 2:
                faces += [(v00, v01, v11), (v00, v11, v10)]
            else:
                faces += [(v00, v01, v10), (v10, v01, v11)]
    scr = _scr(pts)
    count = np.zeros((24, 24), np.int64)
    for f in faces:
        count += _covered(scr, [f], 24, 24)[0][:, :, 0]
    y, x = np.mgrid[0:24, 0:24]
    inside = (x + 0.5 > o) & (x + 0.5 < o + step * n) & (y + 0.5 > o) & (y + 0.5 < o + step * n)
    assert count.max() <= 1
    assert (count[inside] == 1).all()


def test_point_on_the_camera_axis_projects_to_the_image_centre():
    template = np.array([[0.1, 0.0, 0.0], [0.0, 0.05, 0.0], [0.0, 0.0, -0.02]], np.float32)
    W, H = 512, 384
    k = R.consts(template, W, H)
    pose = R.DEFAULT_PARAMS["cam_pose"].astype(np.float64)
    p = pose[:3, 3] - 0.4 * pose[:3, 2]                 # 0.4 in front of the camera, along its -Z
    v = (p / float(k["s"])).astype(np.float32)[None]
    scr, _ = R.vertex_stage(v, k)
    assert scr[0, 3] == 1
    assert abs(int(scr[0, 0]) - W * 128) <= 2 and abs(int(scr[0, 1]) - H * 128) <= 2
    iw = scr[0, 2:3].view(np.float32)[0]
    assert abs(1.0 / iw - 0.4) < 1e-5


def test_vertex_behind_the_near_plane_or_nan_is_invalid():
    template = np.array([[0.1, 0.0, 0.0], [0.0, 0.05, 0.0]], np.float32)
    k = R.consts(template, 64, 64)
    pose = R.DEFAULT_PARAMS["cam_pose"].astype(np.float64)
    near = pose[:3, 3] - 0.01 * pose[:3, 2]
    behind = pose[:3, 3] + 0.3 * pose[:3, 2]
    v = np.stack([near / float(k["s"]), behind / float(k["s"]), [np.nan, 0, 0]]).astype(np.float32)
    scr, _ = R.vertex_stage(v, k)
    assert (scr[:, 3] == 0).all()


# ---- AVI writer ----

def _frames(n, H=48, W=64):
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for i in range(n):
        img = np.stack([128 + 100 * np.sin((x + 3 * i) / 9.0), 128 + 100 * np.cos((y - 2 * i) / 7.0), 60 + 2 * x + i], -1)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_avi_round_trip(tmp_path):
    from PIL import Image
    import io
    from scipy.io import wavfile
    from speech_anime import video, audio
    fps, n, sr = 60.0, 25, 44100
    frames = _frames(n)
    sound = (0.3 * np.sin(np.arange(int(n / fps * sr) + 777) * 0.01)).astype(np.float32)
    sound[::97] = 1.5                                                   # clipped like write_wav clips
    path = str(tmp_path / "clip.avi")
    w = video.AviWriter(path, 64, 48, fps, n, audio.pcm16(sound), sr)
    for f in frames:
        w.write_jpeg(video.encode_jpeg(f))
    w.close()
    r = video.read_avi(path)
    assert r["avih"]["total_frames"] == n and r["avih"]["us_per_frame"] == round(1e6 / fps)
    assert r["avih"]["streams"] == 2 and (r["avih"]["width"], r["avih"]["height"]) == (64, 48)
    assert r["streams"] == [(b"vids", b"MJPG"), (b"auds", b"\0\0\0\0")]
    assert len(r["video"]) == n
    for jpg, ref in zip(r["video"], frames):
        dec = np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))
        assert dec.shape == ref.shape and _psnr(dec, ref) >= 35.0
    audio.write_wav(str(tmp_path / "audio.wav"), sound, sr)
    _, pcm = wavfile.read(str(tmp_path / "audio.wav"))
    assert np.array_equal(r["audio"], pcm)
    kinds = [e[0] for e in r["index"]]
    assert kinds.count(b"00dc") == n and kinds[0] == b"00dc" and kinds[1] == b"01wb"
    data = open(path, "rb").read()
    movi = data.index(b"movi")
    for fcc, _, off, size in r["index"]:                               # idx1 offsets point at the chunks (from 'movi')
        assert data[movi + off:movi + off + 4] == fcc
        assert int.from_bytes(data[movi + off + 4:movi + off + 8], "little") == size


def test_avi_without_audio_and_empty_track(tmp_path):
    from speech_anime import video
    path = str(tmp_path / "v.avi")
    w = video.AviWriter(path, 64, 48, 30.0, 2)
    for f in _frames(2):
        w.write_jpeg(video.encode_jpeg(f))
    w.close()
    r = video.read_avi(path)
    assert r["avih"]["streams"] == 1 and len(r["video"]) == 2 and len(r["audio"]) == 0


def test_avi_refuses_above_the_size_limit(tmp_path):
    from speech_anime import video
    path = str(tmp_path / "big.avi")
    w = video.AviWriter(path, 64, 48, 60.0, 50, max_bytes=20000)
    with pytest.raises(ValueError, match="AVI 1.0"):
        for f in _frames(50):
            w.write_jpeg(video.encode_jpeg(f))
    assert not os.path.exists(path)
    assert video.AVI1_LIMIT == 1 << 30


# ---- video frame count ----

def _render_video_loop(max_ts, video_fps):
    """speech_anime/viewer/video.py:211-275, literally."""
    ts = 0
    delta_ts = 1000.0 / float(video_fps)
    frames = 0
    while ts < max_ts:
        frames += 1
        ts += delta_ts
    return frames


def test_video_frame_count_is_the_reference_loop():
    from speech_anime import video
    from sdfa_amd import seek
    rs = np.random.RandomState(3)
    lasts = [10000, 1000, 5000, 20000, 60000, 16, 17, 33, 34, 1, 0, -117] + list(rs.randint(1, 120000, 200))
    for fps in (60, 30, 25):
        for last in lasts:
            k = video.video_frame_count(int(last), fps)
            assert k == _render_video_loop(int(last), fps), (last, fps)
            assert k <= seek.query_count(int(last), fps), (last, fps)
    assert video.video_frame_count(10000, 60) == _render_video_loop(10000, 60)


# ---- --save_video needs --template_mesh ----

def test_save_video_without_template_fails_up_front(tmp_path):
    from speech_anime import api, viewer
    from speech_anime.__main__ import _parser
    viewer.clear_template()
    ns = _parser().parse_args(["evaluate", "--save_video", "--load_from", str(tmp_path / "missing.ckpt"),
                               "--output_dir", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="--template_mesh"):
        api.evaluate_model(ns)
    assert not os.path.exists(tmp_path / "out")


def test_model_evaluate_save_video_without_template_fails_up_front(tmp_path):
    from speech_anime import viewer
    from speech_anime.api import build_model
    from speech_anime.hparams import configure
    viewer.clear_template()
    model = build_model(configure({}))                 # no weights: the template check comes before everything else
    with pytest.raises(ValueError, match="--template_mesh"):
        model.evaluate({"test": [["x.wav"]]}, save_video=True, output_dir=str(tmp_path))
