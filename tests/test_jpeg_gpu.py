"""The GPU JPEG encoder (csrc/jpeg.hip via sdfa_amd.jpeg) against its numpy restatement (tests/jpeg_oracle.py) and against
PIL (speech_anime.video.encode_jpeg): coefficients bitwise, files byte for byte, and the evaluate video with either encoder."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import jpeg_oracle as J

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def _batch(w, h, n, seed):
    kinds = JC.CONTENTS
    return np.stack([JC.frame(kinds[(i + seed) % len(kinds)], w, h, seed=seed * 1000 + i) for i in range(n)])


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
@pytest.mark.parametrize("size", JC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coefficients_bitwise(size, quality):
    from sdfa_amd.jpeg import JpegEncoder
    w, h = size
    frames = _batch(w, h, 4, seed=1)
    enc = JpegEncoder(w, h, quality)
    got = enc.coefficients(_cuda(frames)).cpu().numpy()
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], J.coefficients(f, quality)), i


@pytest.mark.parametrize("size", JC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_and_capacity(size):
    from sdfa_amd.jpeg import JpegEncoder
    w, h = size
    for q in (1, 90):
        enc = JpegEncoder(w, h, q)
        assert enc.header == J.header(w, h, q)
        assert enc.max_frame_bytes == J.max_frame_bytes(w, h)


@pytest.mark.parametrize("quality", JC.QUALITIES)
@pytest.mark.parametrize("size", JC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_equals_pil_batch_1_and_3(size, quality):
    from sdfa_amd.jpeg import JpegEncoder
    from speech_anime.video import encode_jpeg
    w, h = size
    enc = JpegEncoder(w, h, quality)
    for n, seed in ((1, 0), (3, 1), (3, 2)):
        frames = _batch(w, h, n, seed)
        got = enc.encode(_cuda(frames))
        assert len(got) == n
        for i in range(n):
            assert got[i] == encode_jpeg(frames[i], quality), (n, seed, i)


@pytest.mark.parametrize("size", [(1, 1), (17, 9), (300, 170), (512, 512), (8192, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("quality", [75, 100])
def test_encode_equals_pil_batch_64(size, quality):
    from sdfa_amd.jpeg import JpegEncoder
    from speech_anime.video import encode_jpeg
    w, h = size
    frames = _batch(w, h, 64, seed=5)
    got = JpegEncoder(w, h, quality).encode(_cuda(frames))
    assert [len(g) for g in got] == [len(encode_jpeg(f, quality)) for f in frames]
    for i, f in enumerate(frames):
        assert got[i] == encode_jpeg(f, quality), i


def test_batch_independence_and_determinism():
    from sdfa_amd.jpeg import JpegEncoder
    frames = _batch(300, 170, 64, seed=9)
    enc = JpegEncoder(300, 170, 90)
    whole = enc.encode(_cuda(frames))
    again = enc.encode(_cuda(frames))
    assert whole == again
    for i in (0, 17, 63):
        assert enc.encode(_cuda(frames[i:i + 1]))[0] == whole[i]
    shuffled = frames[::-1].copy()
    assert enc.encode(_cuda(shuffled)) == whole[::-1]
    assert enc.encode(_cuda(frames[:0])) == []


def test_more_frames_than_one_chunk():
    from sdfa_amd import render
    from sdfa_amd.jpeg import JpegEncoder
    from speech_anime.video import encode_jpeg
    n = render.CHUNK_FRAMES + 5
    frames = _batch(33, 47, n, seed=4)
    got = JpegEncoder(33, 47, 95).encode(_cuda(frames))
    assert len(got) == n and all(got[i] == encode_jpeg(frames[i], 95) for i in range(n))


def test_rendered_flame_frames_512_samples4(golden):
    from sdfa_amd.jpeg import JpegEncoder
    from sdfa_amd.render import Renderer
    from speech_anime.video import encode_jpeg
    g = golden["mesh_flame"]
    verts = np.stack([g["verts"]] + list(g["mesh"])).astype(np.float32)
    rgb = Renderer(g["verts"].astype(np.float32), g["faces"].astype(np.uint32), (512, 512), samples=4).render(torch.from_numpy(verts).cuda())
    host = rgb.cpu().numpy()
    got = JpegEncoder(512, 512, 90).encode(rgb)
    for i in range(len(host)):
        assert got[i] == encode_jpeg(host[i], 90), i


def test_write_video_gpu_equals_pil(tmp_path):
    from speech_anime import video
    frames = _cuda(_batch(200, 120, 77, seed=3))
    sound = np.sin(np.arange(44100) * 0.01).astype(np.float32) * 0.5
    paths = {}
    for encoder in ("pil", "gpu"):
        paths[encoder] = str(tmp_path / f"{encoder}.avi")
        video.write_video(paths[encoder], 77, lambda i0, i1: frames[i0:i1], 200, 120, 60.0, sound=sound, chunk=32, encoder=encoder)
    assert open(paths["pil"], "rb").read() == open(paths["gpu"], "rb").read()
    assert len(video.read_avi(paths["gpu"])["video"]) == 77


def _setup_clip(tmp_path, golden, synth_sd, seconds):
    from scipy.io import wavfile
    from sdfa_amd import synth
    from speech_anime import viewer
    g = golden["mesh_flame"]
    sr = 16000
    wav = tmp_path / "speech@clip0.wav"
    wavfile.write(str(wav), sr, (synth.make_pcm(6, int(seconds * sr)) * 32767).astype(np.int16))
    ck = tmp_path / "epoch0050.ckpt"
    torch.save({"epoch": 50, "global_step": 1, "state": {k: torch.from_numpy(np.array(v)) for k, v in synth_sd["dgrad"].items()}}, str(ck))
    hpj = tmp_path / "hparams.json"
    hpj.write_text('{"audio": {"sample_rate": 16000}}')
    obj = tmp_path / "flame.obj"
    viewer.write_obj(str(obj), g["verts"].astype(np.float32), g["faces"].astype(np.uint32))
    cn = tmp_path / "flame_cnsts.txt"
    cn.write_text(" ".join(str(int(i)) for i in g["cnsts"]) + "\n")
    return dict(wav=str(wav), ck=str(ck), hpj=str(hpj), obj=str(obj), cn=str(cn))


def test_evaluate_cli_process_gpu_equals_pil(tmp_path, golden, synth_sd):
    import subprocess
    import sys
    c = _setup_clip(tmp_path, golden, synth_sd, 1.0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "sdfa-2019_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    avi = {}
    for encoder in ("pil", "gpu"):
        out = tmp_path / f"results_{encoder}"
        cmd = [sys.executable, "-m", "speech_anime", "evaluate", "--load_from", c["ck"], "--custom_hparams", c["hpj"],
               "--output_dir", str(out), "--eval_input", c["wav"], "--eval_spk_cond", "m1", "--template_mesh", c["obj"],
               "--mesh_constraints", c["cn"], "--save_video", "--grid_w", "160", "--grid_h", "128", "--jpeg_encoder", encoder]
        r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        avi[encoder] = (out / "speech@clip0.avi").read_bytes()
    assert len(avi["pil"]) > 10000 and avi["gpu"] == avi["pil"]
