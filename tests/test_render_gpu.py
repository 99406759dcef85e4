"""The GPU rasterizer (csrc/render.hip via sdfa_amd.render) against its numpy restatement (tests/render_oracle.py) on the FLAME
topology of tests/golden/mesh_flame.npz, and the evaluate video (--save_video) end to end."""
import io
import os

import numpy as np
import pytest
import torch

import render_oracle as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def flame(golden):
    g = golden["mesh_flame"]
    return dict(verts=g["verts"].astype(np.float32), faces=g["faces"].astype(np.uint32), cnsts=g["cnsts"], mesh=g["mesh"].astype(np.float32))


def _rotated(verts, seed):
    rs = np.random.RandomState(seed)
    axis = rs.randn(3)
    axis /= np.linalg.norm(axis)
    ang = rs.uniform(0.3, 0.8)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    c = verts.mean(0)
    return ((verts - c) @ Rm.T + c).astype(np.float32)


@pytest.fixture(scope="module")
def frames(flame):
    return np.stack([flame["verts"]] + list(flame["mesh"]) + [_rotated(flame["verts"], 7)])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.mark.parametrize("normals", ["template", "frame"])
def test_screen_visibility_bitwise_and_colour_samples1(flame, frames, normals):
    from sdfa_amd.render import Renderer
    r = Renderer(flame["verts"], flame["faces"], (512, 512), samples=1, normals=normals)
    scr = r.screen(_cuda(frames)).cpu().numpy()
    rgb, ids = r.render(_cuda(frames), want_ids=True)
    rgb, ids = rgb.cpu().numpy(), ids.cpu().numpy()
    for i, v in enumerate(frames):
        o_rgb, o_ids, o_scr = R.render(flame["verts"], flame["faces"], v, 512, 512, 1, normals)
        assert np.array_equal(scr[i], o_scr), f"frame {i}: snapped screen positions differ"
        assert np.array_equal(ids[i], o_ids), f"frame {i}: visibility differs at {np.argwhere(ids[i] != o_ids)[:5]}"
        assert (o_ids >= 0).sum() > 10000, "the face should cover a good part of the image"
        d = np.abs(rgb[i].astype(np.int32) - o_rgb.astype(np.int32)).max()
        assert d <= 1, f"frame {i}: colour differs by {d}"


def test_colour_samples4(flame, frames):
    from sdfa_amd.render import Renderer
    r = Renderer(flame["verts"], flame["faces"], (512, 512), samples=4)
    rgb, ids = r.render(_cuda(frames), want_ids=True)
    rgb, ids = rgb.cpu().numpy(), ids.cpu().numpy()
    for i, v in enumerate(frames):
        o_rgb, o_ids, _ = R.render(flame["verts"], flame["faces"], v, 512, 512, 4, "template")
        assert np.array_equal(ids[i], o_ids), f"frame {i}: visibility of sample 0 differs"
        d = np.abs(rgb[i].astype(np.int32) - o_rgb.astype(np.int32)).max()
        assert d <= 1, f"frame {i}: colour differs by {d}"


def test_non_square_image_and_partial_tiles(flame, frames):
    from sdfa_amd.render import Renderer
    r = Renderer(flame["verts"], flame["faces"], (300, 170), samples=1)
    rgb, ids = r.render(_cuda(frames[:2]), want_ids=True)
    assert rgb.shape == (2, 170, 300, 3)
    for i in range(2):
        o_rgb, o_ids, _ = R.render(flame["verts"], flame["faces"], frames[i], 300, 170, 1)
        assert np.array_equal(ids[i].cpu().numpy(), o_ids)
        assert np.abs(rgb[i].cpu().numpy().astype(np.int32) - o_rgb.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("samples", [1, 4])
def test_watertight_camera_facing_grid(samples):
    from sdfa_amd.render import Renderer
    n = 128
    pose = R.DEFAULT_PARAMS["cam_pose"].astype(np.float64)
    u = np.linspace(-0.12, 0.12, n + 1)
    gx, gy = np.meshgrid(u, u)
    cam = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -0.4)], 1)          # a plane facing the camera
    world = cam @ pose[:3, :3].T + pose[:3, 3]
    verts = (world * (0.15 / np.abs(world).max())).astype(np.float32)             # the scale 0.15 / max|v| then maps it back
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            faces += [(a, b, d), (a, d, c)]                                         # counter-clockwise seen from +Z
    r = Renderer(verts, np.asarray(faces, np.uint32), (256, 256), samples=samples)
    _, ids = r.render(_cuda(verts[None]), want_ids=True)
    cov = ids[0].cpu().numpy() >= 0
    assert cov.sum() > 0.3 * cov.size
    for line in list(cov) + list(cov.T):                   # the projected grid is convex: coverage of a row / column has no hole
        idx = np.flatnonzero(line)
        if len(idx):
            assert idx[-1] - idx[0] + 1 == len(idx), "background pixel inside the grid"


def test_batch_independence_and_determinism(flame, frames):
    from sdfa_amd.render import Renderer
    rs = np.random.RandomState(11)
    batch = np.stack([frames[i % len(frames)] + rs.normal(0, 1e-3, frames[0].shape).astype(np.float32) for i in range(37)])
    r = Renderer(flame["verts"], flame["faces"], (256, 256), samples=4)
    v = _cuda(batch)
    whole = r.render(v).cpu().numpy()
    again = r.render(v).cpu().numpy()
    split = np.concatenate([r.render(v[:1]).cpu().numpy(), r.render(v[1:]).cpu().numpy()])
    chunks = np.concatenate([r.render(v[i:i + 5]).cpu().numpy() for i in range(0, 37, 5)])
    assert np.array_equal(whole, again)
    assert np.array_equal(whole, split)
    assert np.array_equal(whole, chunks)


def test_frame_normals_on_template_equal_template_normals(flame):
    from sdfa_amd.render import Renderer
    v = _cuda(flame["verts"][None])
    a = Renderer(flame["verts"], flame["faces"], (512, 512), samples=4, normals="template").render(v)
    b = Renderer(flame["verts"], flame["faces"], (512, 512), samples=4, normals="frame").render(v)
    assert torch.equal(a, b)


def test_near_plane_and_nan_triangles_are_dropped(flame):
    from sdfa_amd.render import Renderer
    v = flame["verts"].copy()
    k = R.consts(flame["verts"], 256, 256)
    pose = R.DEFAULT_PARAMS["cam_pose"].astype(np.float64)
    faces = flame["faces"].astype(np.int64)
    _, o_ids0, _ = R.render(flame["verts"], flame["faces"], v, 256, 256, 1)
    seen = np.unique(o_ids0[o_ids0 >= 0])
    nan_v, near_v = faces[seen[0], 0], faces[seen[len(seen) // 2], 1]        # vertices of visible triangles
    v[nan_v] = np.nan
    v[near_v] = ((pose[:3, 3] - 0.01 * pose[:3, 2]) / float(k["s"])).astype(np.float32)    # in front of the camera, before znear
    r = Renderer(flame["verts"], flame["faces"], (256, 256), samples=1)
    rgb, ids = r.render(_cuda(v[None]), want_ids=True)
    ids = ids[0].cpu().numpy()
    _, o_ids, o_scr = R.render(flame["verts"], flame["faces"], v, 256, 256, 1)
    assert o_scr[nan_v, 3] == 0 and o_scr[near_v, 3] == 0
    assert np.array_equal(ids, o_ids)
    bad = np.flatnonzero(((faces == nan_v) | (faces == near_v)).any(1))
    assert not np.isin(ids, bad).any(), "a triangle with a dropped vertex was drawn"
    empty = r.render(torch.empty((0, len(v), 3), device="cuda"))
    assert empty.shape == (0, 256, 256, 3)


def test_render_track_equals_render_of_track_to_mesh(flame):
    from speech_anime import viewer
    from sdfa_amd.seek import SeekPlan
    viewer.set_dgrad_static(flame["verts"], flame["faces"], list(flame["cnsts"]))
    rs = np.random.RandomState(2)
    ts = list(range(-117, 1200, 17))
    plan = SeekPlan([ts], 60.0)
    rows = torch.from_numpy((rs.normal(0, 0.03, (len(ts), viewer.N_MODEL_TRIS * 9))).astype(np.float32)).cuda()
    img = viewer.render_track(rows, plan, (256, 256))
    ref = viewer.renderer((256, 256)).render(viewer.track_to_mesh(rows, plan))
    assert img.shape == (plan.n_queries, 256, 256, 3) and torch.equal(img, ref)
    assert torch.equal(viewer.render_track(rows, plan, (256, 256), n=5), ref[:5])
    # the offsets head: seek, + template on the device, render
    offs = torch.from_numpy(rs.normal(0, 1e-3, (len(ts), len(flame["verts"]) * 3)).astype(np.float32)).cuda()
    img = viewer.render_track(offs, plan, (256, 256), face_data_type="verts_off_3d")
    verts = plan.rows(offs).reshape(plan.n_queries, -1, 3) + _cuda(flame["verts"])[None]
    assert torch.equal(img, viewer.renderer((256, 256)).render(verts))
    one = viewer.render_frame(flame["mesh"][0], "verts_3d", (256, 256))
    assert np.array_equal(one, viewer.renderer((256, 256)).render(_cuda(flame["mesh"][:1]))[0].cpu().numpy())
    viewer.clear_template()


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def _setup_clip(tmp_path, flame, synth_sd, seconds):
    from scipy.io import wavfile
    from sdfa_amd import synth
    from speech_anime import viewer
    sr = 16000
    wav = tmp_path / "speech@clip0.wav"
    wavfile.write(str(wav), sr, (synth.make_pcm(6, int(seconds * sr)) * 32767).astype(np.int16))
    ck = tmp_path / "epoch0050.ckpt"
    torch.save({"epoch": 50, "global_step": 1, "state": {k: torch.from_numpy(np.array(v)) for k, v in synth_sd["dgrad"].items()}}, str(ck))
    hpj = tmp_path / "hparams.json"
    hpj.write_text('{"audio": {"sample_rate": 16000}}')
    obj = tmp_path / "flame.obj"
    viewer.write_obj(str(obj), flame["verts"], flame["faces"])
    cn = tmp_path / "flame_cnsts.txt"
    cn.write_text(" ".join(str(int(i)) for i in flame["cnsts"]) + "\n")
    return dict(wav=str(wav), ck=str(ck), hpj=str(hpj), obj=str(obj), cn=str(cn))


def test_evaluate_save_video(tmp_path, flame, synth_sd):
    import filecmp
    from PIL import Image
    from scipy.io import wavfile
    from speech_anime import viewer, video
    from speech_anime.api import evaluate_model
    from speech_anime.datasets import DatasetSlidingWindow
    from sdfa_amd.seek import SeekPlan
    c = _setup_clip(tmp_path, flame, synth_sd, 2.0)
    outs = {}
    for sv in (False, True):
        DatasetSlidingWindow.hparams = None
        viewer.clear_template()
        out = tmp_path / f"out_{int(sv)}"
        evaluate_model(dict(mode="evaluate", load_from=c["ck"], custom_hparams=c["hpj"], output_dir=str(out), eval_input=c["wav"],
                            eval_spk_cond="m1", template_mesh=c["obj"], mesh_constraints=c["cn"], export_mesh_frames=True,
                            save_video=sv, grid_w=256, grid_h=192))
        outs[sv] = out
    d0, d1 = outs[False] / "speech@clip0", outs[True] / "speech@clip0"
    assert not (outs[False] / "speech@clip0.avi").exists()
    names = sorted(os.listdir(d0))
    assert names == sorted(os.listdir(d1)) and len(names) > 10
    _, mismatch, errors = filecmp.cmpfiles(str(d0), str(d1), names, shallow=False)
    assert not mismatch and not errors, "save_video changed the other files"
    avi = video.read_avi(str(outs[True] / "speech@clip0.avi"))
    ts = np.load(d1 / "tslist.npy")
    K = video.video_frame_count(int(ts[-1]), 60)
    plan = SeekPlan([list(ts)], 60.0)
    assert 0 < K <= plan.n_queries
    assert avi["avih"]["total_frames"] == K and len(avi["video"]) == K
    assert (avi["avih"]["width"], avi["avih"]["height"]) == (256, 192)
    track = torch.from_numpy(np.load(d1 / "dgrad_3d.npy").astype(np.float32)).cuda().reshape(len(ts), -1)
    ref = viewer.renderer((256, 192)).render(viewer.track_to_mesh(track, plan)[:K]).cpu().numpy()
    for k in range(K):
        dec = np.asarray(Image.open(io.BytesIO(avi["video"][k])).convert("RGB"))
        assert _psnr(dec, ref[k]) >= 35.0, k
    _, pcm = wavfile.read(str(d1 / "audio.wav"))
    assert np.array_equal(avi["audio"], pcm)
    viewer.clear_template()


def test_evaluate_save_video_cli_process(tmp_path, flame, synth_sd):
    import subprocess
    import sys
    from speech_anime import video
    c = _setup_clip(tmp_path, flame, synth_sd, 1.0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "sdfa-2019_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "results_flame"
    cmd = [sys.executable, "-m", "speech_anime", "evaluate", "--load_from", c["ck"], "--custom_hparams", c["hpj"], "--output_dir", str(out),
           "--eval_input", c["wav"], "--eval_spk_cond", "m1", "--template_mesh", c["obj"], "--mesh_constraints", c["cn"],
           "--save_video", "--grid_w", "128", "--grid_h", "128"]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ts = np.load(out / "speech@clip0" / "tslist.npy")
    avi = video.read_avi(str(out / "speech@clip0.avi"))
    K = video.video_frame_count(int(ts[-1]), 60)
    assert avi["avih"]["total_frames"] == K == len(avi["video"]) and avi["avih"]["streams"] == 2
    from speech_anime import audio
    _, sound = audio.load_source(c["wav"], 16000, return_sound=True)
    assert np.array_equal(avi["audio"], audio.pcm16(sound))            # all of the 44.1 kHz sound, as audio.wav would hold it
    assert not (out / "speech@clip0" / "audio.wav").exists()
