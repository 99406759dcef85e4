"""speech_anime.datasets.dgrad.generate_dgrad on the MI355X: a small offsets data root -> the dgrad data root the reference's
generate_dgrad (preload.py:765-835) writes, checked against the reference's own rows (tests/golden/track_filter.npz, fixture
(b)) and against the float64 models of both steps; resumption by the _audio marker; refusals; and that the PCA step accepts
the result."""
import os

import numpy as np
import pytest

import tfilter_ref64 as R
from dgrad_ref64 import deform_grad64
from ply_cases import write_ply

pytestmark = pytest.mark.gpu

BOUND = 1e-9            # tests/test_deform_grad_gpu.py, its preload case
NAMES = ["-00001.npy", "000000.npy", "000001.npy", "000002.npy", "000003.npy", "000004.npy"]


def _tree(root, golden):
    g = golden["mesh_flame"]
    z = golden["track_filter"]
    os.makedirs(root / "templates")
    write_ply(root / "templates" / "subject_a.ply", g["verts"], g["faces"])
    src = root / "offsets"
    for clip, frames in (("000", dict(zip(NAMES, z["dgrad_offsets"]))), ("007", {"000010.npy": z["dgrad_offsets"][2]})):
        d = src / "data" / "m0" / "neutral" / clip
        os.makedirs(d)
        for name, row in frames.items():
            np.save(d / name, row)
        np.save(d / "000000_lips_dist.npy", np.float32(0.004))
        np.save(d / "info_lips_dist.npy", np.arange(3, dtype=np.float32))
        np.save(d / "notes.npy", np.zeros(2))                           # neither a frame nor a lips file: not converted, not copied
        (src / "data" / "m0" / "neutral" / (clip + "_audio")).write_bytes(b"RIFF" + bytes(range(40)) + clip.encode())
    os.makedirs(src / "data" / "m0" / "neutral" / "009")                 # no _audio beside it: not a clip
    (src / "train.csv").write_text("speaker:str,npy_data_path:path\nm0,data/m0/neutral/000\n")
    (src / "valid.csv").write_text("speaker:str,npy_data_path:path\nm0,data/m0/neutral/007\n")
    return src, root / "dgrad", root / "templates"


def _files(root):
    return {os.path.relpath(os.path.join(d, n), root): os.stat(os.path.join(d, n)).st_mtime_ns for d, _, names in os.walk(root) for n in names}


def test_generate_dgrad_writes_the_references_root(tmp_path, golden):
    from speech_anime.datasets.dgrad import generate_dgrad
    from speech_anime.datasets.vocaset_mask import non_face_tris
    src, dst, templates = _tree(tmp_path, golden)
    done = generate_dgrad(str(src), str(dst), str(templates), speaker_alias={"m0": "subject_a"})
    assert sorted(done) == [("m0", "neutral", "000"), ("m0", "neutral", "007")]

    g, z = golden["mesh_flame"], golden["track_filter"]
    V, faces = g["verts"].astype(np.float32), g["faces"]
    mask = non_face_tris(faces)
    clip = dst / "data" / "m0" / "neutral" / "000"
    assert sorted(os.listdir(clip)) == sorted(NAMES + ["000000_lips_dist.npy", "info_lips_dist.npy"])
    rows = np.stack([np.load(clip / n) for n in NAMES])
    assert rows.dtype == np.float32 and rows.shape == (6, 89784)
    one = np.load(dst / "data" / "m0" / "neutral" / "007" / "000010.npy")
    assert one.dtype == np.float32 and one.shape == (89784,)
    assert sorted(os.listdir(dst / "data" / "m0" / "neutral")) == ["000", "000_audio", "007", "007_audio"]

    tri = rows.reshape(6, -1, 9)
    assert np.all(tri[:, mask] == 0) and np.all(one.reshape(-1, 9)[mask] == 0)            # masked: exact zeros
    st = int(z["dgrad_stride"])
    err_ref = float(np.abs(tri[:, ::st].astype(np.float64) - z["dgrad_rows"].astype(np.float64)).max())
    smooth = R.gaussian_ref(z["dgrad_offsets"], 1)
    model = np.stack([deform_grad64(V, (V + s.reshape(-1, 3)).astype(np.float32), faces, 1e-6) for s in smooth]).reshape(6, -1, 9)
    model[:, mask] = 0
    err_model = float(np.abs(tri.astype(np.float64) - model.astype(np.float32).astype(np.float64)).max())
    lone = deform_grad64(V, (V + z["dgrad_offsets"][2].reshape(-1, 3)).astype(np.float32), faces, 1e-6).reshape(-1, 9)   # one frame: the filter is the identity
    lone[mask] = 0
    err_one = float(np.abs(one.reshape(-1, 9).astype(np.float64) - lone.astype(np.float32).astype(np.float64)).max())
    print(f"max|rows - reference rows| = {err_ref:.2e} (every {st}th triangle); max|rows - float32(model)| = {err_model:.2e}; one-frame clip {err_one:.2e}")
    assert err_ref <= BOUND
    assert err_model <= BOUND
    assert err_one <= BOUND

    for rel in ("data/m0/neutral/000_audio", "data/m0/neutral/007_audio", "data/m0/neutral/000/000000_lips_dist.npy",
                "data/m0/neutral/007/info_lips_dist.npy", "train.csv", "valid.csv"):
        assert (dst / rel).read_bytes() == (src / rel).read_bytes(), rel
    assert not (dst / "test.csv").exists()

    # a second run converts nothing and rewrites no clip file
    before = _files(dst / "data")
    assert generate_dgrad(str(src), str(dst), str(templates), speaker_alias={"m0": "subject_a"}) == []
    assert _files(dst / "data") == before
    # without its completion marker exactly that clip is redone
    os.remove(dst / "data" / "m0" / "neutral" / "007_audio")
    assert generate_dgrad(str(src), str(dst), str(templates), speaker_alias={"m0": "subject_a"}) == [("m0", "neutral", "007")]
    after = _files(dst / "data")
    assert set(after) == set(before)
    changed = {k for k in after if after[k] != before[k]}
    assert changed == {"m0/neutral/007_audio", "m0/neutral/007/000010.npy", "m0/neutral/007/000000_lips_dist.npy", "m0/neutral/007/info_lips_dist.npy"}
    assert np.array_equal(np.load(dst / "data" / "m0" / "neutral" / "007" / "000010.npy"), one)

    # the PCA step takes the root
    from speech_anime.datasets.pca import load_chunks
    chunks = load_chunks(str(dst))
    assert len(chunks) == 1 and tuple(chunks[0].shape) == (6, 89784)
    assert np.array_equal(chunks[0].cpu().numpy(), rows)


def test_a_non_flame_template_is_refused_before_anything_is_written(tmp_path, golden):
    from speech_anime.datasets.dgrad import generate_dgrad
    src, dst, templates = _tree(tmp_path, golden)
    g = golden["mesh_flame"]
    write_ply(templates / "subject_a.ply", g["verts"][:-1], g["faces"][(g["faces"] < len(g["verts"]) - 1).all(1)])
    with pytest.raises(ValueError, match="FLAME topology"):
        generate_dgrad(str(src), str(dst), str(templates), speaker_alias={"m0": "subject_a"})
    assert not dst.exists()
    with pytest.raises(FileNotFoundError, match="FaceTalk_170728_03272_TA"):        # VOCASET's name of m0, the default alias
        generate_dgrad(str(src), str(dst), str(templates))
    with pytest.raises(ValueError):
        generate_dgrad(str(src), str(dst), str(templates), sigma=0.0, speaker_alias={"m0": "subject_a"})
    assert not dst.exists()


def test_the_command_line(tmp_path, golden):
    from speech_anime.datasets import dgrad
    src, dst, templates = _tree(tmp_path, golden)
    os.rename(templates / "subject_a.ply", templates / "FaceTalk_170728_03272_TA.ply")
    dgrad.main(["--offsets_root", str(src), "--dgrad_root", str(dst), "--templates_dir", str(templates), "--sigma", "1"])
    assert np.load(dst / "data" / "m0" / "neutral" / "000" / "-00001.npy").shape == (89784,)
