"""The GPU OBJ formatter (csrc/obj.hip, sdfa_amd.obj) against the integer oracle (tests/obj_oracle.py) and against the files
speech_anime.viewer.write_obj writes: byte for byte, over tile-edge vertex counts, misaligned blocks, the capacity bound, the
out-of-domain flag and the host path behind it, chunking, and `evaluate --export_mesh_frames` with both heads."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import obj_oracle as O

pytestmark = pytest.mark.gpu

KINDS = ("edges", "patterns", "normal")


@pytest.fixture(scope="module")
def pool():
    """One pool of values per kind, generated once; a case takes the first n * V * 3 of it."""
    need = 3 * 5023 * 3
    edges = O.edge_values()
    return {"edges": np.tile(edges, need // len(edges) + 1)[:need], "patterns": O.domain_patterns(need, 21),
            "normal": O.normal_values(need, 22)}


def _faces(V):
    i = np.arange(max(V - 2, 0), dtype=np.uint32)
    return np.stack([i, i + 1, i + 2], 1) if V >= 3 else np.zeros((0, 3), np.uint32)


def _written(tmp_path, verts, faces):
    from speech_anime.viewer import write_obj
    p = tmp_path / "ref.obj"
    write_obj(str(p), verts, faces)
    return p.read_bytes()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 5023])
def test_vertex_blocks_equal_oracle_and_write_obj(V, n, pool, tmp_path):
    from sdfa_amd.obj import ObjFormatter, format_faces
    fmt = ObjFormatter(V)
    faces = _faces(V)
    for kind in KINDS:
        verts = pool[kind][:n * V * 3].reshape(n, V, 3)
        blocks, flags = fmt.format(torch.from_numpy(verts).cuda())
        assert flags == [False] * n, kind
        for i in range(n):
            assert blocks[i] == O.vertex_block(verts[i]), (kind, i)
        assert blocks[n - 1] + format_faces(faces, V) == _written(tmp_path, verts[n - 1], faces), kind


def _raw_format(verts, front=0, slack=64):
    """sdfa_obj_format_verts itself, the output `front` bytes into a 0xAA-filled buffer of exactly the capacity bound
    plus `slack`: returns (buffer, offsets, lengths, flags) on the host."""
    from sdfa_amd import obj
    from sdfa_amd._lib import check
    lib = obj.lib
    n, V = verts.shape[:2]
    d = torch.from_numpy(np.ascontiguousarray(verts)).cuda()
    cap = int(lib.sdfa_obj_max_frame_bytes(V)) * n
    buf = torch.full((front + cap + slack,), 0xAA, dtype=torch.uint8, device="cuda")
    offs, lens = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    flags = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sdfa_obj_workspace_bytes(V, n)), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    check(lib.sdfa_obj_format_verts(p(d), n, V, C.c_void_p(buf.data_ptr() + front), cap, p(offs), p(lens), p(flags), p(ws), ws.numel(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy().tobytes(), offs.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("V,n", [(1, 4), (257, 3)])
def test_blocks_at_odd_offsets(V, n, pool):
    """Frame 0 is all zero: 29 bytes per vertex, so every later block -- and every tile in it -- starts at an odd address."""
    verts = pool["patterns"][:n * V * 3].reshape(n, V, 3).copy()
    verts[0] = 0
    buf, offs, lens, flags = _raw_format(verts)
    assert lens[0] == 29 * V and offs[1] % 2 == 1
    assert np.array_equal(offs, np.cumsum(lens) - lens) and not flags.any()
    for i in range(n):
        assert buf[offs[i]:offs[i] + lens[i]] == O.vertex_block(verts[i]), i
    total = int(lens.sum())
    assert buf[total:] == b"\xaa" * (len(buf) - total)


@pytest.mark.parametrize("front", [0, 1, 13])
def test_longest_lines_fill_the_capacity_exactly(front):
    V, n = 257, 2
    verts = np.full((n, V, 3), -2147483520.0, np.float32)
    buf, offs, lens, flags = _raw_format(verts, front=front)
    assert lens.tolist() == [59 * V] * n and offs.tolist() == [0, 59 * V] and not flags.any()
    line = b"v -2147483520.000000 -2147483520.000000 -2147483520.000000\n"
    assert buf[:front] == b"\xaa" * front                       # an unaligned output: nothing before it is touched
    assert buf[front:front + n * 59 * V] == line * (n * V)
    assert buf[front + n * 59 * V:] == b"\xaa" * 64              # and nothing after the bound


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 2.0 ** 31], ids=["nan", "inf", "-inf", "2p31"])
def test_out_of_domain_frame_is_flagged_and_written_by_the_host(value, pool, tmp_path):
    from sdfa_amd.obj import ObjFormatter, ObjWriter
    from speech_anime.viewer import write_obj
    V = 300
    verts = pool["normal"][:3 * V * 3].reshape(3, V, 3).copy()
    verts[1, 277, 1] = value                                    # in the second tile of frame 1
    d = torch.from_numpy(verts).cuda()
    blocks, flags = ObjFormatter(V).format(d)
    assert flags == [False, True, False]
    assert blocks[0] == O.vertex_block(verts[0]) and blocks[2] == O.vertex_block(verts[2])
    assert len(blocks[1]) <= 59 * V
    faces = _faces(V)
    w = ObjWriter(faces, V)
    paths = [str(tmp_path / f"{i}.obj") for i in range(3)]
    w.write(paths, d)
    assert (w.device_frames, w.host_frames) == (2, 1)
    for i in range(3):
        write_obj(str(tmp_path / "want.obj"), verts[i], faces)
        assert open(paths[i], "rb").read() == (tmp_path / "want.obj").read_bytes(), i


def test_chunk_boundary(pool, tmp_path):
    from sdfa_amd.obj import ObjWriter
    V, n = 257, 5
    verts = pool["patterns"][:n * V * 3].reshape(n, V, 3)
    d = torch.from_numpy(verts).cuda()
    faces = _faces(V)
    files = {}
    for chunk in (None, 2):
        w = ObjWriter(faces, V)
        if chunk:
            w.chunk = chunk
        assert w.chunk == (chunk or 64)
        paths = [str(tmp_path / f"c{chunk}_{i}.obj") for i in range(n)]
        w.write(paths, d)
        assert (w.device_frames, w.host_frames) == (n, 0)
        files[chunk] = [open(p, "rb").read() for p in paths]
    assert files[2] == files[None]
    assert files[2][4] == O.vertex_block(verts[4]) + O.face_block(faces)


def test_write_obj_frames_caches_the_writer_per_template(golden, pool, tmp_path):
    from speech_anime import viewer
    g = golden["mesh_flame"]
    viewer.set_dgrad_static(g["verts"], g["faces"], list(g["cnsts"]))
    try:
        V = len(g["verts"])
        verts = (g["verts"][None] + pool["normal"][:2 * V * 3].reshape(2, V, 3)).astype(np.float32)
        w = viewer.write_obj_frames(str(tmp_path), torch.from_numpy(verts).cuda(), viewer.template_faces())
        assert w is viewer.obj_writer("cuda:0") and w.device_frames == 2
        assert (tmp_path / "000001.obj").read_bytes() == _written(tmp_path, verts[1], g["faces"])
        viewer.set_dgrad_static(g["verts"], g["faces"], list(g["cnsts"]))
        assert viewer.obj_writer("cuda:0") is not w                # a new template: a new writer
    finally:
        viewer.clear_template()
    assert not viewer._obj_writers


@pytest.mark.parametrize("head", ["dgrad", "offsets"])
def test_evaluate_export_mesh_frames(head, tmp_path, golden, synth_sd):
    """One clip just over the minimum length on the FLAME template: every NNNNNN.obj is write_obj of the expected vertices
    (dgrad head: seek + solve; offsets head without a source mesh: template + seeked offsets), all formatted on the device."""
    from scipy.io import wavfile
    from sdfa_amd import synth
    from sdfa_amd.seek import SeekPlan
    from speech_anime import viewer
    from speech_anime.api import build_model
    from speech_anime.datasets import DatasetSlidingWindow
    from speech_anime.hparams import configure
    g = golden["mesh_flame"]
    sr = 16000
    wav = tmp_path / "clip.wav"
    wavfile.write(str(wav), sr, (synth.make_pcm(3, 9600) * 32767).astype(np.int16))       # 0.6 s
    hp = configure(dict(mode="evaluate", custom_hparams=head))
    hp.audio.set_key("sample_rate", sr)
    DatasetSlidingWindow.hparams = None
    model = build_model(hp, synth_sd[head])
    viewer.clear_source_mesh()
    viewer.set_dgrad_static(g["verts"], g["faces"], list(g["cnsts"]))
    try:
        res = model.evaluate({"test": [[str(wav)]]}, output_dir=str(tmp_path / "out"), export_mesh_frames=True)
        _, tslist, animes = res[0]
        d = tmp_path / "out" / "clip"
        n = len([p for p in os.listdir(d) if p.endswith(".obj")])
        assert n > 10 and n == len([p for p in os.listdir(d) if p.endswith("_dgrad.npy")])
        if head == "dgrad":
            track = torch.from_numpy(np.ascontiguousarray(animes, dtype=np.float32)).cuda().reshape(len(tslist), -1)
            expect = viewer.track_to_mesh(track, SeekPlan([list(tslist)], model.hp.anime.fps)).cpu().numpy()
        else:
            rows = np.stack([np.load(d / f"{i:06d}_dgrad.npy") for i in range(n)]).astype(np.float32)
            expect = rows.reshape(n, -1, 3) + np.asarray(g["verts"], np.float32)[None]
        assert len(expect) == n
        for i in range(n):
            assert (d / f"{i:06d}.obj").read_bytes() == _written(tmp_path, expect[i], g["faces"]), i
        writers = list(viewer._obj_writers.values())
        assert len(writers) == 1 and (writers[0].device_frames, writers[0].host_frames) == (n, 0)
    finally:
        viewer.clear_template()
