"""CPU checks of the GPU OBJ formatter's contract: the integer recipe of include/sdfa_obj.h (tests/obj_oracle.py) prints
exactly what "{:.6f}".format prints for a float32 over the edge list, the exact ties, the whole domain and N(0, 0.1); the host
face formatter writes write_obj's face lines; the ABI of include/sdfa_obj.h is bound and exported; the kernels use no scratch."""
import os
import re

import numpy as np
import pytest

import obj_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _python_text(x):
    return ["{:.6f}".format(v) for v in np.asarray(x, np.float32).reshape(-1)]


@pytest.mark.parametrize("data", ["edges", "ties", "patterns", "normal"])
def test_oracle_equals_python_format(data):
    x = {"edges": O.edge_values, "ties": O.tie_values, "patterns": lambda: O.domain_patterns(200000, 11),
         "normal": lambda: O.normal_values(200000, 12)}[data]()
    assert O.in_domain(x).all()
    got, want = O.numbers(x), _python_text(x)
    wrong = [(float(v), g, w) for v, g, w in zip(x, got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])


def test_oracle_known_texts():
    f = lambda v: O.numbers(np.float32(v))[0]
    assert f(1 / 128) == "0.007812" and f(3 / 128) == "0.023438"               # exact ties go to the even digit
    assert f(-0.0) == "-0.000000" and f(-1e-7) == "-0.000000" and f(1e-45) == "0.000000"
    assert f(0.9999995) == "{:.6f}".format(np.float32(0.9999995))
    assert f(-2147483520.0) == "-2147483520.000000"
    line = ("v" + " -2147483520.000000" * 3 + "\n").encode()
    assert len(line) == O.MAX_LINE_BYTES == 59
    assert O.vertex_block(np.full((2, 3), -2147483520.0, np.float32)) == line * 2
    assert not O.in_domain(np.array([np.nan, np.inf, -np.inf, 2.0 ** 31], np.float32)).any()


def test_oracle_blocks_equal_write_obj(tmp_path):
    from speech_anime.viewer import write_obj
    verts = np.concatenate([O.edge_values(), O.normal_values(300, 5)])
    verts = verts[:len(verts) // 3 * 3].reshape(-1, 3)
    faces = np.array([[0, 1, 2], [8, 9, 10], [98, 99, 100]], np.uint32)
    write_obj(str(tmp_path / "a.obj"), verts, faces)
    assert (tmp_path / "a.obj").read_bytes() == O.vertex_block(verts) + O.face_block(faces)


def test_format_faces_equals_write_obj(tmp_path):
    from sdfa_amd import obj
    from speech_anime.viewer import write_obj
    idx = [0, 7, 8, 9, 10, 11, 97, 98, 99, 100, 101, 997, 998, 999, 1000, 1001, 9997, 9998, 9999, 10000, 10001, 123456]
    faces = np.array([[a, b, c] for a, b, c in zip(idx, idx[1:] + idx[:1], idx[2:] + idx[:2])], np.uint32)
    n_verts = max(idx) + 1
    write_obj(str(tmp_path / "f.obj"), np.zeros((0, 3), np.float32), faces)
    want = (tmp_path / "f.obj").read_bytes()
    assert want.startswith(b"f 1 8 9\n") and b" 10000 " in want
    assert obj.format_faces(faces, n_verts) == want == O.face_block(faces)
    assert obj.format_faces(faces.astype(np.int64), n_verts) == want
    assert obj.format_faces(np.zeros((0, 3), np.uint32), 5) == b""


def test_format_faces_refuses_an_index_past_the_vertices():
    from sdfa_amd import obj, _lib
    faces = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)
    assert obj.format_faces(faces, 5) == b"f 1 2 3\nf 3 4 5\n"
    with pytest.raises(_lib.SdfaError, match="vertex 4") as e:
        obj.format_faces(faces, 4)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(ValueError):
        obj.format_faces(np.array([[0, -1, 2]]), 5)


def test_format_faces_length_and_truncated_copy():
    import ctypes as C
    from sdfa_amd import obj, _lib
    faces = np.array([[0, 9, 99]], np.uint32)
    want = b"f 1 10 100\n"
    assert _lib.lib.sdfa_obj_format_faces(faces.ctypes.data, 1, 100, None, 0) == len(want)
    buf = (C.c_uint8 * 16)(*([0xAA] * 16))
    assert _lib.lib.sdfa_obj_format_faces(faces.ctypes.data, 1, 100, buf, 4) == len(want)
    assert bytes(buf) == want[:4] + b"\xaa" * 12


def test_obj_header_symbols_bound_and_exported():
    from sdfa_amd import obj, jpeg, render, _lib
    hdr = open(os.path.join(ROOT, "include", "sdfa_obj.h")).read()
    assert re.search(r"#define SDFA_OBJ_ABI_VERSION 1\b", hdr)
    assert int(re.search(r"#define SDFA_OBJ_MAX_LINE_BYTES\s+(\d+)", hdr).group(1)) == obj.MAX_LINE_BYTES == O.MAX_LINE_BYTES == 59
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    declared = set(re.findall(r"\b(sdfa_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(obj.SYMBOLS), declared ^ set(obj.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.sdfa_obj_abi_version() == obj.ABI_VERSION == 1
    for other in (_lib, jpeg, render):
        assert not declared & set(other.SYMBOLS), "obj symbols belong to their own header"
    assert _lib.lib.sdfa_abi_version() == _lib.ABI_VERSION == 5              # the core ABI did not move


def test_max_frame_bytes_and_argument_checks():
    from sdfa_amd import obj, _lib
    lib = _lib.lib
    for v in (0, 1, 255, 256, 257, 5023, 1 << 20):
        assert lib.sdfa_obj_max_frame_bytes(v) == 59 * v
    assert lib.sdfa_obj_workspace_bytes(5023, 64) > 0
    assert lib.sdfa_obj_workspace_bytes(5023, 0) == 0
    assert lib.sdfa_obj_workspace_bytes(0, 1) == _lib.EINVAL
    assert lib.sdfa_obj_workspace_bytes(1, -1) == _lib.EINVAL
    # n == 0 is a no-op, whatever the pointers; bad arguments are refused on the host, before any launch
    assert lib.sdfa_obj_format_verts(None, 0, 5023, None, 0, None, None, None, None, 0, None) == 0
    assert lib.sdfa_obj_format_verts(None, 1, 5023, None, 0, None, None, None, None, 0, None) == _lib.EINVAL
    assert b"null pointer" in lib.sdfa_last_error()
    p = 1 << 12                                                               # never dereferenced: the checks come first
    assert lib.sdfa_obj_format_verts(p, 2, 10, p, 2 * 590 - 1, p, p, p, p, 1 << 20, None) == _lib.EINVAL
    assert b"output of 1179 bytes" in lib.sdfa_last_error()
    need = lib.sdfa_obj_workspace_bytes(10, 2)
    assert lib.sdfa_obj_format_verts(p, 2, 10, p, 2 * 590, p, p, p, p, need - 1, None) == _lib.EINVAL
    assert b"workspace of" in lib.sdfa_last_error()
    assert lib.sdfa_obj_format_verts(p, 2, 10, p, 2 * 590, p, p, p, p + 8, need, None) == _lib.EINVAL
    assert b"aligned" in lib.sdfa_last_error()


def test_obj_kernels_use_no_scratch():
    from test_scratch_guard_cpu import _kernel_metadata
    meta = _kernel_metadata()
    kernels = {k: v for k, v in meta.items() if k.startswith("obj_")}
    assert set(kernels) == {"obj_length_kernel", "obj_frame_kernel", "obj_offsets_kernel", "obj_format_kernel"}, sorted(kernels)
    for name, m in kernels.items():
        got = {x: int(m[x]) for x in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        assert not any(got.values()), (name, got)
    assert int(kernels["obj_format_kernel"]["group_segment_fixed_size"]) <= 16 * 1024      # a tile's text: 256 * 59 + 16 bytes
