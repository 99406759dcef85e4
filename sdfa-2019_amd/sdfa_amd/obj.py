"""Vertices on the GPU -> Wavefront OBJ files: host side of the OBJ text formatter in libsdfa_hip.so (csrc/obj.hip, C ABI in
include/sdfa_obj.h).  Every file is byte for byte what speech_anime.viewer.write_obj writes for the same vertices and
faces; the format contract is written down in the header and in DESIGN.md "OBJ text".

The vertex block ("v X Y Z\\n" per vertex) of every frame is formatted on the device; the face block is the same in every
frame of a template and is formatted once, on the host.  A frame with a value outside the kernel's domain (not finite, or
|x| >= 2^31) comes back flagged and is written by write_obj itself: the data decides, there is no option.  A library
without the OBJ symbols fails at import."""
import ctypes as C

import numpy as np
import torch

from ._lib import bind, lib, check
from ._packed import PackedReadback, ptr as _ptr, stream as _stream
from .jpeg import CHUNK_BYTES
from .render import CHUNK_FRAMES

ABI_VERSION = 1      # include/sdfa_obj.h SDFA_OBJ_ABI_VERSION this binding was written against
MAX_LINE_BYTES = 59  # SDFA_OBJ_MAX_LINE_BYTES

_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_obj_abi_version": (C.c_int, []),
    "sdfa_obj_max_frame_bytes": (_i64, [_i64]),
    "sdfa_obj_workspace_bytes": (_i64, [_i64, _i64]),
    "sdfa_obj_format_verts": (C.c_int, [_p, _i64, _i64, _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "sdfa_obj_format_faces": (_i64, [_p, _i64, _i64, _p, _i64]),
}


bind(SYMBOLS, "sdfa_obj_abi_version", ABI_VERSION, "obj")


def format_faces(faces, n_verts):
    """(T, 3) 0-based triangles -> the face block of their .obj file, "f a b c\\n" with 1-based indices (bytes).  An index
    that is negative or >= n_verts is refused."""
    f = np.asarray(faces)
    if f.size and int(f.min()) < 0:
        raise ValueError("format_faces: negative vertex index")
    f = np.ascontiguousarray(f.reshape(-1, 3), dtype=np.uint32)
    n = int(check(lib.sdfa_obj_format_faces(f.ctypes.data, len(f), int(n_verts), None, 0)))
    buf = (C.c_uint8 * n)()
    check(lib.sdfa_obj_format_faces(f.ctypes.data, len(f), int(n_verts), buf, n))
    return bytes(buf)


class PendingChunk(PackedReadback):
    """One format call in flight: offsets, lengths and flags are on their way to pinned host memory; result() waits for
    them, then reads back exactly the formatted bytes in one copy."""

    def result(self):
        """(blocks, flags): the n vertex blocks (bytes) and n bools; the block of a flagged frame is not to be used."""
        if self.n == 0:
            return [], []
        flags = self.meta()[2 * self.n:].view(torch.int32)[:self.n].numpy() != 0
        return self.records(), flags.tolist()


class ObjFormatter:
    """Formats (n, n_verts, 3) float32 cuda vertices into the vertex blocks of their .obj files, on the current stream, in
    chunks of at most `chunk` frames (CHUNK_FRAMES, fewer when a chunk's output and workspace would pass CHUNK_BYTES)."""

    def __init__(self, n_verts, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("ObjFormatter needs a ROCm GPU: there is no CPU implementation")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_verts = int(n_verts)
        self.max_frame_bytes = int(check(lib.sdfa_obj_max_frame_bytes(self.n_verts)))
        per_frame = self.max_frame_bytes + int(check(lib.sdfa_obj_workspace_bytes(self.n_verts, 1)))
        self.chunk = max(1, min(CHUNK_FRAMES, CHUNK_BYTES // per_frame))
        self._ws = None

    def frames(self, verts):
        assert torch.is_tensor(verts) and verts.is_cuda, "ObjFormatter takes cuda vertices: there is no CPU path"
        assert verts.dtype == torch.float32, verts.dtype
        return verts.to(self.device).reshape(-1, self.n_verts, 3).contiguous()

    def _workspace(self, n):
        need = int(check(lib.sdfa_obj_workspace_bytes(self.n_verts, n)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def submit(self, verts):
        """Enqueue one call of at most self.chunk frames; returns a PendingChunk.  The device output is kept alive by the
        PendingChunk, so several may be in flight (the workspace is reused in stream order)."""
        verts = self.frames(verts)
        n = verts.shape[0]
        assert n <= self.chunk, (n, self.chunk)
        if n == 0:
            return PendingChunk(None, None, 0)
        with torch.cuda.device(self.device):
            out = torch.empty(n * self.max_frame_bytes, dtype=torch.uint8, device=self.device)
            meta = torch.empty(2 * n + (n + 1) // 2, dtype=torch.int64, device=self.device)     # offsets, lengths, int32 flags
            ws = self._workspace(n)
            check(lib.sdfa_obj_format_verts(_ptr(verts), n, self.n_verts, _ptr(out), out.numel(), _ptr(meta),
                                            C.c_void_p(meta.data_ptr() + 8 * n), C.c_void_p(meta.data_ptr() + 16 * n),
                                            _ptr(ws), ws.numel(), _stream()))
            return PendingChunk(out, meta, n)

    def format(self, verts):
        """(n, V, 3) (or (V, 3)) float32 cuda vertices -> (blocks, flags) of all n frames."""
        verts = self.frames(verts)
        blocks, flags = [], []
        for i0 in range(0, verts.shape[0], self.chunk):
            b, f = self.submit(verts[i0:i0 + self.chunk]).result()
            blocks += b
            flags += f
        return blocks, flags


class ObjWriter:
    """Writes the .obj files of one template's frames: device-formatted vertex block + the cached face block."""

    def __init__(self, faces, n_verts, device=None):
        self.faces = np.asarray(faces).reshape(-1, 3)
        self.face_block = format_faces(self.faces, n_verts)
        self.formatter = ObjFormatter(n_verts, device)
        self.device_frames = 0       # frames whose vertex block the device formatted
        self.host_frames = 0         # flagged frames, written by speech_anime.viewer.write_obj

    @property
    def chunk(self):
        return self.formatter.chunk

    @chunk.setter
    def chunk(self, n):
        self.formatter.chunk = int(n)

    def write(self, paths, verts):
        """paths[i] <- frame i of the (n, V, 3) float32 cuda vertices.  One chunk is in flight while the files of the chunk
        before it are written."""
        verts = self.formatter.frames(verts)
        assert len(paths) == verts.shape[0], (len(paths), tuple(verts.shape))
        step = self.chunk
        starts = list(range(0, len(paths), step))
        pending = self.formatter.submit(verts[:step]) if starts else None
        for i0 in starts:
            blocks, flags = pending.result()
            if i0 + step < len(paths):
                pending = self.formatter.submit(verts[i0 + step:i0 + 2 * step])
            for i, (block, flagged) in enumerate(zip(blocks, flags), i0):
                if flagged:
                    from speech_anime.viewer import write_obj
                    write_obj(paths[i], verts[i].cpu().numpy(), self.faces)
                    self.host_frames += 1
                else:
                    with open(paths[i], "wb") as fp:
                        fp.write(block)
                        fp.write(self.face_block)
                    self.device_frames += 1
