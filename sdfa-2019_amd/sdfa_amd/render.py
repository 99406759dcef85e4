"""Vertices of animation frames on the GPU -> RGB images: host side of the rasterizer in libsdfa_hip.so (csrc/render.hip,
C ABI in include/sdfa_render.h).  The reference renders each frame with pyrender (speech_anime/viewer/render_py.py); the
rendering contract here is the one written down in the header and in DESIGN.md "Rendering".

There is no CPU fallback, as with sdfa_amd.mesh: a library without the render symbols fails at import."""
import ctypes as C

import numpy as np
import torch

from ._lib import bind, lib, check, SdfaError

ABI_VERSION = 1      # include/sdfa_render.h SDFA_RENDER_ABI_VERSION this binding was written against
NORMALS = {"template": 0, "frame": 1}
CHUNK_FRAMES = 64    # frames per library call: bounds the workspace (~0.3 MB per frame for the FLAME mesh)


class Params(C.Structure):
    """sdfa_render_params."""
    _fields_ = [("cam_pose", C.c_float * 16), ("yfov", C.c_float), ("znear", C.c_float), ("ambient", C.c_float),
                ("dir_intensity", C.c_float), ("point_intensity", C.c_float), ("albedo", C.c_float * 3),
                ("background", C.c_float * 3)]


_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_render_abi_version": (C.c_int, []),
    "sdfa_render_default_params": (C.c_int, [C.POINTER(Params)]),
    "sdfa_render_create": (_p, [_p, _i64, _p, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), _p]),
    "sdfa_render_destroy": (None, [_p]),
    "sdfa_render_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_render_frames": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, _p]),
    "sdfa_render_debug_screen": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
}


bind(SYMBOLS, "sdfa_render_abi_version", ABI_VERSION, "render")


def default_params():
    p = Params()
    check(lib.sdfa_render_default_params(C.byref(p)))
    return p


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Renderer:
    """Renders (n, V, 3) fp32 cuda vertices of one topology into (n, H, W, 3) uint8 cuda images (row 0 at the top).

    template_verts / faces: the template mesh (host arrays); its extent fixes the scale 0.15 / max|v| and its vertex normals
    shade every frame with normals="template" (the reference's behaviour); normals="frame" recomputes them per frame.
    image_size = (width, height) as render_mesh takes it; samples 1 or 4; params: a Params (None = the reference's rig)."""

    def __init__(self, template_verts, faces, image_size=(512, 512), samples=4, normals="template", params=None, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("Renderer needs a ROCm GPU: there is no CPU implementation")
        if normals not in NORMALS:
            raise ValueError(f"normals must be one of {sorted(NORMALS)}, not {normals!r}")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        v = np.ascontiguousarray(np.asarray(template_verts, np.float32).reshape(-1, 3))
        f = np.ascontiguousarray(np.asarray(faces, np.uint32).reshape(-1, 3))
        self.n_verts, self.n_tris = len(v), len(f)
        self.width, self.height = int(image_size[0]), int(image_size[1])
        self.samples, self.normals = int(samples), normals
        self.params = default_params() if params is None else params
        self._r = lib.sdfa_render_create(v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p), len(f),
                                         self.width, self.height, self.samples, NORMALS[normals], C.byref(self.params), _stream())
        if not self._r:
            raise SdfaError(-1, lib.sdfa_last_error().decode())
        self._ws = None

    def __del__(self):
        r, self._r = getattr(self, "_r", None), None
        if r:
            lib.sdfa_render_destroy(r)

    def _workspace(self, n):
        need = int(check(lib.sdfa_render_workspace_bytes(self._r, n)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _verts(self, verts):
        assert torch.is_tensor(verts) and verts.is_cuda, "Renderer.render takes cuda vertices: there is no CPU path"
        v = verts.to(device=self.device, dtype=torch.float32).reshape(-1, self.n_verts, 3).contiguous()
        return v

    def render(self, verts, out=None, want_ids=False):
        """(n, V, 3) (or (V, 3)) fp32 cuda vertices -> (n, H, W, 3) uint8 cuda images [, (n, H, W) int32 triangle ids of each
        pixel's first sample, -1 for background].  Runs in chunks of CHUNK_FRAMES frames on the current stream."""
        v = self._verts(verts)
        n = v.shape[0]
        shape = (n, self.height, self.width)
        if out is None:
            out = torch.empty(shape + (3,), dtype=torch.uint8, device=self.device)
        assert out.shape == shape + (3,) and out.dtype == torch.uint8 and out.is_contiguous()
        ids = torch.empty(shape, dtype=torch.int32, device=self.device) if want_ids else None
        for i0 in range(0, n, CHUNK_FRAMES):
            i1 = min(n, i0 + CHUNK_FRAMES)
            ws = self._workspace(i1 - i0)
            check(lib.sdfa_render_frames(self._r, _ptr(v[i0:i1]), i1 - i0, _ptr(out[i0:i1]),
                                         _ptr(ids[i0:i1]) if want_ids else None, _ptr(ws), ws.numel(), _stream()))
        return (out, ids) if want_ids else out

    def screen(self, verts):
        """The vertex stage alone (tests): (n, V, 4) int32 = x, y in 1/256 pixel, bits of fp32 1/w, valid."""
        v = self._verts(verts)
        n = v.shape[0]
        out = torch.empty((n, self.n_verts, 4), dtype=torch.int32, device=self.device)
        for i0 in range(0, n, CHUNK_FRAMES):
            i1 = min(n, i0 + CHUNK_FRAMES)
            ws = self._workspace(i1 - i0)
            check(lib.sdfa_render_debug_screen(self._r, _ptr(v[i0:i1]), i1 - i0, _ptr(out[i0:i1]), _ptr(ws), ws.numel(), _stream()))
        return out
