"""RGB frames on the GPU -> JPEG files: host side of the baseline-JPEG encoder in libsdfa_hip.so (csrc/jpeg.hip, C ABI in
include/sdfa_jpeg.h).  Every file is byte for byte what speech_anime.video.encode_jpeg (PIL) writes at the same quality; the
format contract is written down in the header and in DESIGN.md "GPU JPEG".

There is no CPU fallback, as with sdfa_amd.render: a library without the JPEG symbols fails at import."""
import ctypes as C

import torch

from ._lib import bind, lib, check, SdfaError
from ._packed import PackedReadback, ptr as _ptr, stream as _stream
from .render import CHUNK_FRAMES

ABI_VERSION = 1      # include/sdfa_jpeg.h SDFA_JPEG_ABI_VERSION this binding was written against
CHUNK_BYTES = 1 << 30  # workspace + output budget of one library call; large frames take fewer than CHUNK_FRAMES per call

_p, _i64 = C.c_void_p, C.c_int64
SYMBOLS = {
    "sdfa_jpeg_abi_version": (C.c_int, []),
    "sdfa_jpeg_create": (_p, [C.c_int, C.c_int, C.c_int, _p]),
    "sdfa_jpeg_destroy": (None, [_p]),
    "sdfa_jpeg_header": (_i64, [_p, _p, _i64]),
    "sdfa_jpeg_max_frame_bytes": (_i64, [_p]),
    "sdfa_jpeg_workspace_bytes": (_i64, [_p, _i64]),
    "sdfa_jpeg_encode": (C.c_int, [_p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _p]),
    "sdfa_jpeg_debug_coefs": (C.c_int, [_p, _p, _i64, _p, _p]),
}


bind(SYMBOLS, "sdfa_jpeg_abi_version", ABI_VERSION, "jpeg")


class PendingChunk(PackedReadback):
    """One encode call in flight: the file lengths are on their way to pinned host memory; result() waits for them, then
    reads back exactly the encoded bytes in one copy and splits them into files."""

    def result(self):
        return self.records()


class JpegEncoder:
    """Encodes (n, height, width, 3) uint8 cuda frames into JPEG files (PIL's bytes at `quality`), on the current stream,
    in chunks of at most CHUNK_FRAMES frames."""

    def __init__(self, width, height, quality=90, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("JpegEncoder needs a ROCm GPU: there is no CPU implementation")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.width, self.height, self.quality = int(width), int(height), int(quality)
        self._e = lib.sdfa_jpeg_create(self.width, self.height, self.quality, _stream())
        if not self._e:
            raise SdfaError(-1, lib.sdfa_last_error().decode())
        self.max_frame_bytes = int(check(lib.sdfa_jpeg_max_frame_bytes(self._e)))
        per_frame = self.max_frame_bytes + int(check(lib.sdfa_jpeg_workspace_bytes(self._e, 1)))
        self.chunk = max(1, min(CHUNK_FRAMES, CHUNK_BYTES // per_frame))
        self._ws = None

    def __del__(self):
        e, self._e = getattr(self, "_e", None), None
        if e:
            lib.sdfa_jpeg_destroy(e)

    @property
    def header(self):
        """SOI .. SOS of every file of this encoder (bytes)."""
        n = int(check(lib.sdfa_jpeg_header(self._e, None, 0)))
        buf = (C.c_uint8 * n)()
        check(lib.sdfa_jpeg_header(self._e, buf, n))
        return bytes(buf)

    def _frames(self, rgb):
        assert torch.is_tensor(rgb) and rgb.is_cuda, "JpegEncoder takes cuda frames: there is no CPU path"
        assert rgb.dtype == torch.uint8, rgb.dtype
        rgb = rgb.to(self.device).reshape(-1, self.height, self.width, 3).contiguous()
        return rgb

    def _workspace(self, n):
        need = int(check(lib.sdfa_jpeg_workspace_bytes(self._e, n)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def submit(self, rgb):
        """Enqueue one call of at most self.chunk frames; returns a PendingChunk.  The device output is kept alive by the
        PendingChunk, so several may be in flight (the workspace is reused in stream order)."""
        rgb = self._frames(rgb)
        n = rgb.shape[0]
        assert n <= self.chunk, (n, self.chunk)
        if n == 0:
            return PendingChunk(None, None, 0)
        out = torch.empty(n * self.max_frame_bytes, dtype=torch.uint8, device=self.device)
        meta = torch.empty(2 * n, dtype=torch.int64, device=self.device)          # offsets, then lengths
        ws = self._workspace(n)
        check(lib.sdfa_jpeg_encode(self._e, _ptr(rgb), n, _ptr(out), out.numel(), _ptr(meta), C.c_void_p(meta.data_ptr() + 8 * n),
                                   _ptr(ws), ws.numel(), _stream()))
        return PendingChunk(out, meta, n)

    def encode(self, rgb):
        """(n, H, W, 3) (or (H, W, 3)) uint8 cuda frames -> list of n JPEG files (bytes)."""
        rgb = self._frames(rgb)
        files = []
        for i0 in range(0, rgb.shape[0], self.chunk):
            files += self.submit(rgb[i0:i0 + self.chunk]).result()
        return files

    def coefficients(self, rgb):
        """The transform stage alone (tests): (n, MCUs, 6, 64) int16 cuda, quantised zigzag coefficients in coding order."""
        rgb = self._frames(rgb)
        n = rgb.shape[0]
        mcus = ((self.width + 15) // 16) * ((self.height + 15) // 16)
        out = torch.empty((n, mcus, 6, 64), dtype=torch.int16, device=self.device)
        for i0 in range(0, n, self.chunk):
            i1 = min(n, i0 + self.chunk)
            check(lib.sdfa_jpeg_debug_coefs(self._e, _ptr(rgb[i0:i1]), i1 - i0, _ptr(out[i0:i1]), _stream()))
        return out

