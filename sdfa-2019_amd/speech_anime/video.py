"""Evaluated animation -> video file: the part of speech_anime/viewer/video.py:199-290 (render_video) that evaluate()
uses for one source, without OpenCV or ffmpeg.

The reference writes XVID frames with cv2.VideoWriter, saves the sound next to them and muxes both into an .mp4 with
ffmpeg (video.py:286).  Neither an H.264 nor an MPEG-4 encoder exists in this image, so the video is an AVI 1.0 file written
here in pure Python: MJPEG frames (PIL, quality 90) and 16-bit mono PCM audio, one audio chunk interleaved after each video
frame, with an idx1 index.  Any MJPEG-capable player plays it.  The frames themselves come from the GPU rasterizer
(sdfa_amd.render); by default host threads encode them with PIL, overlapped with rendering and readback of the next chunk.
write_video(encoder="gpu") encodes them on the device instead (sdfa_amd.jpeg: the same bytes, only the JPEG files are read
back)."""
import io
import os
import struct
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

from .audio import pcm16, SOUND_SR

AVI1_LIMIT = 1 << 30          # RIFF size of an AVI 1.0 file (no OpenDML extension written here)
JPEG_QUALITY = 90


def video_frame_count(last_ts_ms, fps):
    """Number of frames render_video writes for a track ending at `last_ts_ms` (video.py:211-275, literally):
    ts = 0.0; while ts < max_ts: (one frame); ts += 1000.0 / fps -- the accumulated float64 sum, not i * 1000 / fps."""
    ts, delta, n = 0.0, 1000.0 / float(fps), 0
    while ts < last_ts_ms:
        n += 1
        ts += delta
    return n


def encode_jpeg(rgb, quality=JPEG_QUALITY):
    """(H, W, 3) uint8 -> JPEG bytes (PIL releases the GIL while it encodes)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def _chunk(fourcc, data):
    pad = b"\0" if len(data) & 1 else b""
    return fourcc + struct.pack("<I", len(data)) + data + pad


def _list(kind, body):
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


class AviWriter:
    """AVI 1.0: stream 0 = MJPG video (width x height at `fps`), stream 1 (if `audio` is given) = 16-bit mono PCM at
    `sample_rate`.  Frame k is followed by audio samples [round(k sr / fps), round((k + 1) sr / fps)); the last frame's chunk
    takes every remaining sample, so the audio chunks concatenate to the whole track.  `n_frames` is fixed up front.
    Writing past `max_bytes` (1 GiB, the AVI 1.0 RIFF limit) raises ValueError."""

    def __init__(self, path, width, height, fps, n_frames, audio=None, sample_rate=SOUND_SR, max_bytes=AVI1_LIMIT):
        self.path, self.width, self.height = path, int(width), int(height)
        self.fps, self.n_frames, self.sr = float(fps), int(n_frames), int(sample_rate)
        self.audio = None if audio is None else np.ascontiguousarray(audio, dtype="<i2").reshape(-1)
        self.max_bytes = int(max_bytes)
        self.frames_written = 0
        self._index = []                  # (fourcc, flags, offset from 'movi', size)
        self._max_chunk = 0
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self._fp = open(path, "wb")
        hdr = self._headers()
        self._fp.write(b"RIFF" + struct.pack("<I", 0) + b"AVI " + hdr)
        self._movi_at = self._fp.tell()               # position of the 'LIST' of movi
        self._fp.write(b"LIST" + struct.pack("<I", 0) + b"movi")
        self._size = self._fp.tell()

    def _audio_span(self, k):
        if self.audio is None:
            return 0, 0
        n = len(self.audio)
        lo = min(int(round(k * self.sr / self.fps)), n)
        hi = n if k == self.n_frames - 1 else min(int(round((k + 1) * self.sr / self.fps)), n)
        return lo, hi

    def _headers(self, max_chunk=0):
        rate = Fraction(self.fps).limit_denominator(1000000)
        us_per_frame = int(round(1e6 / self.fps))
        n_streams = 1 if self.audio is None else 2
        avih = struct.pack("<IIIIIIIIII4I", us_per_frame, 0, 0, 0x10 | 0x100, self.n_frames, 0, n_streams, max_chunk,
                           self.width, self.height, 0, 0, 0, 0)
        strh_v = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, rate.denominator, rate.numerator, 0,
                             self.n_frames, max_chunk, 0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf_v = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        body = _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))
        if self.audio is not None:
            strh_a = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 2, 2 * self.sr, 0, len(self.audio),
                                 0, 0xFFFFFFFF, 2, 0, 0, 0, 0)
            strf_a = struct.pack("<HHIIHH", 1, 1, self.sr, 2 * self.sr, 2, 16)
            body += _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a))
        return _list(b"hdrl", body)

    def _put(self, fourcc, data, flags):
        ck = _chunk(fourcc, data)
        if self._size + len(ck) + 16 * (len(self._index) + 3) + 8 > self.max_bytes:
            self._fp.close()
            os.remove(self.path)
            raise ValueError(f"{self.path}: the video would exceed {self.max_bytes} bytes, the AVI 1.0 limit this writer keeps to "
                             "(no OpenDML index); render a shorter clip or a smaller --grid_w / --grid_h")
        self._index.append((fourcc, flags, self._size - self._movi_at - 8, len(data)))
        self._fp.write(ck)
        self._size += len(ck)
        self._max_chunk = max(self._max_chunk, len(data))

    def write_jpeg(self, jpeg):
        """Append the next frame (JPEG bytes) and its audio chunk."""
        assert self.frames_written < self.n_frames, "more frames than announced"
        self._put(b"00dc", jpeg, 0x10)
        lo, hi = self._audio_span(self.frames_written)
        if hi > lo:
            self._put(b"01wb", self.audio[lo:hi].tobytes(), 0x10)
        self.frames_written += 1

    def close(self):
        assert self.frames_written == self.n_frames, f"{self.frames_written} of {self.n_frames} frames written"
        if self.n_frames == 0 and self.audio is not None and len(self.audio):
            self._put(b"01wb", self.audio.tobytes(), 0x10)
        movi_end = self._size
        idx = b"".join(struct.pack("<4sIII", *e) for e in self._index)
        self._fp.write(_chunk(b"idx1", idx))
        end = self._fp.tell()
        self._fp.seek(4)
        self._fp.write(struct.pack("<I", end - 8))
        self._fp.seek(12)
        self._fp.write(self._headers(self._max_chunk))         # same length: only the buffer sizes change
        self._fp.seek(self._movi_at + 4)
        self._fp.write(struct.pack("<I", movi_end - self._movi_at - 8))
        self._fp.close()


def read_avi(path):
    """Minimal RIFF reader (tests, tools): dict(avih=..., streams=[(fccType, fccHandler)], video=[jpeg bytes],
    audio=int16 array, index=[(fourcc, flags, offset, size)])."""
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    out = dict(streams=[], video=[], audio=[], index=[])

    def walk(lo, hi):
        while lo + 8 <= hi:
            fcc, size = data[lo:lo + 4], struct.unpack("<I", data[lo + 4:lo + 8])[0]
            body = data[lo + 8:lo + 8 + size]
            if fcc == b"LIST":
                walk(lo + 12, lo + 8 + size)
            elif fcc == b"avih":
                v = struct.unpack("<IIIIIIIIII", body[:40])
                out["avih"] = dict(us_per_frame=v[0], flags=v[3], total_frames=v[4], streams=v[6], width=v[8], height=v[9])
            elif fcc == b"strh":
                out["streams"].append((body[:4], body[4:8]))
            elif fcc == b"00dc":
                out["video"].append(body)
            elif fcc == b"01wb":
                out["audio"].append(np.frombuffer(body, "<i2"))
            elif fcc == b"idx1":
                out["index"] = [struct.unpack("<4sIII", body[i:i + 16]) for i in range(0, len(body), 16)]
            lo += 8 + size + (size & 1)
    walk(12, 8 + struct.unpack("<I", data[4:8])[0])
    out["audio"] = np.concatenate(out["audio"]) if out["audio"] else np.zeros(0, np.int16)
    return out


JPEG_ENCODERS = ("pil", "gpu")


def write_video(path, n_frames, render_chunk, width, height, fps, sound=None, sample_rate=SOUND_SR, chunk=32, workers=None,
                encoder="pil"):
    """Render, encode and write `n_frames` frames.  `render_chunk(i0, i1)` returns frames [i0, i1) as a
    (i1 - i0, height, width, 3) uint8 cuda tensor.  `sound`: float signal at `sample_rate` (converted like audio.wav).

    encoder="pil": chunks are copied into two pinned host buffers on a side stream while the JPEG encoder threads work on
    the previous chunk.  encoder="gpu": each chunk is encoded on the device (sdfa_amd.jpeg, the same bytes) and only the
    JPEG files are read back; the host writes chunk k - 1 while the device renders and encodes chunk k."""
    if encoder not in JPEG_ENCODERS:
        raise ValueError(f"encoder must be one of {JPEG_ENCODERS}, not {encoder!r}")
    audio = None if sound is None else pcm16(sound)
    writer = AviWriter(path, width, height, fps, n_frames, audio, sample_rate)
    try:
        if encoder == "gpu":
            _encode_gpu(writer, n_frames, render_chunk, width, height, chunk)
        else:
            _encode_pil(writer, n_frames, render_chunk, width, height, chunk, workers)
        writer.close()
    except BaseException:
        if not writer._fp.closed:
            writer._fp.close()
        raise
    return writer


def _encode_gpu(writer, n_frames, render_chunk, width, height, chunk):
    from sdfa_amd.jpeg import JpegEncoder
    enc = JpegEncoder(width, height, JPEG_QUALITY)
    step = max(1, min(chunk, enc.chunk))
    done = []                                      # JPEG files of the previous chunk
    for i0 in range(0, n_frames, step):
        pending = enc.submit(render_chunk(i0, min(n_frames, i0 + step)))
        for jpeg in done:
            writer.write_jpeg(jpeg)
        done = pending.result()
    for jpeg in done:
        writer.write_jpeg(jpeg)


def _encode_pil(writer, n_frames, render_chunk, width, height, chunk, workers):
    import torch
    dev = torch.cuda.current_device()
    bufs = [torch.empty((chunk, height, width, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    copy_stream = torch.cuda.Stream(device=dev)
    pending = []               # (futures of one chunk)
    with ThreadPoolExecutor(max_workers=workers or min(16, os.cpu_count() or 1)) as pool:
        def drain(keep):
            while len(pending) > keep:
                for fut in pending.pop(0):
                    writer.write_jpeg(fut.result())
        for ci, i0 in enumerate(range(0, n_frames, chunk)):
            i1 = min(n_frames, i0 + chunk)
            drain(1)                                  # the buffer this chunk reuses is free once chunk ci-2 is written
            rgb = render_chunk(i0, i1)
            buf = bufs[ci % 2]
            copy_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(copy_stream):
                buf[:i1 - i0].copy_(rgb, non_blocking=True)
                rgb.record_stream(copy_stream)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            ev.synchronize()
            host = buf.numpy()
            pending.append([pool.submit(encode_jpeg, host[j]) for j in range(i1 - i0)])
        drain(0)
