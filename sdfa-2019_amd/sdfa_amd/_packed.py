"""What the bindings of the library's variable-length outputs share (sdfa_amd.jpeg files, sdfa_amd.obj vertex blocks): one
call packs n records back to back into a device buffer and leaves their int64 offsets and lengths next to each other on
the device; the host reads the lengths first and then exactly the bytes that were written."""
import ctypes as C

import torch


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


class PackedReadback:
    """One call in flight.  `meta` is the call's int64 device tensor: n offsets, n lengths, then whatever else the caller
    keeps there.  Its copy to pinned host memory is enqueued here, on the current stream, with an event behind it; the
    device buffers stay alive with this object, so several calls may be in flight."""

    def __init__(self, out, meta, n):
        self._out, self._meta_dev, self.n = out, meta, n
        if n:
            self._meta_host = torch.empty(meta.shape, dtype=meta.dtype, pin_memory=True)
            self._meta_host.copy_(meta, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()

    def meta(self):
        """The host copy of `meta` (waits for it)."""
        self._event.synchronize()
        return self._meta_host

    def records(self):
        """Waits for the lengths, reads back exactly the packed bytes in one copy and splits them: a list of n bytes."""
        if self.n == 0:
            return []
        meta = self.meta().numpy()
        offs, lens = meta[:self.n], meta[self.n:2 * self.n]
        total = int(offs[-1] + lens[-1])
        data = self._out[:total].cpu().numpy().tobytes()
        return [data[o:o + ln] for o, ln in zip(offs.tolist(), lens.tolist())]
