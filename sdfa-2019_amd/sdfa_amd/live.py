"""Live streaming inference: many audio streams that arrive in pieces, stepped together on one GPU.  Host side of the
C ABI in include/sdfa_stream.h (csrc/frontend.hip: ring append and the spectral-stream front end over ring views).

The contract: every frame a stream emits is bit-identical to the same frame of the offline call on the
whole signal (`generate_animation`, `Engine.mel_frontend` + `forward_host`), with the same timestamp.  A frame is emitted as
soon as its window [s_k, s_k + sliding) and one sample more have arrived (never while n - 1 < sliding: the short-clip assert can
still fire then); `close` emits the tail frames past the end of the audio, sdfa_frame_index(n) frames in all.

A step is one host -> device copy (every stream's new samples, the segment table, the frame table and the speaker ids), one
ring-append launch, the front end (share_prev + the stream kernel + its repair pass), the encoder and the regressor -- whatever
the number of streams.

Capture-rate streams (`open(..., input_rate=, gain=)`): the samples go to an input ring, and each step converts the outputs that have
become final (include/sdfa_stream.h "Capture-rate streams") into the stream's model ring with the offline resampler's arithmetic, a
float32 gain and the +-0.999 clamp -- one more ring append and one resample launch per step, whatever the number of streams and
rates.  Such a stream emits the frames of generate_animation(clip(resample(x, input_rate, sr) * gain, -0.999, 0.999)), bit for bit.
The session does not normalise RMS (a whole-clip statistic: `speech_anime.audio.rms_gain` gives the gain of a known clip)."""
import ctypes as C

import numpy as np
import torch

from ._lib import bind, lib, check
from .engine import FEAT_SHAPE, FPS, TS_DELTA_MS, frame_geometry

ABI_VERSION = 1      # include/sdfa_stream.h SDFA_STREAM_ABI_VERSION this binding was written against
MAX_SAMPLES = 0x1fffffff
RING_MIRROR = 2048   # include/sdfa_stream.h SDFA_STREAM_RING_MIRROR
MAX_RATES = 8        # include/sdfa_stream.h SDFA_STREAM_MAX_RATES
T_OPEN = (1 << 63) - 1      # t_zero of a resample segment while its stream is open

_p, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
SYMBOLS = {
    "sdfa_stream_abi_version": (C.c_int, []),
    "sdfa_stream_frame_positions": (_i64, [_i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p]),
    "sdfa_stream_final_frames": (_i64, [_i64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sdfa_stream_ring_append": (C.c_int, [_p, C.c_int, _i32, _p, _i32, _p, _i64, _p]),
    "sdfa_mel_frontend_ring": (C.c_int, [_p, C.c_int, _i32, _p, _p, _i32, _p, _p, _i64, C.c_int, _p, _p, _i64, _p]),
    "sdfa_stream_resample_final": (_i64, [_i64, C.c_int, C.c_int]),
    "sdfa_stream_resample_register": (_i64, [_i64, C.c_int, C.c_int, _p, _p]),
    "sdfa_stream_resample_close": (_i64, [_i64, C.c_int, C.c_int, _p]),
    "sdfa_stream_resample_wing": (_i64, [C.c_int, C.c_int]),
    "sdfa_stream_resample": (C.c_int, [_p, C.c_int, _i32, _p, C.c_int, _i32, _p, _i32, _i64, _p, _i64, _p, _i32, C.c_int, _p]),
}


bind(SYMBOLS, "sdfa_stream_abi_version", ABI_VERSION, "stream")


def frame_positions(k0, count, sr, fps=FPS, ts_delta=TS_DELTA_MS):
    """(starts int64[count], tslist int32[count]) of frames k0 .. k0 + count - 1: bit-equal to `frame_index`'s entries."""
    win, hop, _ = frame_geometry(sr)
    starts = np.empty(count, np.int64)
    ts = np.empty(count, np.int32)
    if count:
        check(lib.sdfa_stream_frame_positions(int(k0), int(count), int(sr), int(fps), win, hop, int(ts_delta),
                                              starts.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p)))
    return starts, ts


def final_frames(n_samples, sr, fps=FPS):
    """Frames a stream that has received n_samples samples has made final: #{k : e_k < n}, 0 while n - 1 < sliding."""
    win, hop, _ = frame_geometry(sr)
    return int(check(lib.sdfa_stream_final_frames(int(n_samples), int(sr), int(fps), win, hop)))


def close_frames(n_samples, sr, fps=FPS):
    """Frames of a stream that ended after n_samples samples: sdfa_frame_index's count (raises the short-clip
    AssertionError, SDFA_ESHORTCLIP, for a stream shorter than one window)."""
    win, hop, _ = frame_geometry(sr)
    return int(check(lib.sdfa_frame_index(int(n_samples), int(sr), int(fps), win, hop, TS_DELTA_MS, None, None, 0)))


def resample_final(n_in, input_rate, sr):
    """Model-rate samples a stream at `input_rate` has made final after n_in input samples (include/sdfa_stream.h)."""
    return int(check(lib.sdfa_stream_resample_final(int(n_in), int(input_rate), int(sr))))


def resample_register(state, count, input_rate, sr):
    """(time registers float64[count] of `count` consecutive outputs, the carried register after them); `state` is the register of the
    first (0.0 for output 0).  The sequential accumulation of the offline call, however the calls are cut."""
    st = C.c_double(float(state))
    out = np.empty(int(count), np.float64)
    check(lib.sdfa_stream_resample_register(int(count), int(input_rate), int(sr), C.byref(st), out.ctypes.data_as(C.c_void_p)))
    return out, st.value


def resample_close(n_in, input_rate, sr):
    """(n_out, n_res) of a stream that ended after n_in input samples: its model-rate length and the outputs that are filtered
    (zeros behind them).  Raises what the offline `resample` raises ("too small to resample")."""
    n_res = _i64(0)
    n_out = int(check(lib.sdfa_stream_resample_close(int(n_in), int(input_rate), int(sr), C.byref(n_res))))
    return n_out, int(n_res.value)


def resample_wing(input_rate, sr):
    """nwin / step of the rate pair: the reach of one filter wing in input samples (0 for equal rates)."""
    return int(check(lib.sdfa_stream_resample_wing(int(input_rate), int(sr))))


def input_ring_bits(input_rate, sr, budget):
    """r_in with 2^r_in >= left wing + right wing + push budget (in input samples: `budget` model-rate samples' worth of time) + 1."""
    wing = resample_wing(input_rate, sr) + 1
    budget_in = -(-int(budget) * int(input_rate) // int(sr))
    return max(int(np.ceil(np.log2(2 * wing + budget_in + 1))), 1)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class _Stream:
    __slots__ = ("sid", "ring", "speaker", "pad", "n_dev", "n_total", "pending", "emitted", "end", "closing", "out_ts", "out_rows",
                 "rate", "gain", "wing", "in_dev", "in_total", "treg", "n_res")

    def __init__(self, sid, ring, speaker, pad, rate=None, gain=1.0):
        self.sid, self.ring, self.speaker, self.pad = sid, ring, speaker, pad
        self.rate, self.gain = rate, gain      # capture-rate stream: its input rate and gain (rate None: samples at the model rate)
        self.wing = 0               # reach of the left wing in input samples (the sample at n included)
        self.in_dev = 0             # input samples in the input ring (ring `ring` of the input ring array)
        self.in_total = 0           # ... plus input samples pushed and not yet uploaded
        self.treg = 0.0             # time register of output n_dev, the first not yet resampled
        self.n_res = T_OPEN         # once closed: outputs from here on are zeros
        self.n_dev = 0              # samples in the ring (capture-rate: outputs resampled so far)
        self.n_total = 0            # ... plus samples pushed and not yet uploaded (capture-rate: outputs final, or all once closed)
        self.pending = []           # host chunks not yet uploaded
        self.emitted = 0            # frames computed so far
        self.end = None             # frame count once closed
        self.closing = False
        self.out_ts, self.out_rows = [], []      # output of steps run inside push(), handed out by the next step()


class LiveSession:
    """Live streams over one Engine, stepped together on one CUDA stream with the session's own workspaces.

      engine            sdfa_amd.engine.Engine (its weights and precision mode)
      max_streams       rings on the device (one per open stream)
      sample_rate       the model rate of every stream (8000 or 16000)
      outputs           "rows" (the model's output rows) or "coef" (the PCA coefficients, 265 / 59 per frame;
                        `Engine.expand_coef` turns them into the bit-identical rows)
      host_copy         also return a pinned host copy of each step's output (the step then waits for it)
      push_budget       samples a stream may receive between two steps without forcing one (default 1 s)
      max_ensembling_ms the largest `ensembling_ms` an `open` may ask for
      max_step_frames   main frames per launch group (default: the engine's max_frames, halved when a stream ensembles)
      max_input_rate    the highest `input_rate` an `open` may ask for (sizes the input rings)

    Ring size R = 2^r >= sliding + max ensembling pad + push budget + 1.  A push that would overwrite samples that a frame not
    yet computed still needs runs a step first and keeps its output for the next `step()`, so any chunking works.  Input ring size
    R_in = 2^r_in >= both filter wings + the push budget in input samples + 1 at max_input_rate (`input_ring_bits`); the input rings
    are made by the first step that has a capture-rate stream."""

    def __init__(self, engine, max_streams, sample_rate=16000, outputs="rows", host_copy=False, push_budget=None,
                 max_ensembling_ms=20, max_step_frames=None, max_input_rate=48000):
        if outputs not in ("rows", "coef"):
            raise ValueError(f"outputs must be 'rows' or 'coef', not {outputs!r}")
        self.eng = engine
        self.device = engine.device
        self.sr = int(sample_rate)
        self.win, self.hop, self.sliding = frame_geometry(self.sr)
        self.outputs, self.host_copy = outputs, bool(host_copy)
        self.max_pad = int(max_ensembling_ms) * self.sr // 1000
        budget = int(push_budget) if push_budget else self.sr
        self.r = max(int(np.ceil(np.log2(self.sliding + self.max_pad + budget + 1))), 1)
        if self.r > 28:
            raise ValueError("ring of more than 2^28 samples: lower push_budget")
        self.R = 1 << self.r
        self.max_input_rate = int(max_input_rate)
        self.r_in = input_ring_bits(self.max_input_rate, self.sr, budget)
        if self.r_in > 28:
            raise ValueError("input ring of more than 2^28 samples: lower push_budget or max_input_rate")
        self.R_in = 1 << self.r_in
        self.in_rings = None
        self._rates = []            # distinct input rates of the session's streams so far (segments name them by index)
        self.max_streams = int(max_streams)
        self.max_step_frames = int(max_step_frames) if max_step_frames else int(engine.max_frames)
        self.stream = None          # the session's CUDA stream, rings and counters: made by the first step (open / push / close
        self.rings = None           # check their arguments on the host and touch no device)
        self._free = list(range(self.max_streams - 1, -1, -1))
        self._streams = {}
        self._next_sid = 0
        self._fe_ws = None
        self._ws = None
        self._stage = None          # pinned upload buffer and the event of the copy that last read it
        self._stage_ev = None
        self._dev = None            # device side of the upload
        self._fe_repairs = None
        self._lstm_carried = 0      # time-LSTM repairs counted in model workspaces the session has since replaced
        self.last_calls = {}        # what the last step enqueued (host -> device copies and library calls)

    def _device_init(self):
        if self.stream is not None:
            return
        self.stream = torch.cuda.Stream(self.device)
        # made on the session's stream, where they are used: the allocator then orders their reuse behind the session's kernels
        with torch.cuda.stream(self.stream):
            self.rings = torch.zeros(self.max_streams * (self.R + RING_MIRROR), dtype=torch.float32, device=self.device)
            self._fe_repairs = torch.zeros(1, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ streams
    def open(self, speaker_id, ensembling_ms=0, input_rate=None, gain=1.0):
        """A new stream for speaker `speaker_id`; its frames average two passes when ensembling_ms > 0 (model.py:373-384).
        With `input_rate` the stream takes samples at that rate and converts them on the device, times `gain`, clamped to
        +-0.999 (input_rate = the model rate: gain and clamp alone); without it `gain` must stay 1.  Returns the stream id."""
        self.eng.check_speaker_ids(int(speaker_id))
        gain = float(gain)
        f32 = np.finfo(np.float32)
        if not float(f32.tiny) <= gain <= float(f32.max):          # (NaN fails the comparison too)
            raise ValueError(f"gain must be finite and > 0, not {gain!r}")
        if input_rate is None:
            if gain != 1.0:
                raise ValueError("gain needs input_rate: a stream at the model rate is taken as it is")
        else:
            if int(input_rate) != input_rate or int(input_rate) <= 0:
                raise ValueError(f"input_rate must be a positive integer, not {input_rate!r}")
            input_rate = int(input_rate)
            if input_rate > self.max_input_rate:
                raise ValueError(f"input_rate={input_rate} is above this session's max_input_rate={self.max_input_rate}")
            resample_final(0, input_rate, self.sr)                # a rate pair the offline call refuses: its message
            if input_rate not in self._rates and len(self._rates) >= MAX_RATES:
                raise ValueError(f"a session takes at most {MAX_RATES} distinct input rates")
        ens = int(ensembling_ms or 0)
        if ens < 0:
            raise ValueError("ensembling_ms must be >= 0")
        pad = ens * self.sr // 1000
        if pad > self.max_pad:
            raise ValueError(f"ensembling_ms={ens} is above this session's max_ensembling_ms")
        if pad > 0 and self.outputs == "coef":
            raise ValueError("outputs='coef' cannot ensemble: the reference averages rows, not coefficients")
        if not self._free:
            raise RuntimeError(f"all {self.max_streams} streams of the session are open")
        sid = self._next_sid
        self._next_sid += 1
        if input_rate is not None and input_rate not in self._rates:
            self._rates.append(input_rate)
        st = self._streams[sid] = _Stream(sid, self._free.pop(), int(speaker_id), pad, input_rate, gain)
        if input_rate is not None:
            st.wing = resample_wing(input_rate, self.sr) + 1
        return sid

    def _get(self, sid):
        st = self._streams.get(sid)
        if st is None:
            raise KeyError(f"no open stream {sid}")
        if st.closing:
            raise ValueError(f"stream {sid} is closed")
        return st

    def _oldest_needed(self, st):
        """First ring position whose content a frame not yet computed uses: its window from s - 1 (the column 0 request) in
        the delayed view, s - pad - 1.  Nothing below -pad is ever used: positions before the stream read as zero by selection,
        and the one-run column form starts at p - 1 >= -pad (the zeros appended ahead of the stream)."""
        s, _ = frame_positions(st.emitted, 1, self.sr)
        return max(int(s[0]) - st.pad - 1, -st.pad)

    def push(self, sid, pcm):
        """Appends samples (float32 in [-1, 1], at the stream's input rate: the model rate unless it was opened with another) to
        stream `sid`."""
        st = self._get(sid)
        x = pcm.detach().cpu().numpy() if torch.is_tensor(pcm) else np.asarray(pcm)
        x = np.asarray(x, np.float32).reshape(-1)
        if x.size == 0:
            return
        if not (x.min() >= -1 and x.max() <= 1):                 # generate_animation's input check (model.py:339-349)
            raise ValueError("samples must lie in [-1, 1]")
        if st.rate is not None:
            return self._push_input(st, x)
        if st.n_total + x.size > MAX_SAMPLES:
            final_frames(st.n_total + x.size, self.sr)            # raises sdfa_frame_index's message
        pos = 0
        while pos < x.size:
            room = self._oldest_needed(st) + self.R - st.n_total
            if room <= 0:
                # R >= sliding + pad + budget + 1 makes a step free room: every frame ending before n is then emitted
                emitted = st.emitted
                self._run_step()
                if st.emitted == emitted:
                    raise RuntimeError("live session: a forced step freed no ring space (ring too small for this stream)")
                continue
            take = min(room, x.size - pos)
            st.pending.append(x[pos:pos + take])
            st.n_total += take
            pos += take

    def _push_input(self, st, x):
        """push() of a capture-rate stream.  Two rings bound what fits before a step: the input ring keeps every sample from the left
        wing of the first output not yet resampled, and the model ring takes the outputs the samples make final."""
        pos = 0
        while pos < x.size:
            oldest = st.n_dev if st.rate == self.sr else int(st.treg) - st.wing   # equal rates: a copy, no wings
            room = oldest + self.R_in - st.in_total
            take = min(room, x.size - pos)
            if take > 0:
                cap = self._oldest_needed(st) + self.R           # model-rate length the model ring can take before a step
                n = resample_final(st.in_total + take, st.rate, self.sr)
                if n > cap:
                    lo, hi = 0, take                              # the most samples whose final outputs fit (final is monotone)
                    while hi - lo > 1:
                        mid = (lo + hi) // 2
                        if resample_final(st.in_total + mid, st.rate, self.sr) <= cap:
                            lo = mid
                        else:
                            hi = mid
                    take = lo
                    n = resample_final(st.in_total + take, st.rate, self.sr)
            if take <= 0:
                before = (st.emitted, st.n_dev)
                self._run_step()
                if (st.emitted, st.n_dev) == before:
                    raise RuntimeError("live session: a forced step freed no ring space (rings too small for this stream)")
                continue
            if n > MAX_SAMPLES:
                final_frames(n, self.sr)                          # raises sdfa_frame_index's message
            st.pending.append(x[pos:pos + take])
            st.in_total += take
            st.n_total = n
            pos += take

    def close(self, sid):
        """Ends stream `sid`: the next step emits its tail frames (zero padding past the end, as offline).  A stream shorter than
        one window raises the offline call's short-clip AssertionError and is dropped; other streams are unaffected."""
        st = self._get(sid)
        try:
            if st.rate is not None:
                n_out, n_res = resample_close(st.in_total, st.rate, self.sr)      # raises what the offline resample raises
                if n_out > self._oldest_needed(st) + self.R:
                    # the outputs held back until now do not fit the model ring: a step computes the final frames and frees it
                    self._run_step()
                    if n_out > self._oldest_needed(st) + self.R:
                        raise RuntimeError("live session: the model ring cannot take the stream's tail (push_budget too small)")
                st.n_total, st.n_res = n_out, n_res
            st.end = close_frames(st.n_total, self.sr)
        except Exception:
            self._drop(st)
            raise
        st.closing = True

    def _drop(self, st):
        self._streams.pop(st.sid, None)
        self._free.append(st.ring)

    # ------------------------------------------------------------------ step
    def step(self):
        """Runs every stream's final frames.  Returns {sid: (tslist int32 ndarray, output)} for the streams with new frames (and
        closed streams); output = (n, out_dim) rows or (n, coef_dim) coefficients on the device (ready in the caller's
        current stream's order, and kept from reuse by the session until the work the caller queues on that stream has used
        them) -- a pinned host copy with host_copy=True."""
        self._run_step()
        if self.stream is None:             # nothing was ever pushed
            return {}
        res = {}
        for st in list(self._streams.values()):
            if st.out_ts or st.closing:
                ts = np.concatenate(st.out_ts) if st.out_ts else np.empty(0, np.int32)
                if not st.out_rows:
                    rows = torch.empty((0, self._width()), dtype=torch.float32, device=self.device)
                elif len(st.out_rows) == 1:
                    rows = st.out_rows[0]
                else:
                    with torch.cuda.stream(self.stream):
                        rows = torch.cat(st.out_rows)
                res[st.sid] = (ts, rows)
                st.out_ts, st.out_rows = [], []
            if st.closing:
                self._drop(st)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.stream)
        if not self.host_copy:
            # the outputs were made on the session's stream: without this, a later step could be handed their memory as soon as
            # the caller drops them, while kernels the caller queued behind them on its own stream still read it
            for _, rows in res.values():
                if rows.numel():
                    rows.record_stream(cur)
        if self.host_copy and res:
            with torch.cuda.stream(self.stream):
                host = {sid: (ts, torch.empty(rows.shape, dtype=torch.float32, pin_memory=True).copy_(rows, non_blocking=True))
                        for sid, (ts, rows) in res.items()}
            self.stream.synchronize()
            res = host
        return res

    def _width(self):
        return self.eng.coef_dim if self.outputs == "coef" else self.eng.out_dim

    def _run_step(self):
        sts = list(self._streams.values())
        # streams that ensemble first: their main frames are then one block, averaged with the delayed block in one call
        sts.sort(key=lambda s: (s.pad == 0, s.sid))
        segs, srcs, src_n = [], [], 0
        in_segs, rs_segs, tregs, treg_n, rs_max = [], [], [], 0, 0
        for st in sts:
            if st.rate is not None:
                if st.pending:
                    cnt = st.in_total - st.in_dev
                    in_segs.append((st.ring, st.in_dev, cnt, src_n))
                    srcs.extend(st.pending)
                    src_n += cnt
                if st.n_total > st.n_dev:
                    # outputs n_dev .. n_total - 1, and the zeros at -pad .. -1 ahead of the first of an ensembling stream
                    lead = st.pad if st.n_dev == 0 else 0
                    n_reg = max(min(st.n_total, st.n_res) - st.n_dev, 0) if st.rate != self.sr else 0
                    reg, st.treg = resample_register(st.treg, n_reg, st.rate, self.sr)
                    rate_gain = self._rates.index(st.rate) | (int(np.float32(st.gain).view(np.uint32)) << 32)
                    rs_segs.append((st.ring, st.ring, st.n_dev - lead, st.n_total - st.n_dev + lead, st.in_total, st.n_res, treg_n,
                                    rate_gain - (1 << 64) if rate_gain >= 1 << 63 else rate_gain))
                    tregs.append(reg)
                    treg_n += n_reg
                    rs_max = max(rs_max, st.n_total - st.n_dev + lead)
                continue
            if st.pending:
                cnt = st.n_total - st.n_dev
                lead = st.pad if st.n_dev == 0 else 0      # positions -pad .. -1 of a delayed view read as zeros
                segs.append((st.ring, st.n_dev - lead, cnt + lead, src_n))
                if lead:
                    srcs.append(np.zeros(lead, np.float32))
                srcs.extend(st.pending)
                src_n += cnt + lead
        # frames: per stream the range [emitted, final) -- or [emitted, end) once closed
        work = []
        for st in sts:
            k1 = st.end if st.closing else final_frames(st.n_total, self.sr)
            if k1 > st.emitted:
                work.append((st, st.emitted, k1))
        if not segs and not in_segs and not rs_segs and not work:
            return
        self._device_init()
        if in_segs and self.in_rings is None:
            with torch.cuda.stream(self.stream):
                self.in_rings = torch.zeros(self.max_streams * (self.R_in + RING_MIRROR), dtype=torch.float32, device=self.device)
        ens_any = any(st.pad > 0 for st, _, _ in work)
        cap = max(1, self.max_step_frames // (2 if ens_any else 1))
        # launch groups of at most `cap` main frames; each holds its streams' main frames, then the delayed ones
        groups, cur, cur_n = [], [], 0
        for st, k0, k1 in work:
            k = k0
            while k < k1:
                take = min(k1 - k, cap - cur_n)
                cur.append((st, k, k + take))
                cur_n += take
                k += take
                if cur_n == cap:
                    groups.append(cur)
                    cur, cur_n = [], 0
        if cur:
            groups.append(cur)
        # views: 2 per stream (main, delayed) -> (ring, valid_hi)
        vidx = {}
        view_ring, view_hi = [], []
        for st in sts:
            vidx[st.sid] = len(view_ring)
            view_ring += [st.ring, st.ring | (st.pad << 32)]
            view_hi += [st.n_total, max(st.n_total - st.pad, 0)]
        fstart, fview, fspk, tsl, layout = [], [], [], [], []
        for g in groups:
            m = d = 0
            for st, k0, k1 in g:
                s, ts = frame_positions(k0, k1 - k0, self.sr)
                fstart.append(s); fview.append(np.full(k1 - k0, vidx[st.sid], np.int32)); fspk.append(np.full(k1 - k0, st.speaker, np.int64))
                tsl.append(ts)
                m += k1 - k0
            for st, k0, k1 in g:
                if st.pad > 0:
                    s, _ = frame_positions(k0, k1 - k0, self.sr)
                    fstart.append(s - st.pad); fview.append(np.full(k1 - k0, vidx[st.sid] + 1, np.int32))
                    fspk.append(np.full(k1 - k0, st.speaker, np.int64))
                    d += k1 - k0
            layout.append((m, d))
        # ONE upload: [segments | view ring | view hi | frame starts | speaker ids | input-ring segments | resample segments |
        # time registers (float64)] int64, frame views int32, samples float32
        nseg, nv = len(segs), len(view_ring)
        nf = int(sum(a.size for a in fstart))
        i64 = np.concatenate([np.asarray(segs, np.int64).reshape(-1), np.asarray(view_ring, np.int64), np.asarray(view_hi, np.int64)]
                             + fstart + fspk + [np.asarray(in_segs, np.int64).reshape(-1), np.asarray(rs_segs, np.int64).reshape(-1)]
                             + [t.view(np.int64) for t in tregs])
        fv = np.concatenate(fview) if fview else np.empty(0, np.int32)
        o_fv = i64.size * 8
        o_pcm = (o_fv + fv.size * 4 + 15) // 16 * 16
        total = o_pcm + src_n * 4
        if self._stage_ev is not None:
            self._stage_ev.synchronize()
        if self._stage is None or self._stage.numel() < total:
            self._stage = torch.empty(max(int(total * 1.5), 1 << 16), dtype=torch.uint8, pin_memory=True)
        st_np = self._stage.numpy()
        st_np[:o_fv].view(np.int64)[:] = i64
        st_np[o_fv:o_fv + fv.size * 4].view(np.int32)[:] = fv
        if src_n:
            pcm = st_np[o_pcm:total].view(np.float32)
            o = 0
            for c in srcs:
                pcm[o:o + c.size] = c
                o += c.size
        calls = {"h2d_copy": 1, "ring_append": 0, "resample": 0, "frontend_ring": 0, "encoder": 0, "regress": 0, "ensemble_mean": 0,
                 "status_add": 0}
        with torch.cuda.stream(self.stream):
            if self._dev is None or self._dev.numel() < total:
                self._dev = None
                self._dev = torch.empty(max(int(total * 1.5), 1 << 16), dtype=torch.uint8, device=self.device)
            dev = self._dev
            dev[:total].copy_(self._stage[:total], non_blocking=True)
            self._stage_ev = torch.cuda.Event()
            self._stage_ev.record(self.stream)
            sp = C.c_void_p(self.stream.cuda_stream)
            base = dev.data_ptr()
            d_seg = base
            d_vring = base + nseg * 32
            d_vhi = d_vring + nv * 8
            d_fstart = d_vhi + nv * 8
            d_fspk = d_fstart + nf * 8
            d_fview = base + o_fv
            if nseg:
                check(lib.sdfa_stream_ring_append(_ptr(self.rings), self.r, self.max_streams, C.c_void_p(d_seg), nseg,
                                                  C.c_void_p(base + o_pcm), src_n, sp))
                calls["ring_append"] += 1
            if in_segs:
                d_inseg = d_fspk + nf * 8
                check(lib.sdfa_stream_ring_append(_ptr(self.in_rings), self.r_in, self.max_streams, C.c_void_p(d_inseg), len(in_segs),
                                                  C.c_void_p(base + o_pcm), src_n, sp))
                calls["ring_append"] += 1
            if rs_segs:
                d_rsseg = d_fspk + nf * 8 + len(in_segs) * 32
                rates = (C.c_int32 * len(self._rates))(*self._rates)
                check(lib.sdfa_stream_resample(_ptr(self.in_rings), self.r_in, self.max_streams, _ptr(self.rings), self.r, self.max_streams,
                                               C.c_void_p(d_rsseg), len(rs_segs), rs_max, C.c_void_p(d_rsseg + len(rs_segs) * 64), treg_n,
                                               rates, len(self._rates), self.sr, sp))
                calls["resample"] += 1
            for st in sts:
                if st.rate is not None:
                    st.in_dev, st.n_dev, st.pending = st.in_total, st.n_total, []
                elif st.pending:
                    st.n_dev = st.n_total
                    st.pending = []
            f0 = 0
            t0 = 0
            for g, (m, d) in zip(groups, layout):
                n = m + d
                self._group(g, m, d, d_vring, d_vhi, nv, d_fview + 4 * f0, d_fstart + 8 * f0, d_fspk + 8 * f0, sp, calls)
                # hand the rows out per stream
                r0 = 0
                for st, k0, k1 in g:
                    st.out_ts.append(tsl[t0])
                    st.out_rows.append(self._last_out[r0:r0 + (k1 - k0)])
                    st.emitted = k1
                    r0 += k1 - k0
                    t0 += 1
                f0 += n
        self.last_calls = calls

    def _group(self, g, m, d, d_vring, d_vhi, nv, d_fview, d_fstart, d_fspk, sp, calls):
        """Front end, encoder, regressor (and the ensembling mean) of one launch group: m main frames, then d delayed ones."""
        eng, n = self.eng, m + d
        need = int(check(lib.sdfa_frontend_workspace_bytes(n)))
        if self._fe_ws is None or self._fe_ws.numel() < need:
            self._fe_ws = None
            self._fe_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        feat = torch.empty((n,) + FEAT_SHAPE, dtype=torch.float32, device=self.device)
        check(lib.sdfa_mel_frontend_ring(_ptr(self.rings), self.r, self.max_streams, C.c_void_p(d_vring), C.c_void_p(d_vhi), nv,
                                         C.c_void_p(d_fview), C.c_void_p(d_fstart), n, self.sr, _ptr(feat), _ptr(self._fe_ws),
                                         self._fe_ws.numel(), sp))
        self._fe_repairs += self._fe_ws[32:36].view(torch.int32)     # the front end's status word (zeroed by every call)
        calls["frontend_ring"] += 1
        calls["status_add"] += 1
        wneed = int(check(lib.sdfa_workspace_bytes(eng._m, n)))
        if self._ws is None or self._ws.numel() < wneed:
            self._lstm_carried += self._ws_status() if self._ws is not None else 0
            self._ws = None
            self._ws = torch.empty(wneed, dtype=torch.uint8, device=self.device)
            check(lib.sdfa_workspace_init(_ptr(self._ws), self._ws.numel(), sp))
        z = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        check(lib.sdfa_encoder_forward_shared(eng._m, _ptr(feat), n, C.c_void_p(d_fview), C.c_void_p(d_fstart), self.hop, _ptr(z), None,
                                              _ptr(self._ws), self._ws.numel(), sp))
        coef = out = None
        if self.outputs == "coef":
            coef = torch.empty((n, eng.coef_dim), dtype=torch.float32, device=self.device)
        else:
            out = torch.empty((n, eng.out_dim), dtype=torch.float32, device=self.device)
        check(lib.sdfa_regress_forward(eng._m, _ptr(z), C.c_void_p(d_fspk), n, None if coef is None else _ptr(coef),
                                       None if out is None else _ptr(out), _ptr(self._ws), self._ws.numel(), sp))
        calls["encoder"] += 1
        calls["regress"] += 1
        if d:
            # the ensembling streams' main frames are rows 0 .. d - 1 (sorted first), their delayed frames rows m .. m + d - 1
            check(lib.sdfa_ensemble_mean(_ptr(out), C.c_void_p(out.data_ptr() + m * eng.out_dim * 4), d * eng.out_dim, _ptr(out), sp))
            calls["ensemble_mean"] += 1
        self._last_out = (coef if coef is not None else out)[:m]

    def _ws_status(self):
        return int(check(lib.sdfa_workspace_status(_ptr(self._ws), 0, C.c_void_p(self.stream.cuda_stream))))

    # ------------------------------------------------------------------ health
    def health(self):
        """Status words of the session's workspaces (synchronises the session's stream): time-LSTM waits that expired and were
        repaired on the device, and front-end hand-off waits that expired and were repaired -- rows are right either way; a
        count that grows says the device was oversubscribed (include/sdfa_hip.h "Status block")."""
        if self.stream is None:
            return {"time_lstm_repairs": 0, "frontend_repairs": 0, "open_streams": len(self._streams)}
        lstm = self._lstm_carried + (self._ws_status() if self._ws is not None else 0)
        self.stream.synchronize()
        return {"time_lstm_repairs": lstm, "frontend_repairs": int(self._fe_repairs.item()),
                "open_streams": len(self._streams)}
