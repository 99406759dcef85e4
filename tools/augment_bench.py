"""Augmented training-window features on the MI355X: sdfa_augment_frontend on a reference training batch
(2 x 100 windows) and on 20,352 windows, against the per-window sdfa_mel_frontend on the same count of neutral windows in the same
process -- the floor the kernel sits on: the same transform without cut extension, noise, resize, gain and dropout -- and against
the reference-route host loop for one batch.  bench.py (the headline workload) is not involved.

  python tools/augment_bench.py --out profiles/augment_bench.json

Windows   random starts over --clips (32) synthetic clips of 10 s at --sr (16000); every descriptor field drawn as the reference's
          __getitem__ draws it (ex_time -4..4, ex_feat -5..5, flags, pre-emphasis 0..0.95, a dropout mask of up to 19 rows), noise and
          scale present.  The neutral windows have the same starts.
Timed     each call by device events after a warm-up call; median of --reps.  The noise is drawn before the clock starts;
          sdfa_amd.augment.white_noise (torch.randn) is timed on its own.
Host      windowed_features restated with numpy in float32 (cut, noise, pre-emphasis, rfft, mel, dB, np.pad edit, bilinear resize,
          gain, dropout, deltas), one window after the other in this process; the reference spreads the same loop over its
          data-loader workers.  --host-windows (200) windows, wall clock.
No threshold is set: nobody had measured any of this."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def draw(rs, n, n_clips, clip_len, sliding):
    from sdfa_amd import augment
    masks = [rs.choice(128, max(1, int(rs.uniform(0, 0.15) * 128))) if rs.rand() < 0.5 else [] for _ in range(n)]
    fields = dict(clip=rs.randint(0, n_clips, n), start=rs.randint(-sliding // 2, clip_len - sliding // 2, n), ex_time=rs.randint(-4, 5, n),
                  preemph=rs.uniform(0, 0.95, n), ex_feat=rs.randint(-5, 6, n), lower_freq=rs.rand(n) < 0.5, trunck=rs.rand(n) < 0.5,
                  pad_reflect=rs.rand(n) < 0.5, drop=masks)
    scale = np.exp(np.sin(np.linspace(0, 2 * np.pi, 128)[None] * rs.uniform(-np.pi / 2, np.pi / 2, (n, 1)) + rs.uniform(0, np.pi, (n, 1))) * 0.15)
    noise_scale = np.where(rs.rand(n) < 0.5, rs.uniform(0.002, 0.01, n), 0.0)
    return fields, augment.pack_desc(**fields), scale.astype(np.float32), noise_scale


def resize_f32(img, h_out, w_out):
    f32 = np.float32

    def taps(n_in, n_out):
        f = ((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5).astype(f32)
        i0 = np.floor(f).astype(np.int64)
        f = f - i0.astype(f32)
        edge = (i0 < 0) | (i0 >= n_in - 1)
        f[edge] = 0
        i0 = np.clip(i0, 0, n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), f
    x0, x1, fx = taps(img.shape[1], w_out)
    y0, y1, fy = taps(img.shape[0], h_out)
    rows = img[:, x0] * (f32(1) - fx) + img[:, x1] * fx
    return rows[y0] * (f32(1) - fy)[:, None] + rows[y1] * fy[:, None]


def host_loop(clips, fields, scale, noise_scale, sr, count):
    """The reference's route for `count` windows, numpy float32.  Returns (seconds, features)."""
    import librosa_restate as lr
    win, hop = int(0.064 * sr), int(0.008 * sr)
    sliding = 63 * hop + win
    hamm = np.hamming(win).astype(np.float32)
    melw = lr.mel_filters(sr, win, 128, 50, 3600).astype(np.float32)
    used = int(np.nonzero(melw.any(0))[0].max()) + 1
    rs = np.random.RandomState(1)
    out = []
    t0 = time.perf_counter()
    for i in range(count):
        sig = clips[int(fields["clip"][i])]
        et, ef = int(fields["ex_time"][i]), int(fields["ex_feat"][i])
        wl, wr = int(fields["start"][i]) - et * hop, int(fields["start"][i]) + sliding + et * hop
        wav = np.zeros(wr - wl, np.float32)
        lo, hi = max(wl, 0), min(wr, len(sig))
        if hi > lo:
            wav[lo - wl:hi - wl] = sig[lo:hi]
        if noise_scale[i] > 0:
            wav += rs.normal(0, noise_scale[i], wr - wl).astype(np.float32)
        a = np.float32(fields["preemph"][i])
        wav = np.append(wav[0], wav[1:] - a * wav[:-1])
        fr = np.lib.stride_tricks.sliding_window_view(wav, win)[::hop] * hamm
        p = np.abs(np.fft.rfft(fr, axis=1)).astype(np.float32) ** 2
        # einsum's own loops over the bins that carry weight: a BLAS call of this size spends its time starting threads
        db = 10 * np.log10(np.maximum(np.einsum("tb,mb->tm", p[:, :used], melw[:, :used]), np.float32(1.1920929e-07)))
        feat = np.clip((db - 20 + 80) / 80, 0, 1).astype(np.float32).T                     # (128, T)
        if ef < 0:
            feat = feat[-ef:] if fields["lower_freq"][i] else feat[:ef]
        elif ef > 0 and fields["lower_freq"][i]:
            feat = np.pad(feat, [[ef, 0], [0, 0]], "constant")
            feat = feat[:-ef] if fields["trunck"][i] else feat
        elif ef > 0:
            feat = np.pad(feat, [[0, ef], [0, 0]], "reflect" if fields["pad_reflect"][i] else "constant")
            feat = feat[ef:] if fields["trunck"][i] else feat
        feat = resize_f32(feat, 128, 64) * scale[i][:, None]
        feat[np.asarray(fields["drop"][i], np.int64)] = 0
        out.append(np.stack([feat, lr.delta(feat, 9, 1, -1, "interp"), lr.delta(feat, 9, 2, -1, "interp")]).astype(np.float32).transpose(2, 1, 0))
    return time.perf_counter() - t0, np.stack(out)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 20352])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-windows", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    import ctypes as C
    import torch
    from sdfa_amd import augment, synth
    from sdfa_amd._lib import lib, check
    assert torch.cuda.is_available(), "augment_bench needs the MI355X"
    sr = args.sr
    win, hop = int(0.064 * sr), int(0.008 * sr)
    sliding = 63 * hop + win
    clips = [synth.make_pcm(c, 10 * sr) for c in range(args.clips)]
    pcm, off, ln = augment.upload_clips(clips)
    stride = augment.noise_samples(sr)
    p = lambda t: C.c_void_p(t.data_ptr())
    report = {"sample_rate": sr, "clips": args.clips, "clip_seconds": 10, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    host = None
    for n in args.sizes:
        fields, desc, scale, noise_scale = draw(np.random.RandomState(n), n, args.clips, 10 * sr, sliding)
        d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).cuda()
        d_scale = torch.from_numpy(scale).cuda()
        noise_ms = timed(lambda: augment.white_noise(n, stride, noise_scale), args.reps)
        d_noise = augment.white_noise(n, stride, noise_scale)
        out = torch.empty((n, 64, 128, 3), dtype=torch.float32, device="cuda")
        aug_ms = timed(lambda: augment.augment_frontend(pcm, off, ln, d_desc, sr, d_noise, d_scale, out), args.reps)
        bare_ms = timed(lambda: augment.augment_frontend(pcm, off, ln, d_desc, sr, None, None, out), args.reps)
        assert bool(torch.isfinite(out).all())
        d_fc = torch.from_numpy(np.asarray(fields["clip"], np.int32)).cuda()
        d_fs = torch.from_numpy(np.asarray(fields["start"], np.int64)).cuda()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        base_ms = timed(lambda: check(lib.sdfa_mel_frontend(p(pcm), p(off), p(ln), args.clips, p(d_fc), p(d_fs), n, sr, p(out), st)), args.reps)
        a, b, c = statistics.median(aug_ms), statistics.median(base_ms), statistics.median(bare_ms)
        report["sizes"][str(n)] = {
            "windows": n, "augment_ms": aug_ms, "augment_ms_median": a, "augment_without_noise_and_scale_ms_median": c,
            "mel_frontend_per_window_ms": base_ms, "mel_frontend_per_window_ms_median": b, "ratio_to_mel_frontend": a / b,
            "white_noise_ms_median": statistics.median(noise_ms), "us_per_window": 1e3 * a / n,
            "bytes_written": n * 64 * 128 * 3 * 4, "noise_bytes_read": n * stride * 4}
        if host is None and n >= args.host_windows:
            host = (fields, scale, noise_scale, a * args.host_windows / n)
    if host is not None and args.host_windows > 0:
        fields, scale, noise_scale, gpu_ms = host
        host_loop(clips, fields, scale, noise_scale, sr, 2)                                # warm-up (imports, FFT plans)
        s, _ = host_loop(clips, fields, scale, noise_scale, sr, args.host_windows)
        report["host_loop"] = {"windows": args.host_windows, "seconds": s, "ms_per_window": 1e3 * s / args.host_windows,
                               "how": "numpy float32 restatement of windowed_features, one process, one window after the other",
                               "ratio_to_augment": 1e3 * s / gpu_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
