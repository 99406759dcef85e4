"""Live streaming throughput (sdfa_amd/live.py): S streams each push 1/60 s of synthetic speech-like audio per tick, then one
step() runs every stream's new frames.  Per (rate, S, output mode): wall time of the pushes and of the step (the step timed to the
device's completion), p50 / p99 over the measured ticks, and whether a 60 ticks/s cadence fits.  Synthetic dgrad weights (the
timing does not depend on the values).  With --input-rate the streams are capture-rate streams: each pushes 1/60 s of audio at that
rate per tick and the step resamples it on the device (default output profiles/live_resample_bench.json).

  python tools/live_bench.py --out profiles/live_bench.json [--ticks 60] [--streams 1,64,256,1024,2048] [--input-rate 44100]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

from sdfa_amd import synth, live                      # noqa: E402
from sdfa_amd.engine import Engine, frame_geometry    # noqa: E402

TICK_MS = 1000.0 / 60


def run(eng, sr, S, mode, ticks, pcm, input_rate=None):
    outputs, host = {"rows": ("rows", False), "rows+host": ("rows", True), "coef+host": ("coef", True)}[mode]
    if input_rate is None:
        s = live.LiveSession(eng, S, sample_rate=sr, outputs=outputs, host_copy=host, max_step_frames=eng.max_frames)
        sids = [s.open(i % 8) for i in range(S)]
    else:
        s = live.LiveSession(eng, S, sample_rate=sr, outputs=outputs, host_copy=host, max_step_frames=eng.max_frames, max_input_rate=input_rate)
        sids = [s.open(i % 8, input_rate=input_rate, gain=0.9) for i in range(S)]
    per_tick = (input_rate or sr) // 60
    _, _, sliding = frame_geometry(sr)
    warm = sliding // (sr // 60) + (3 if input_rate is None else 5)      # until every stream emits a frame per tick
    pos, push_ms, step_ms, frames = 0, [], [], []
    for t in range(warm + ticks):
        t0 = time.perf_counter()
        for i, sid in enumerate(sids):
            o = (pos + 977 * i) % (len(pcm) - per_tick)
            s.push(sid, pcm[o:o + per_tick])
        t1 = time.perf_counter()
        res = s.step()
        torch.cuda.current_stream().synchronize()
        t2 = time.perf_counter()
        pos += per_tick
        if t >= warm:
            push_ms.append((t1 - t0) * 1e3)
            step_ms.append((t2 - t1) * 1e3)
            frames.append(sum(len(v[0]) for v in res.values()))
    calls = dict(s.last_calls)
    h = s.health()
    for sid in sids:
        s.close(sid)
    s.step()
    p = lambda a, q: float(np.percentile(a, q))
    tot = [a + b for a, b in zip(push_ms, step_ms)]
    extra = {} if input_rate is None else {"input_rate": input_rate, "input_ring_samples": s.R_in}
    return {**extra, "sr": sr, "streams": S, "mode": mode, "ticks": ticks, "frames_per_tick_mean": float(np.mean(frames)),
            "step_ms_p50": p(step_ms, 50), "step_ms_p99": p(step_ms, 99), "push_ms_p50": p(push_ms, 50), "push_ms_p99": p(push_ms, 99),
            "tick_ms_p99": p(tot, 99), "sustains_60_ticks_per_s": p(tot, 99) <= TICK_MS, "calls_per_step": calls, "health": h,
            "ring_samples": s.R}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--input-rate", type=int, default=None, help="capture rate of every stream (default: streams at the model rate)")
    ap.add_argument("--modes", default="rows,rows+host,coef+host")
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--streams", default="1,64,256,1024,2048,4096")
    ap.add_argument("--rates", default="8000,16000")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "live_bench.json" if a.input_rate is None else "live_resample_bench.json")
    results = []
    sd = synth.make_state_dict("dgrad", 1234)
    for sr in [int(x) for x in a.rates.split(",")]:
        eng = Engine(sd, device="cuda:0", max_frames=8192)
        pcm = synth.make_pcm(5, 20 * (a.input_rate or sr))
        best = 0
        for S in [int(x) for x in a.streams.split(",")]:
            row = None
            for mode in a.modes.split(","):
                row = run(eng, sr, S, mode, a.ticks, pcm, a.input_rate)
                results.append(row)
                print(json.dumps(row), flush=True)
            ok = [r for r in results if r["sr"] == sr and r["streams"] == S and r["mode"] == a.modes.split(",")[0]][0]["sustains_60_ticks_per_s"]
            if ok:
                best = S
            else:
                break
        results.append({"sr": sr, "largest_S_sustaining_60_ticks_per_s_rows_on_device": best,
                        "note": "largest S of the list tried (device rows, no host copy) whose p99 push + step fits 16.7 ms"})
        del eng
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
    print(json.dumps(results[-1]))


if __name__ == "__main__":
    main()
