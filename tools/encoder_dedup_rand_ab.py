"""The input the scan cannot help: Engine.encoder on 8,192 frames of torch.rand features, switch on / off alternating in one
process, HIP-event times, with the library's per-stage profile of each side."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
import torch
from sdfa_amd import synth, _lib
from sdfa_amd.engine import Engine

N, REPS, ROUNDS = 8192, 3, 4
eng = Engine(synth.make_state_dict("dgrad", 1234), max_frames=N)
feat = torch.rand((N, 64, 128, 3), generator=torch.Generator().manual_seed(1)).cuda()
STAGES = ("share_map", "conv23", "freq_lstm", "freq_proj", "gx0", "lstm0", "gx1", "lstm1", "attn_proj", "attn")


def run(off):
    _lib.set_option("encoder_dedup_off", off)
    eng.profile(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        eng.encoder(feat, want_align=False)
    e1.record()
    torch.cuda.synchronize()
    st = {}
    for k in STAGES:
        try:
            st[k] = round(eng.profile_ms(k) / REPS, 3)
        except Exception:
            pass
    eng.profile(False)
    _lib.set_option("encoder_dedup_off", 0)
    return e0.elapsed_time(e1) / REPS, st


for off in (0, 1):      # warm both
    run(off)
times = {0: [], 1: []}
for r in range(ROUNDS):
    for off in (0, 1):
        ms, st = run(off)
        times[off].append(ms)
        print(f"round {r} encoder_dedup_off={off}: {ms:.3f} ms per 8192-frame call  stages {st}")
print("distinct columns (switch on):", end=" ")
_lib.set_option("encoder_dedup_off", 0)
eng.encoder(feat, want_align=False)
print(eng.distinct_columns(N), "of", 64 * N)
on, off = sorted(times[0])[len(times[0]) // 2 - 1: len(times[0]) // 2 + 1], sorted(times[1])[len(times[1]) // 2 - 1: len(times[1]) // 2 + 1]
mon, moff = sum(on) / 2, sum(off) / 2
print(f"median on {mon:.3f} ms, off {moff:.3f} ms, slow-down {100 * (mon / moff - 1):.2f} %")
