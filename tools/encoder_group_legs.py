"""The encoder on the headline batch (32 clips of 10 s at 16 kHz, chunks of 8,192 / 8,192 / 3,968 frames), three ways in one process:
the default call (the map from the features themselves), the frame-table call and "encoder_dedup_off" = 1, alternating.  Prints the
distinct fraction of each chunk for the two maps, and per leg the HIP-event time of the call and the library's per-stage times per
step -- share_map and lstm0 above all (profiles/encoder_group_ab.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
import torch
from sdfa_amd import synth, _lib
from sdfa_amd.engine import Engine

SR, CHUNK, REPS, ROUNDS = 16000, 8192, 3, 3
eng = Engine(synth.make_state_dict("dgrad", 1234), max_frames=CHUNK)
feat, _, _ = eng.mel_frontend([synth.make_pcm(c, 10 * SR) for c in range(32)], SR)
fc, fs, hop = eng.last_frame_table
n = feat.shape[0]
STAGES = ("share_map", "conv23", "freq_lstm", "freq_proj", "gx0", "lstm0", "gx1", "lstm1", "attn_proj", "attn")
LEGS = {"default": {}, "table": dict(frame_clip=fc, frame_start=fs, hop=hop), "off": {}}

for f0 in range(0, n, CHUNK):
    m = min(CHUNK, n - f0)
    d, ms = {}, {}
    for leg in ("default", "table"):
        kw = dict(frame_clip=fc[f0:f0 + m], frame_start=fs[f0:f0 + m], hop=hop) if leg == "table" else {}
        eng.encoder(feat[f0:f0 + m], want_align=False, **kw)
        d[leg] = eng.distinct_columns(m)
        eng.profile(True)
        for _ in range(REPS):
            eng.encoder(feat[f0:f0 + m], want_align=False, **kw)
        ms[leg] = (eng.profile_ms("share_map") / REPS, eng.profile_ms("lstm0") / REPS)
        eng.profile(False)
    print(f"chunk at {f0}: {m} frames of {64 * m} columns; distinct default {d['default']} ({d['default'] / (64 * m):.4f}) table {d['table']} "
          f"({d['table'] / (64 * m):.4f}); share_map default {ms['default'][0]:.3f} table {ms['table'][0]:.3f} ms; "
          f"lstm0 default {ms['default'][1]:.3f} table {ms['table'][1]:.3f} ms")


def run(leg):
    _lib.set_option("encoder_dedup_off", 1 if leg == "off" else 0)
    eng.profile(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        eng.encoder(feat, want_align=False, **LEGS[leg])
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


for leg in LEGS:        # warm each
    run(leg)
for r in range(ROUNDS):
    for leg in LEGS:
        ms, st = run(leg)
        print(f"round {r} {leg}: {ms:.3f} ms per step  lstm0 {st.get('lstm0')}  share_map {st.get('share_map')}  stages {st}")
