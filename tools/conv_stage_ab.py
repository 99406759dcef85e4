"""conv23 and pca stage times per precision mode: Engine.profile at 8,192 frames of torch.rand features (identity share map), three
rounds of five calls.  For A/B runs of two builds of the library, alternate processes:
    python tools/conv_stage_ab.py new_1 [modes...]; SDFA_HIP_LIB=old.so python tools/conv_stage_ab.py parent_1 [modes...]; ..."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
import torch
from sdfa_amd import synth
from sdfa_amd.engine import Engine

tag = sys.argv[1]
N, REPS, ROUNDS = 8192, 5, 3
feat = torch.rand((N, 64, 128, 3), generator=torch.Generator().manual_seed(1)).cuda()
spk = torch.arange(N) % 8
sd = synth.make_state_dict("dgrad", 1234)
for prec in (sys.argv[2:] or ("fp32", "bf16x3", "bf16x6", "bf16")):
    eng = Engine(sd, max_frames=N, precision=prec)
    out = torch.empty((N, eng.out_dim), dtype=torch.float32, device='cuda')
    z, _ = eng.encoder(feat, want_align=False); eng.regress(z, spk, out=out)      # warm
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        eng.profile(True)
        for _ in range(REPS):
            z, _ = eng.encoder(feat, want_align=False)
            eng.regress(z, spk, out=out)
        torch.cuda.synchronize()
        st = {}
        for k in ("conv23", "pca"):
            st[k] = round(eng.profile_ms(k) / REPS, 4)
        eng.profile(False)
        print(f"[{tag}] {prec} round {r}: conv23 {st['conv23']:.4f} ms  pca {st['pca']:.4f} ms per 8192-frame call", flush=True)
    del eng, out
