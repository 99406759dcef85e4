"""Chunks whose columns all meet on one slot of the encoder scan's hash table: Engine.encoder on all-zero features (700 and 8,192 frames),
and 8,192 frames of torch.rand features for comparison.  One warm call, then the share_map stage per call over 5 calls and the number of
distinct columns (profiles/encoder_group_ab.txt)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
import torch
from sdfa_amd import synth
from sdfa_amd.engine import Engine
eng = Engine(synth.make_state_dict("dgrad", 1234), max_frames=8192)
for name, feat in (("zeros700", torch.zeros((700, 64, 128, 3), device="cuda")), ("zeros8192", torch.zeros((8192, 64, 128, 3), device="cuda")),
                   ("rand8192", torch.rand((8192, 64, 128, 3), device="cuda"))):
    eng.encoder(feat, want_align=False)
    eng.profile(True)
    for _ in range(5):
        eng.encoder(feat, want_align=False)
    torch.cuda.synchronize()
    print(f"{name}: share_map {eng.profile_ms('share_map') / 5:.4f} ms per call, distinct {eng.distinct_columns(feat.shape[0])}")
    eng.profile(False)
