"""Regenerates tests/golden/score_criterion.npz: small seeded rows and what the reference's own PLoss / MLoss
(speech_anime/model/criterion.py) return for them in float32, called the way get_loss (speech_anime/model/model.py:261-330)
calls them, on the batch [a; b] collated from one clip as the validation set does (datasets/sliding_window.py:66-76).
tests/test_score_ref64_cpu.py pins tests/score_ref64.py to it.

    python -B tests/gen_golden_score.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import score_ref64 as R  # noqa: E402

CASES = {           # name -> (layout, frames, W, seed, weights seed or None)
    "dgrad_ones": ("dgrad", 7, 45, 21, None),
    "dgrad_weighted": ("dgrad", 7, 45, 22, 5),
    "dgrad_two_frames": ("dgrad", 2, 45, 23, 6),
    "plain_ones": ("plain", 6, 11, 24, None),
    "plain_weighted": ("plain", 9, 11, 25, 7),
}


def inputs(name):
    layout, fc, W, seed, wseed = CASES[name]
    truth = R.tracks(fc, W, seed, 0.3)
    pred = (truth + R.tracks(fc, W, seed + 100, 0.1)).astype(np.float32)
    weights = np.ones(fc, np.float32) if wseed is None else np.random.RandomState(wseed).uniform(0.2, 2.0, fc).astype(np.float32)
    return layout, pred, truth, weights


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch
    out = {}
    for head, layout_of in (("dgrad", "dgrad"), ("offsets", "plain")):
        hp, _, _ = ref_import.load_reference(head)
        from speech_anime.model import criterion
        ploss, mloss = criterion.PLoss(hp), criterion.MLoss(hp)
        for name in CASES:
            layout, pred, truth, weights = inputs(name)
            if layout != layout_of:
                continue
            a, b = R.collate(pred.shape[0])
            idx = np.concatenate((a, b))
            P, T, wt = torch.from_numpy(pred[idx]), torch.from_numpy(truth[idx]), torch.from_numpy(weights[idx])
            got = {}
            if layout == "dgrad":
                tri = lambda x: x.view(x.shape[0], 1, -1, 9)      # noqa: E731
                for tag, sl in (("s", slice(0, 6)), ("r", slice(6, 9))):
                    got["scalar_p" + tag] = float(ploss(tri(P)[..., sl], tri(T)[..., sl], wt).mean().item())
                    got["scalar_m" + tag] = float(mloss(tri(P)[..., sl], tri(T)[..., sl], wt).mean().item())
                got["scalar_ploss"] = got["scalar_ps"] + got["scalar_pr"]
                got["scalar_mloss"] = got["scalar_ms"] + got["scalar_mr"]
            else:
                got["scalar_ploss"] = float(ploss(P.view(P.shape[0], 1, -1), T.view(T.shape[0], 1, -1), wt).mean().item())
                got["scalar_mloss"] = float(mloss(P.view(P.shape[0], 1, -1), T.view(T.shape[0], 1, -1), wt).mean().item())
            out[name + ".pred"], out[name + ".truth"], out[name + ".weights"] = pred, truth, weights
            for k, v in got.items():
                out[f"{name}.{k}"] = np.float64(v)
    path = os.path.join(HERE, "golden", "score_criterion.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: float(v) for k, v in out.items() if "scalar" in k})


if __name__ == "__main__":
    main()
