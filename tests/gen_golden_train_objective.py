"""Regenerates tests/golden/train_objective.npz and META_train_objective.json: small seeded batches [a; b] of PCA coefficients
and what the reference's own PcaInversion (speech_anime/modules/output_module.py), PLoss, MLoss and DynamicLossScaler
(speech_anime/model/criterion.py) and torch.autograd make of them, called the way get_loss (speech_anime/model/model.py:261-330)
calls them: the four losses and d loss_i / d coef, each separately, once in float32 as the reference runs and once with the
modules and inputs cast to double; and a DynamicLossScaler's state over three training steps and one eval step.
tests/test_objective_ref64_cpu.py pins tests/objective_ref64.py and sdfa_amd.objective.DynamicLossScaler to it.  Results only.

    python -B tests/gen_golden_train_objective.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import objective_ref64 as R  # noqa: E402

CASES = {           # name -> (layout, T | W, Ks, Kr, B, seed, weights, coefficient scale)
    "dgrad_unit": ("dgrad", 5, 4, 7, 3, 31, "unit", 15.0),
    "dgrad_weighted": ("dgrad", 5, 4, 7, 3, 32, "uniform", 15.0),
    "plain_weighted": ("plain", 11, 3, 0, 4, 33, "uniform", 15.0),
    "dgrad_one_pair": ("dgrad", 5, 4, 7, 1, 34, "uniform", 15.0),
}
SCALER_STEPS = (1.0, 0.9, 0.8, 0.7)     # the coefficients of dgrad_weighted times these: three training steps, one eval step


def inputs(name):
    return R.case(*CASES[name])


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch
    out, meta = {}, {"cases": {k: list(v) for k, v in CASES.items()}, "scaler_steps": list(SCALER_STEPS), "max_abs_rotat_argument": {}}
    mods = {}
    for head in ("dgrad", "offsets"):
        hp, _, _ = ref_import.load_reference(head)
        from speech_anime.model import criterion
        mods[head] = (criterion.PLoss(hp), criterion.MLoss(hp))
    from speech_anime.model.criterion import DynamicLossScaler
    from speech_anime.modules.output_module import PcaInversion

    def run(c, dtype, scale=1.0):
        """[(loss, d loss / d coef)] in the order ps, ms, pr, mr (plain: ploss, mloss)"""
        layout, b = c["layout"], c["bases"]
        ploss, mloss = mods["dgrad" if layout == "dgrad" else "offsets"]
        coef = (torch.from_numpy(c["coef"]).to(dtype) * scale).requires_grad_(True)
        truth, wt = torch.from_numpy(c["truth"]).to(dtype), torch.from_numpy(c["weight"]).to(dtype)
        N = coef.shape[0]
        res = []
        if layout == "dgrad":
            ks = b["compT_s"].shape[1]
            inv_s = PcaInversion(b["compT_s"], b["means_s"], False, ks, b["compT_s"].shape[0], True).to(dtype)
            inv_r = PcaInversion(b["compT_r"], b["means_r"], False, b["compT_r"].shape[1], b["compT_r"].shape[0], True).to(dtype)
            pred = (inv_s(coef[:, :ks]).view(N, 1, -1, 6), inv_r(coef[:, ks:]).view(N, 1, -1, 3))
            tri = truth.view(N, 1, -1, 9)
            true = (tri[..., :6], tri[..., 6:])
            rot_max = float(pred[1].detach().abs().max())
            for p, t in zip(pred, true):
                for fn in (ploss, mloss):
                    res.append(fn(p, t, wt))
        else:
            inv = PcaInversion(b["compT_s"], b["means_s"], False, b["compT_s"].shape[1], b["compT_s"].shape[0], True).to(dtype)
            pred = inv(coef).view(N, 1, -1)
            rot_max = 0.0
            for fn in (ploss, mloss):
                res.append(fn(pred, truth.view(N, 1, -1), wt))
        grads = [torch.autograd.grad(l, coef, retain_graph=True)[0] for l in res]
        return res, grads, rot_max

    for name in CASES:
        c = inputs(name)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            res, grads, rot_max = run(c, dtype)
            out[f"{name}.{tag}.loss"] = np.asarray([float(l.detach()) for l in res], np.float64)
            out[f"{name}.{tag}.grad"] = np.stack([g.numpy().astype(np.float64) for g in grads])
        assert rot_max <= 3.0, (name, rot_max)
        meta["max_abs_rotat_argument"][name] = rot_max

    # the scaler: criterion.DynamicLossScaler on the float32 ps of dgrad_weighted at scaled coefficients
    c = inputs("dgrad_weighted")
    sc = DynamicLossScaler()
    rows = []
    for step, s in enumerate(SCALER_STEPS):
        res, _, _ = run(c, torch.float32, s)
        training = step < len(SCALER_STEPS) - 1
        scaled = sc.scale_loss(res[0], training)
        rows.append([float(res[0].detach()), float(training), sc.vt, sc.beta_t, sc.scale, float(scaled.detach())])
    out["scaler.rows"] = np.asarray(rows, np.float64)        # loss (a float32 value), training, vt, beta_t, scale, scaled loss
    meta["scaler_columns"] = ["loss", "training", "vt", "beta_t", "scale", "scaled_loss"]
    meta["torch"] = torch.__version__

    path = os.path.join(HERE, "golden", "train_objective.npz")
    np.savez(path, **out)
    with open(os.path.join(HERE, "golden", "META_train_objective.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", {k: v.tolist() for k, v in out.items() if k.endswith(".loss")})


if __name__ == "__main__":
    main()
