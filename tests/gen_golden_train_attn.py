"""Regenerates tests/golden/train_attn.npz, train_attn_dH.npz (the one full dH, half a megabyte on its own: each committed file
stays under 1 MiB) and META_train_attn.json: what the reference's own BahdanauAttention
(speech_anime/layers/attentions.py; layer 10 of the audio encoder as speech_anime/layers builds it from config/model/dgrad.py),
called as layers/__init__.py calls it (query = H[:, 31:34], key = H, training mode), torch.autograd and
torch.optim.Adam(lr=1e-4, weight_decay=0) make of the seeded cases of tests/attntrain_ref64.py: loss = (z * dz).sum() backward,
then three Adam steps on the same batch, once in float32 as the reference runs and once with the layer and the inputs cast to
double.  Results only: the weights are regenerated from the seed.  z, align and the v / b gradients, one-step and three-step
values are stored in full; dH in full for the double run of the peaked N = 2 case, and its steps 0, 30 .. 34, 63 for both runs of the flat
one; of the
dWc, dWk, dWq gradients every 37th row (dWc as [512][1536]: the peaked N = 2 case only) plus the double run's row and column
sums in double; of their three-step values the double run's row sums.
tests/test_attntrain_ref64_cpu.py pins tests/attntrain_ref64.py to it.

    python -B tests/gen_golden_train_attn.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attntrain_ref64 as R  # noqa: E402

CASES = {           # name -> (N, seed, family)
    "flat_n2": (2, 51, "flat"),
    "peaked_n2": (2, 52, "peaked"),
    "peaked_n5": (5, 53, "peaked"),
}
FULL_DH = "peaked_n2"
STEPS_DH = "flat_n2"
DH_STEPS = (0, 30, 31, 32, 33, 34, 63)
ROW_STRIDE = 37
STEPS = 3
MATRICES = (R.WC, R.WK, R.WQ)


def inputs(name):
    return R.case(*CASES[name])


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch

    out, meta = {}, {"cases": {k: list(v) for k, v in CASES.items()}, "row_stride": ROW_STRIDE, "steps": STEPS, "lr": 1e-4,
                     "full_dH": FULL_DH, "dH_steps": list(DH_STEPS)}
    short = len(R.P)

    def put_matrix(key, name, a, npdt, rows, sums):
        a2 = np.asarray(a).reshape(a.shape[0], -1)
        if npdt is np.float64 and sums:
            out[key + ".rowsum"] = a2.astype(np.float64).sum(1)
            if rows is not None:
                out[key + ".colsum"] = a2.astype(np.float64).sum(0)
        if rows:
            out[key + ".rows"] = np.asarray(a2, npdt)[::ROW_STRIDE]

    for name, (N, seed, family) in CASES.items():
        c = inputs(name)
        for tag, dtype, npdt in (("f32", torch.float32, np.float32), ("f64", torch.float64, np.float64)):
            hp, model, _ = ref_import.load_reference("dgrad")
            att = model._model._audio_encoder._layers[10].to(dtype).train()
            assert type(att).__name__ == "BahdanauAttention", type(att)
            named = dict(att.named_parameters())
            assert sorted(named) == sorted(k[short:] for k in c["params"]), sorted(named)
            with torch.no_grad():
                for k, v in c["params"].items():
                    named[k[short:]].copy_(torch.from_numpy(v).to(dtype))
            H = torch.from_numpy(c["H"]).to(dtype).requires_grad_(True)
            dz = torch.from_numpy(c["dz"]).to(dtype)
            opt = torch.optim.Adam(att.parameters(), lr=1e-4, weight_decay=0)
            for step in range(STEPS):
                opt.zero_grad()
                H.grad = None
                z, align = att(query=H[:, R.W0:R.W0 + R.KW], key=H)
                (z.view(N, -1) * dz).sum().backward()
                if step == 0:
                    pre = f"{name}.{tag}"
                    out[pre + ".z"] = z.detach().numpy().astype(npdt).reshape(N, R.D)
                    out[pre + ".align"] = align.detach().numpy().astype(npdt).reshape(N, R.TS)
                    dH = H.grad.numpy().astype(npdt)
                    if name == FULL_DH and tag == "f64":
                        out[pre + ".dH"] = dH
                    elif name == STEPS_DH:
                        out[pre + ".dH.steps"] = dH[:, list(DH_STEPS)]
                    for k in c["params"]:
                        g = named[k[short:]].grad.numpy()
                        if k in MATRICES:
                            put_matrix(f"{pre}.grad.{k}", k, g, npdt, rows=(k != R.WC or name == FULL_DH), sums=True)
                        else:
                            out[f"{pre}.grad.{k}"] = g.astype(npdt)
                opt.step()
                if step == 0:
                    for k in (R.V, R.B):
                        out[f"{name}.{tag}.param1.{k}"] = named[k[short:]].detach().numpy().astype(npdt)
            for k in c["params"]:
                p = named[k[short:]].detach().numpy()
                if k in MATRICES:
                    put_matrix(f"{name}.{tag}.param{STEPS}.{k}", k, p, npdt, rows=None, sums=True)
                else:
                    out[f"{name}.{tag}.param{STEPS}.{k}"] = p.astype(npdt)
        meta.setdefault("torch", torch.__version__)

    path = os.path.join(HERE, "golden", "train_attn.npz")
    full = f"{FULL_DH}.f64.dH"
    np.savez_compressed(os.path.join(HERE, "golden", "train_attn_dH.npz"), **{full: out.pop(full)})
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "golden", "META_train_attn.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
