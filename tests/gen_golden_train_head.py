"""Regenerates tests/golden/train_head.npz and META_train_head.json: what the reference's own output-module layers
(speech_anime/modules/output_module.py, built by speech_anime/layers from config/model/{dgrad,offsets}.py, each under
torch.nn.utils.weight_norm), its SpeakerEmbedding, torch.autograd and torch.optim.Adam(lr=1e-4, weight_decay=0) make of the
seeded cases of tests/headtrain_ref64.py: loss = (coef * dcoef).sum() backward, then three Adam steps on the same batch, once
in float32 as the reference runs and once with the layers and inputs cast to double.  Results only: the weights are
regenerated from the seed.  coef, dz and the weight_g / bias gradients and three-step values are stored in full; of the
weight_v gradients every 37th row (both runs, B = 3) and the double run's row and column sums in double; of the three-step
weight_v the double run's row sums; the B = 1 cases keep no three-step weight_g / bias (a committed file stays under 1 MiB).  tests/test_headtrain_ref64_cpu.py pins tests/headtrain_ref64.py to it.

    python -B tests/gen_golden_train_head.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headtrain_ref64 as R  # noqa: E402

CASES = {           # name -> (head, B, seed, speakers): mixed speakers, speaker 5 absent
    "dgrad_b1": ("dgrad", 1, 41, (0, 1, 2, 3, 4, 6, 7)),
    "dgrad_b3": ("dgrad", 3, 42, (0, 1, 2, 3, 4, 6, 7)),
    "offsets_b1": ("offsets", 1, 43, (0, 1, 2, 3, 4, 6, 7)),
    "offsets_b3": ("offsets", 3, 44, (0, 1, 2, 3, 4, 6, 7)),
}
ROW_STRIDE = 37
STEPS = 3


def inputs(name):
    return R.case(*CASES[name])


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch
    ref_import.install_stubs()
    from speech_anime import layers

    out, meta = {}, {"cases": {k: list(v) for k, v in CASES.items()}, "row_stride": ROW_STRIDE, "steps": STEPS, "lr": 1e-4}

    def put(key, a, npdt, B, kind):
        """kind "full": stored whole.  Otherwise a [P][K] weight_v quantity: the double run keeps its row sums in double; kind
        "rows" also keeps the column sums and every 37th row of the B = 3 cases.  The float32 run of a B = 1 case keeps coef
        and dz only."""
        a64 = np.asarray(a, np.float64)
        f64 = npdt is np.float64
        if kind == "full":
            out[key] = np.asarray(a, npdt).reshape(a64.shape)
            return
        if f64:
            out[key + ".rowsum"] = a64.sum(1)
            if B == 3 and kind == "rows":
                out[key + ".colsum"] = a64.sum(0)
        if kind == "rows" and B == 3:
            out[key + ".rows"] = np.asarray(a, npdt)[::ROW_STRIDE]

    for name, (head, B, seed, speakers) in CASES.items():
        c = inputs(name)
        for tag, dtype, npdt in (("f32", torch.float32, np.float32), ("f64", torch.float64, np.float64)):
            hp, model, _ = ref_import.load_reference(head)
            net = model._model
            om, emb = net._output_module.to(dtype).train(), net._speaker_embedding
            named = dict(om.named_parameters())
            with torch.no_grad():
                for k, v in c["params"].items():
                    named[k[len("_output_module."):]].copy_(torch.from_numpy(v).to(dtype))
            assert len(named) == len(c["params"])

            def forward(z, cond):
                x = z.view(len(z), 1, -1)
                kw = dict(training=True, condition=cond)
                x = layers.forward("output", x, layers=om._layers, parsers=om._parsers, **kw)
                if head == "dgrad":
                    xs = layers.forward("output-scale", x, layers=om._scale_layers, parsers=om._scale_parsers, **kw)
                    xr = layers.forward("output-rotat", x, layers=om._rotat_layers, parsers=om._rotat_parsers, **kw)
                    x = torch.cat((xs, xr), -1)
                return x.view(len(z), -1)

            z = torch.from_numpy(c["z"]).to(dtype).requires_grad_(True)
            cond = emb(torch.from_numpy(c["sid"])).to(dtype)
            dcoef = torch.from_numpy(c["dcoef"]).to(dtype)
            opt = torch.optim.Adam(om.parameters(), lr=1e-4, weight_decay=0)
            for step in range(STEPS):
                opt.zero_grad()
                z.grad = None
                coef = forward(z, cond)
                (coef * dcoef).sum().backward()
                if step == 0:
                    put(f"{name}.{tag}.coef", coef.detach().numpy(), npdt, B, "full")
                    put(f"{name}.{tag}.dz", z.grad.numpy(), npdt, B, "full")
                    for k in c["params"]:
                        if k.endswith("weight_v"):
                            put(f"{name}.{tag}.grad.{k}", named[k[len('_output_module.'):]].grad.numpy(), npdt, B, "rows")
                        elif B == 3 or tag == "f64":
                            put(f"{name}.{tag}.grad.{k}", named[k[len('_output_module.'):]].grad.numpy(), npdt, B, "full")
                opt.step()
            for k in c["params"]:
                if k.endswith("weight_v"):
                    put(f"{name}.{tag}.param{STEPS}.{k}", named[k[len("_output_module."):]].detach().numpy(), npdt, B, "sums")
                elif B == 3:
                    put(f"{name}.{tag}.param{STEPS}.{k}", named[k[len("_output_module."):]].detach().numpy(), npdt, B, "full")
        meta.setdefault("torch", torch.__version__)

    path = os.path.join(HERE, "golden", "train_head.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "golden", "META_train_head.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
