"""Regenerates tests/golden/train_freq.npz, train_freq_dC.npz, train_freq_sums.npz, train_freq_rows32.npz, train_freq_rows64.npz
(each committed file stays under 1 MiB) and META_train_freq.json: what the reference's own FreqLstm (layer 6 of the audio encoder
as speech_anime/layers builds it from config/model/dgrad.py: a bidirectional torch.nn.LSTM(64, 128, bias=True) along the 32
frequency bins and a Linear(8192, 256) with bias), torch.autograd and torch.optim.Adam(lr=1e-4, weight_decay=0) make of the
seeded cases of tests/freqtrain_ref64.py: loss = (X0 * dX0).sum() backward, then three Adam steps on the same batch, once in
float32 as the reference runs and once with the module and the inputs cast to double.  The module is driven through its own
forward: the case's C [R][32][64] enters as the (B, C, F, T) tensor [1][64][32][R], which FreqLstm.forward permutes back, and
X0 [R][256] leaves as (1, 256, 1, R).  Results only: the weights are regenerated from the seed.  Stored: X0 in full, dC at the
steps 0, 1, 15, 30, 31, the bias tensors' gradients and one- and three-step parameters in full, for both runs; of every weight
gradient and three-step weight the double run's row and column sums; of every weight gradient sampled rows (every 37th, every
85th of _proj.weight) for the float32 run and, in the forget-bias case of one frame, for the double run together with the same
rows of the one-step parameters.  tests/test_freqtrain_ref64_cpu.py pins tests/freqtrain_ref64.py to it.

    python -B tests/gen_golden_train_freq.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import freqtrain_ref64 as R  # noqa: E402

CASES = {           # name -> (R, seed, family)
    "default_r64": (64, 71, "default"),       # one frame, default-scale weights
    "carry_r64": (64, 72, "carry"),           # one frame, the forget gate open: the 32-step carry matters
    "carry_r5": (5, 73, "carry"),             # a small odd R
    "default_r7": (7, 74, "default"),
}
FULL = "carry_r64"
C_STEPS = (0, 1, 15, 30, 31)
ROW_STRIDE, WP_ROW_STRIDE = 37, 85
STEPS = 3
FILES = ("train_freq", "train_freq_dC", "train_freq_sums", "train_freq_rows32", "train_freq_rows64")


def inputs(name):
    return R.case(*CASES[name])


def row_stride(name):
    return WP_ROW_STRIDE if name.endswith("_proj.weight") else ROW_STRIDE


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch

    out = {f: {} for f in FILES}
    meta = {"cases": {k: list(v) for k, v in CASES.items()}, "row_stride": ROW_STRIDE, "wp_row_stride": WP_ROW_STRIDE, "steps": STEPS,
            "lr": 1e-4, "full": FULL, "C_steps": list(C_STEPS)}
    short = len(R.P)
    for name, (rows, seed, family) in CASES.items():
        c = inputs(name)
        for tag, dtype, npdt in (("f32", torch.float32, np.float32), ("f64", torch.float64, np.float64)):
            hp, model, _ = ref_import.load_reference("dgrad")
            mod = model._model._audio_encoder._layers[6]
            assert type(mod).__name__ == "FreqLstm" and type(mod._lstm) is torch.nn.LSTM, mod
            lstm = mod._lstm
            assert (lstm.input_size, lstm.hidden_size, lstm.num_layers, lstm.bidirectional, lstm.bias, lstm.batch_first) == (64, 128, 1, True, True, True), lstm
            mod = mod.to(dtype).train()
            named = dict(mod.named_parameters())
            assert sorted(named) == sorted(k[short:] for k in c["params"]), sorted(named)
            assert {k[short:]: tuple(named[k[short:]].shape) for k in c["params"]} == {k[short:]: s for k, s in R.shapes().items()}
            with torch.no_grad():
                for k, v in c["params"].items():
                    named[k[short:]].copy_(torch.from_numpy(v).to(dtype))
            C = torch.from_numpy(c["C"]).to(dtype).requires_grad_(True)               # [R][32 f][64 ch]
            dX0 = torch.from_numpy(c["dX0"]).to(dtype)
            opt = torch.optim.Adam(mod.parameters(), lr=1e-4, weight_decay=0)
            pre = f"{name}.{tag}"
            for step in range(STEPS):
                opt.zero_grad()
                C.grad = None
                y = mod(C.permute(2, 1, 0).unsqueeze(0))                                # (1, 64 ch, 32 f, R) -> (1, 256, 1, R)
                assert tuple(y.shape) == (1, R.NO, 1, rows), y.shape
                X0 = y[0, :, 0, :].t()
                (X0 * dX0).sum().backward()
                if step == 0:
                    out["train_freq"][pre + ".X0"] = X0.detach().numpy().astype(npdt)
                    out["train_freq_dC"][pre + ".dC.steps"] = C.grad.numpy().astype(npdt)[:, list(C_STEPS)]
                    for k in c["params"]:
                        g = named[k[short:]].grad.numpy()
                        if g.ndim == 1:
                            out["train_freq"][f"{pre}.grad.{k}"] = g.astype(npdt)
                            continue
                        if tag == "f64":
                            out["train_freq_sums"][f"{pre}.grad.{k}.rowsum"] = g.astype(np.float64).sum(1)
                            out["train_freq_sums"][f"{pre}.grad.{k}.colsum"] = g.astype(np.float64).sum(0)
                            if name == FULL:
                                out["train_freq_rows64"][f"{pre}.grad.{k}.rows"] = g[::row_stride(k)].astype(npdt)
                        elif name != FULL:
                            out["train_freq_rows32"][f"{pre}.grad.{k}.rows"] = g[::row_stride(k)].astype(npdt)
                opt.step()
                if step == 0:
                    for k in c["params"]:
                        w = named[k[short:]].detach().numpy()
                        if w.ndim == 1:
                            out["train_freq"][f"{pre}.param1.{k}"] = w.astype(npdt)
                        elif name == FULL and tag == "f64":
                            out["train_freq_rows64"][f"{pre}.param1.{k}.rows"] = w[::row_stride(k)].astype(npdt)
            if tag == "f64":
                for k in c["params"]:
                    w = named[k[short:]].detach().numpy().astype(np.float64)
                    if w.ndim == 1:
                        out["train_freq"][f"{pre}.param{STEPS}.{k}"] = w
                    else:
                        out["train_freq_sums"][f"{pre}.param{STEPS}.{k}.rowsum"] = w.sum(1)
        meta.setdefault("torch", torch.__version__)

    for f in FILES:
        path = os.path.join(HERE, "golden", f + ".npz")
        np.savez_compressed(path, **out[f])
        print(path, os.path.getsize(path), "bytes,", len(out[f]), "arrays")
        assert os.path.getsize(path) < 1 << 20, path
    with open(os.path.join(HERE, "golden", "META_train_freq.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
