"""Regenerates tests/golden/train_lstm.npz, train_lstm_full.npz, train_lstm_rows32.npz, train_lstm_rows64.npz (each committed file
stays under 1 MiB) and META_train_lstm.json: what the reference's own BiLSTM (layer 9 of the audio encoder as speech_anime/layers
builds it from config/model/dgrad.py: torch.nn.LSTM(256, 256, num_layers=2, bias=False, bidirectional=True)), with its `dropout`
attribute set to 0.0 and in training mode, torch.autograd and torch.optim.Adam(lr=1e-4, weight_decay=0) make of the seeded
two-layer cases of tests/lstmtrain_ref64.py: loss = (H * dH).sum() backward, then three Adam steps on the same batch, once in
float32 as the reference runs and once with the layer and the inputs cast to double.  Results only: the weights are regenerated
from the seed.  Stored: H and dX0 at the steps 0, 1, 31, 62, 63 for both runs, and in full for the double run of the carry
N = 2 case; of every weight gradient the double run's row and column sums, every 37th row for the float32 run of the other
cases and for the double run of the carry N = 2 case; of the one-step parameters every 37th row of the layer-1 recurrent
weights (double run, carry N = 2); of the three-step parameters the double run's row sums.
tests/test_lstmtrain_ref64_cpu.py pins tests/lstmtrain_ref64.py to it.

    python -B tests/gen_golden_train_lstm.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lstmtrain_ref64 as R  # noqa: E402

CASES = {           # name -> (N, seed, family)
    "default_n2": (2, 61, "default"),
    "carry_n2": (2, 62, "carry"),
    "carry_n3": (3, 63, "carry"),
}
FULL = "carry_n2"
H_STEPS = (0, 1, 31, 62, 63)
ROW_STRIDE = 37
STEPS = 3
PARAM1 = R.names(1)[2:]
FILES = ("train_lstm", "train_lstm_full", "train_lstm_rows32", "train_lstm_rows64")


def inputs(name):
    return R.stack_case(*CASES[name])


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch

    out = {f: {} for f in FILES}
    meta = {"cases": {k: list(v) for k, v in CASES.items()}, "row_stride": ROW_STRIDE, "steps": STEPS, "lr": 1e-4, "full": FULL,
            "H_steps": list(H_STEPS)}
    short = len(R.P)
    for name, (N, seed, family) in CASES.items():
        c = inputs(name)
        for tag, dtype, npdt in (("f32", torch.float32, np.float32), ("f64", torch.float64, np.float64)):
            hp, model, _ = ref_import.load_reference("dgrad")
            rnn = model._model._audio_encoder._layers[9]
            assert type(rnn) is torch.nn.LSTM and rnn.num_layers == 2 and rnn.bidirectional and not rnn.bias and rnn.batch_first, rnn
            meta["reference_dropout"] = float(rnn.dropout)
            rnn.dropout = 0.0
            rnn = rnn.to(dtype).train()
            named = dict(rnn.named_parameters())
            assert sorted(named) == sorted(k[short:] for k in c["params"]), sorted(named)
            with torch.no_grad():
                for k, v in c["params"].items():
                    named[k[short:]].copy_(torch.from_numpy(v).to(dtype))
            X = torch.from_numpy(c["X"]).to(dtype).requires_grad_(True)
            dY = torch.from_numpy(c["dY"]).to(dtype)
            opt = torch.optim.Adam(rnn.parameters(), lr=1e-4, weight_decay=0)
            pre = f"{name}.{tag}"
            for step in range(STEPS):
                opt.zero_grad()
                X.grad = None
                H, _ = rnn(X)
                (H * dY).sum().backward()
                if step == 0:
                    Hn, dX0 = H.detach().numpy().astype(npdt), X.grad.numpy().astype(npdt)
                    out["train_lstm"][pre + ".H.steps"] = Hn[:, list(H_STEPS)]
                    out["train_lstm"][pre + ".dX0.steps"] = dX0[:, list(H_STEPS)]
                    if name == FULL and tag == "f64":
                        out["train_lstm_full"][pre + ".H"] = Hn
                        out["train_lstm_full"][pre + ".dX0"] = dX0
                    for k in c["params"]:
                        g = named[k[short:]].grad.numpy()
                        if tag == "f64":
                            out["train_lstm"][f"{pre}.grad.{k}.rowsum"] = g.astype(np.float64).sum(1)
                            out["train_lstm"][f"{pre}.grad.{k}.colsum"] = g.astype(np.float64).sum(0)
                            if name == FULL:
                                out["train_lstm_rows64"][f"{pre}.grad.{k}.rows"] = g[::ROW_STRIDE].astype(npdt)
                        elif name != FULL:
                            out["train_lstm_rows32"][f"{pre}.grad.{k}.rows"] = g[::ROW_STRIDE].astype(npdt)
                opt.step()
                if step == 0 and name == FULL and tag == "f64":
                    for k in PARAM1:
                        out["train_lstm_rows64"][f"{pre}.param1.{k}.rows"] = named[k[short:]].detach().numpy()[::ROW_STRIDE].astype(npdt)
            if tag == "f64":
                for k in c["params"]:
                    out["train_lstm"][f"{pre}.param{STEPS}.{k}.rowsum"] = named[k[short:]].detach().numpy().astype(np.float64).sum(1)
        meta.setdefault("torch", torch.__version__)

    for f in FILES:
        path = os.path.join(HERE, "golden", f + ".npz")
        np.savez_compressed(path, **out[f])
        print(path, os.path.getsize(path), "bytes,", len(out[f]), "arrays")
        assert os.path.getsize(path) < 1 << 20, path
    with open(os.path.join(HERE, "golden", "META_train_lstm.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
