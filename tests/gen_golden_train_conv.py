"""Regenerates tests/golden/train_conv_f32.npz, train_conv_f64_<case>.npz (each committed file stays under 1 MiB) and
META_train_conv.json: what the reference's own conv stack (layers 1 to 5 of the audio encoder as speech_anime/layers builds them
from config/model/dgrad.py: three weight-normed Conv2d along frequency, each with LeakyReLU(0.2) and then BatchNorm2d(eps=1e-3)
behind it, and two MaxPool2d((2, 1))), torch.autograd and torch.optim.Adam(lr=1e-4, weight_decay=0) make of the seeded cases of
tests/convtrain_ref64.py: loss = (C * dC).sum() backward, then three Adam steps on the same batch, once in float32 as the reference
runs and once with the modules and the inputs cast to double.  The modules are in eval(): the statistics are frozen (the inference
form; train() mode, batch statistics and moving running ones, is not what the trainer builds).  They are driven through their own
forward: the case's feat [R][128][3] enters as the (B, C, F, T) tensor [1][3][128][R] the encoder's Permute makes, and C [R][32][64]
leaves as (1, 64, 32, R).  Results only: the weights are regenerated from the seed.  Stored: C at the frequency rows 0, 1, 15, 30,
31; every gradient and every one-step parameter in full for both runs (the largest tensor has 6,144 elements); the three-step
parameters of the double run.  tests/test_convtrain_ref64_cpu.py pins tests/convtrain_ref64.py to it.

    python -B tests/gen_golden_train_conv.py          (needs the reference checkout; imported through oracle/ref_import.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import convtrain_ref64 as R  # noqa: E402

CASES = {           # name -> (R, seed, family)
    "default_r64": (64, 81, "default"),       # one frame
    "edge_r64": (64, 82, "edge"),             # one frame of the edge family
    "edge_r5": (5, 83, "edge"),               # a small odd R
    "default_r7": (7, 84, "default"),
}
C_ROWS = (0, 1, 15, 30, 31)
STEPS = 3
FILES = ("train_conv_f32",) + tuple(f"train_conv_f64_{name}" for name in CASES)


def inputs(name):
    return R.case(*CASES[name])


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import ref_import
    import torch

    out = {f: {} for f in FILES}
    meta = {"cases": {k: list(v) for k, v in CASES.items()}, "steps": STEPS, "lr": 1e-4, "C_rows": list(C_ROWS)}
    short = len(R.P)
    for name, (rows, seed, family) in CASES.items():
        c = inputs(name)
        for tag, dtype, npdt in (("f32", torch.float32, np.float32), ("f64", torch.float64, np.float64)):
            hp, model, _ = ref_import.load_reference("dgrad")
            layers = model._model._audio_encoder._layers
            assert [type(layers[i]).__name__ for i in range(1, 6)] == ["Conv2d", "Pool2d", "Conv2d", "Pool2d", "Conv2d"]
            stack = torch.nn.Sequential(*[layers[i] for i in range(1, 6)]).to(dtype).eval()
            named, buffers = {}, {}
            for L, co, ci, kf, pooled in R.LAYERS:
                conv = layers[L]
                assert isinstance(conv, torch.nn.Conv2d) and (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride) == (ci, co, (kf, 1), (1, 1))
                assert hasattr(conv, "weight_g") and hasattr(conv, "weight_v") and conv.bias is not None      # weight norm present
                bn, act = conv._ext_post_bn, conv._ext_post_act
                assert type(bn) is torch.nn.BatchNorm2d and bn.eps == 1e-3 and bn.affine and bn.track_running_stats and not bn.training
                assert type(act) is torch.nn.LeakyReLU and act.negative_slope == 0.2
                assert type(conv._ext_prev_act).__name__ == "Identity" and type(conv._ext_prev_bn).__name__ == "Identity"
                probe = torch.linspace(-2, 2, co * 6, dtype=dtype).reshape(1, co, 6, 1)
                with torch.no_grad():                          # LeakyReLU first, then BatchNorm
                    assert torch.equal(conv._ext_post_module(probe.clone()), bn(torch.nn.functional.leaky_relu(probe, 0.2)))
                if pooled:
                    pool = layers[L + 1]._pool
                    assert type(pool) is torch.nn.MaxPool2d and (pool.kernel_size, pool.stride, pool.padding, pool.ceil_mode) == ((2, 1), (2, 1), 0, False)
                for k, p in conv.named_parameters():
                    named[f"{R.P}{L}.{k}"] = p
                for k, b in conv.named_buffers():
                    buffers[f"{R.P}{L}.{k}"] = b
            assert sorted(named) == sorted(R.names()), sorted(named)
            assert {k: tuple(named[k].shape) for k in named} == {k: s for k, s in R.shapes().items() if k in named}
            with torch.no_grad():
                for k, v in c["params"].items():
                    (named[k] if k in named else buffers[k]).copy_(torch.from_numpy(v).to(dtype))
            feat = torch.from_numpy(c["feat"]).to(dtype)                                # [R][128 f][3 ch]
            dC = torch.from_numpy(c["dC"]).to(dtype)
            opt = torch.optim.Adam(list(named.values()), lr=1e-4, weight_decay=0)
            dst = out["train_conv_f32"] if tag == "f32" else out[f"train_conv_f64_{name}"]
            pre = f"{name}.{tag}"
            for step in range(STEPS):
                opt.zero_grad()
                y = stack(feat.permute(2, 1, 0).unsqueeze(0))                           # (1, 3 ch, 128 f, R) -> (1, 64, 32, R)
                assert tuple(y.shape) == (1, R.OUT, R.OUT_BINS, rows), y.shape
                Cx = y[0].permute(2, 1, 0)
                (Cx * dC).sum().backward()
                if step == 0:
                    dst[pre + ".C.rows"] = Cx.detach().numpy().astype(npdt)[:, list(C_ROWS)]
                    for k in named:
                        dst[f"{pre}.grad.{k[short:]}"] = named[k].grad.numpy().astype(npdt)
                opt.step()
                if step == 0:
                    for k in named:
                        dst[f"{pre}.param1.{k[short:]}"] = named[k].detach().numpy().astype(npdt)
            if tag == "f64":
                for k in named:
                    dst[f"{pre}.param{STEPS}.{k[short:]}"] = named[k].detach().numpy().astype(np.float64)
            for k, b in buffers.items():                       # eval(): the statistics did not move
                if k in c["params"]:
                    assert np.array_equal(b.numpy().astype(np.float32), c["params"][k]), k
        meta.setdefault("torch", torch.__version__)

    for f in FILES:
        path = os.path.join(HERE, "golden", f + ".npz")
        np.savez_compressed(path, **out[f])
        print(path, os.path.getsize(path), "bytes,", len(out[f]), "arrays")
        assert os.path.getsize(path) < 1 << 20, path
    with open(os.path.join(HERE, "golden", "META_train_conv.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
