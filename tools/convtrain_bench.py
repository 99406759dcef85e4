"""What training the conv stack costs on the MI355X: one ConvTrainer step -- forward, backward, Adam --
against the reference's route in torch in the same process (weight-normed Conv2d along frequency, leaky_relu, eval BatchNorm2d,
max_pool2d, autograd, torch.optim.Adam(lr=1e-4)) and against the bytes the step must move once at the copy rate measured in the
same run; and one whole training step of SaberSpeechDrivenAnimation -- train_step, the summed losses' backward, optimizer_step --
with + conv_stack next to + freq_lstm (the step before this section).  bench.py (the headline workload) is not involved.

  python tools/convtrain_bench.py --out profiles/convtrain_bench.json

Model     the synthetic offsets checkpoint (sdfa_amd.synth, seed 1234) and a two-clip synthetic TrainSet; a batch of N frames is
          DatasetSlidingWindow.train_batch of N / 2 seeded indices, built once per N and reused, so train_batch is not in the
          timed region.
Timed     by device events around --calls back-to-back calls after two warm-up calls; median of --reps windows (tools/
          bilstm_bench.py's `timed`).  A training step reads its four loss values back once (get_loss), so its time includes that
          synchronisation and the host work between the launches; the wall time of the same window is recorded next to it.
Trainer   ours: ConvTrainer with the checkpoint's tensors driven directly on seeded features and dC -- forward, backward, Adam, 11
          launches; forward and backward are also timed alone.  torch: the same tensors as leaf parameters, the stack as functional
          calls on the features viewed as (N, 3, 128, 64), zero_grad, forward, backward(dC), optimizer.step.  C must agree with
          torch's to its float32 round-off before anything is timed.
Floor     every buffer of the step written once and read once: the features read (96 KiB per frame), C written and dC read (512
          KiB each), the 6 MiB per frame of kept state written and read: 13.09 MiB per frame, at the rate a device-to-device copy
          of 1 GiB reaches in the same run (bytes read plus bytes written over its time).
Expected  fixed before the tool was run: step(+ conv_stack) - step(+ freq_lstm) = one conv-trainer step + the frequency trainer's
          dC tiles - sdfa_encoder_conv.  The dC tiles are 0.08 ms (N = 100) and 5.39 ms (N = 2,048) and sdfa_encoder_conv 0.13 and
          1.86 ms by section 21's table; the conv-trainer step is this run's.
Ones      of the products launch's 16 tiles per row block, 9 are bias and BatchNorm sums that keep one column of a 64 x 64 tile;
          by chain length they are 245,760 of 557,056 rows per column, 44 % of the launch.  The launch is not timed alone: the
          backward's time, which holds it, is the figure recorded.
Not here  hardware counters; a per-kernel split; the dgrad head; 8 kHz data."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bilstm_bench import make_model, timed, train_set  # noqa: E402

FREQ = dict(attention=True, bilstm_top=True, bilstm_bottom=True, freq_lstm=True)
CONFIGS = (("head+attention+top+bottom+freq_lstm", FREQ), ("head+attention+top+bottom+freq_lstm+conv_stack", dict(FREQ, conv_stack=True)))
DC_TILES_MS = {100: 0.08, 2048: 5.39}           # step with dC - step without
ENCODER_CONV_MS = {100: 0.13, 2048: 1.86}       # sdfa_encoder_conv
FLOOR_BYTES_PER_FRAME = 64 * 128 * 3 * 4 + 2 * 64 * 32 * 64 * 4 + 2 * 6 * 1024 * 1024


class TorchConv:
    """the reference's route: weight-normed Conv2d((kf, 1)) along frequency, LeakyReLU(0.2), BatchNorm2d(eps=1e-3) in eval, MaxPool2d((2, 1))"""

    def __init__(self, sd):
        import torch
        from sdfa_amd.convtrain import LAYERS, PREFIX
        self.layers = []
        get = lambda n: torch.as_tensor(sd["_model." + n] if "_model." + n in sd else sd[n]).float().cuda()
        for L, co, ci, kf in LAYERS:
            n = f"{PREFIX}{L}."
            p = {k: get(n + k).clone().requires_grad_(True) for k in ("weight_g", "weight_v", "bias", "_ext_post_bn.weight", "_ext_post_bn.bias")}
            c = {k: get(n + "_ext_post_bn." + k) for k in ("running_mean", "running_var")}
            self.layers.append((p, c, kf, L != 5))
        self.opt = torch.optim.Adam([t for p, _, _, _ in self.layers for t in p.values()], lr=1e-4, weight_decay=0)

    def forward(self, x):
        import torch
        import torch.nn.functional as F
        for p, c, kf, pooled in self.layers:
            v = p["weight_v"]
            W = p["weight_g"] * v / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1, 1)      # torch's weight_norm, dim 0
            x = F.conv2d(x, W, p["bias"], padding=(kf // 2, 0))
            x = F.leaky_relu(x, 0.2)
            x = F.batch_norm(x, c["running_mean"], c["running_var"], p["_ext_post_bn.weight"], p["_ext_post_bn.bias"], False, 0.01, 1e-3)
            if pooled:
                x = F.max_pool2d(x, (2, 1))
        return x                                  # (N, 64 ch, 32 f, 64 t)

    def step(self, x, dY):
        self.opt.zero_grad()
        self.forward(x).backward(dY)
        self.opt.step()


def copy_rate(calls, reps):
    """bytes per second (read plus written) of a device-to-device copy of 1 GiB"""
    import torch
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    ms, _, _ = timed(lambda: dst.copy_(src), calls, reps)
    del src, dst
    torch.cuda.empty_cache()
    return 2.0 * (1 << 30) / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-train-step", action="store_true", help="the trainer alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convtrain_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdfa_amd import convtrain as CT
    from sdfa_amd import synth
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    assert torch.cuda.is_available(), "convtrain_bench needs the MI355X"
    sd = synth.make_state_dict("offsets", 1234)
    rate = copy_rate(args.calls, args.reps)
    report = {"calls_per_window": args.calls, "reps": args.reps, "lr": 1e-4, "torch": torch.__version__, "head": "offsets",
              "copy_rate_GBps": rate / 1e9, "floor_bytes_per_frame": FLOOR_BYTES_PER_FRAME, "frames": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in args.frames:
        assert N % 2 == 0, "a training batch holds every sample's window and the next one: an even number of frames"
        entry = {"N": N}
        # the trainer alone against torch's route
        feat = torch.randn(N, 64, 128, 3, device="cuda", generator=g) * torch.tensor([1.0, 0.5, 0.25], device="cuda")
        dC = (torch.randn(N, 64, 32, 64, device="cuda", generator=g) + 1.0) / (64 * N)
        x = feat.permute(0, 3, 2, 1).contiguous()               # the encoder's Permute: (N, 3 ch, 128 f, 64 t)
        dY = dC.permute(0, 3, 2, 1).contiguous()
        tr, ref = CT.ConvTrainer(sd), TorchConv(sd)
        C_ours = tr.forward(feat)
        with torch.no_grad():
            C_torch = ref.forward(x).permute(0, 3, 2, 1)
        gap = float((C_ours - C_torch).abs().max() / C_torch.abs().max())
        assert gap < 1e-5, f"C differs from torch's by {gap:.3g} of max |C|: nothing is timed"

        def ours():
            tr.forward(feat)
            tr.backward(feat, dC)
            tr.step()

        def fwd_bwd():
            tr.forward(feat)
            tr.backward(feat, dC)

        step_ms, step_all, _ = timed(ours, args.calls, args.reps)
        fb_ms, fb_all, _ = timed(fwd_bwd, args.calls, args.reps)
        fwd_ms, fwd_all, _ = timed(lambda: tr.forward(feat), args.calls, args.reps)
        base_ms, base_all, _ = timed(lambda: ref.step(x, dY), args.calls, args.reps)
        floor_ms = N * FLOOR_BYTES_PER_FRAME / rate * 1e3
        entry["trainer"] = {"launches_per_step": sum(CT.LAUNCHES.values()), "workspace_bytes": tr.workspace_bytes(N),
                            "step_ms_median": step_ms, "step_ms": step_all, "forward_ms_median": fwd_ms, "forward_ms": fwd_all,
                            "backward_ms_median": fb_ms - fwd_ms, "forward_backward_ms": fb_all,
                            "floor_ms": floor_ms, "step_over_floor": step_ms / floor_ms,
                            "torch_route": {"ms_median": base_ms, "ms": base_all, "speedup": base_ms / step_ms,
                                            "max_C_gap_over_max_C_before_training": gap}}
        del tr, ref, x, dY, C_ours, C_torch
        torch.cuda.empty_cache()
        # the whole step
        batch = None
        entry["train_step"] = {}
        for name, flags in CONFIGS:
            if args.skip_train_step:
                break
            hp, model = make_model(sd, flags)
            if batch is None:
                ts = train_set(model._model._engine.out_dim)
                batch = DSW.train_batch(ts, None, list(np.random.RandomState(3).randint(0, len(ts), N // 2)), np.random.RandomState(4), hparams=hp)
                assert batch["audio_feat"].shape[0] == N

            def step():
                _, losses, _ = model.train_step(batch, 0)
                sum(losses.values()).backward()
                model.optimizer_step()

            ms, windows, wall = timed(step, args.calls, args.reps)
            entry["train_step"][name] = {"flags": flags, "step_ms_median": ms, "step_ms": windows, "wall_ms_median": wall}
            del model
            torch.cuda.empty_cache()
        if not args.skip_train_step:
            a, b = (entry["train_step"][name]["step_ms_median"] for name, _ in CONFIGS)
            expected = None
            if N in DC_TILES_MS:
                expected = step_ms + DC_TILES_MS[N] - ENCODER_CONV_MS[N]
            entry["train_step"]["difference_ms"] = {"measured": b - a, "expected": expected,
                                                    "formula": "conv-trainer step + frequency trainer's dC tiles - sdfa_encoder_conv"}
        report["frames"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
