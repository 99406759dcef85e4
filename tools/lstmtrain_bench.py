"""One training step of a BiLSTM layer on the MI355X: sdfa_amd.lstmtrain.LstmTrainer -- forward, backward
(with and without dX) and Adam -- against the reference's route in torch on the same device in the same process
(torch.nn.LSTM of one bidirectional layer without biases, autograd, torch.optim.Adam(lr=1e-4)), and against the step's floor.
bench.py (the headline workload) is not involved.

  python tools/lstmtrain_bench.py --out profiles/lstmtrain_bench.json

Shapes    both widths (layer 0: 256, layer 1: 512) at N = 100 (the shipped training batch) and N = 2,048 frames of X [N][64][I];
          torch's initialisation, seeded.
Timed     one step = forward(X) + backward(dY) + step(), by device events around --calls back-to-back steps after a warm-up;
          median of --reps windows.  The forward alone and Adam alone are timed the same way; the backward (which consumes the
          kept gates and cannot be repeated alone) is the step minus the two.  The torch route's step is zero_grad, forward,
          backward(dY), optimizer.step under the same events; with dX it differentiates with respect to X as well.
Floor     the step's products at the 155 TFLOP/s measured fp32-matrix rate: per frame and direction
          64 x 1024 x (3 I + 3 x 256) multiply-adds (pre, dW_ih, dX over I; the two recurrences and dW_hh over 256), 604 MFLOP per
          frame for layer 1 and 403 for layer 0 (a third of the I share less without dX); plus the kept state (640 KiB per frame)
          written and read once, at the rate a device-to-device copy of the same bytes reaches here, under the same events.
Launches  counted from the plan (sdfa_amd.lstmtrain.LAUNCHES), not measured.
Not here  hardware counters; a per-kernel split inside the forward and the backward; the wall time of fit_head."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

MATRIX_TFLOPS = 155.0
KEPT_BYTES_PER_FRAME = 2 * 64 * (1024 + 256) * 4


def mflop_per_frame(I, want_dX):
    return 2 * 2 * 64 * 1024 * ((3 if want_dX else 2) * I + 3 * 256) / 1e6


def timed(fn, calls, reps):
    """Median over `reps` windows of (device time of `calls` back-to-back calls) / calls, in ms; and the windows."""
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ms), ms


def make_params(layer, seed):
    import numpy as np
    from sdfa_amd.lstmtrain import tensor_shapes
    rs = np.random.RandomState(seed)
    return {n: rs.uniform(-1.0 / 16, 1.0 / 16, s).astype(np.float32) for n, s in tensor_shapes(layer).items()}


def torch_lstm(layer, params):
    """The reference's layer as torch.nn.LSTM on the device, loaded with `params`."""
    import torch
    from sdfa_amd.lstmtrain import IN_DIM, PREFIX
    net = torch.nn.LSTM(IN_DIM[layer], 256, num_layers=1, bias=False, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(params[PREFIX + n.replace("_l0", f"_l{layer}")]))
    return net.cuda().train()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--layers", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstmtrain_bench.json"))
    args = ap.parse_args()
    import torch
    from sdfa_amd import lstmtrain as LT
    assert torch.cuda.is_available(), "lstmtrain_bench needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    report = {"tile_frames": LT.TILE_FRAMES, "block_frames": LT.BLOCK_FRAMES, "calls_per_window": args.calls, "reps": args.reps, "lr": 1e-4,
              "torch": torch.__version__, "matrix_tflops": MATRIX_TFLOPS, "kept_bytes_per_frame": KEPT_BYTES_PER_FRAME, "launches": LT.LAUNCHES,
              "shapes": []}
    for layer in args.layers:
        I = LT.IN_DIM[layer]
        params = make_params(layer, 5 + layer)
        for N in args.frames:
            X = torch.tanh(torch.randn(N, 64, I, device="cuda", generator=g))
            dY = torch.randn(N, 64, 512, device="cuda", generator=g) / N
            kept = torch.empty(N * KEPT_BYTES_PER_FRAME, dtype=torch.uint8, device="cuda")
            spare = torch.empty_like(kept)
            copy_ms, _ = timed(lambda: spare.copy_(kept), args.calls, args.reps)      # reads the kept state's bytes once, writes as many
            entry = {"layer": layer, "in_dim": I, "N": N, "copy_ms": copy_ms, "copy_GBps": 2 * kept.numel() / copy_ms / 1e6}
            del spare, kept
            for want_dX in (True, False):
                tr = LT.LstmTrainer(params, layer=layer)
                net = torch_lstm(layer, params)
                opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0)
                Xg = X.clone().requires_grad_(want_dX)
                Y_ours = tr.forward(X)
                gap = float((Y_ours - net(X)[0].detach()).abs().max() / Y_ours.abs().max())

                def ours():
                    tr.forward(X)
                    tr.backward(dY, want_dX=want_dX)
                    tr.step()

                def theirs():
                    opt.zero_grad()
                    Xg.grad = None
                    net(Xg)[0].backward(dY)
                    opt.step()

                ours_ms, ours_all = timed(ours, args.calls, args.reps)
                fwd_ms, _ = timed(lambda: tr.forward(X), args.calls, args.reps)
                adam_ms, _ = timed(tr.step, args.calls, args.reps)
                base_ms, base_all = timed(theirs, args.calls, args.reps)
                mflop = mflop_per_frame(I, want_dX)
                flop_ms = N * mflop * 1e6 / (MATRIX_TFLOPS * 1e12) * 1e3
                key = "with_dX" if want_dX else "without_dX"
                entry["parameters"] = tr.numel
                entry["workspace_bytes"] = tr.workspace_bytes(N)
                entry[key] = {"launches_per_step": sum(LT.LAUNCHES.values()), "mflop_per_frame": mflop,
                              "floor_ms": {"matrix": flop_ms, "kept_state": copy_ms, "sum": flop_ms + copy_ms},
                              "step_ms": ours_all, "step_ms_median": ours_ms, "forward_ms_median": fwd_ms, "adam_ms_median": adam_ms,
                              "backward_ms_by_difference": ours_ms - fwd_ms - adam_ms,
                              "torch_route": {"ms": base_all, "ms_median": base_ms, "speedup": base_ms / ours_ms,
                                              "max_Y_gap_over_max_Y_before_training": gap},
                              "over_floor": ours_ms / (flop_ms + copy_ms)}
                del tr, net, opt
                torch.cuda.empty_cache()
            report["shapes"].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
