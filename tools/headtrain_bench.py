"""One training step of the regressor head on the MI355X: sdfa_amd.headtrain.HeadTrainer -- forward,
backward and Adam -- against the reference's route written in torch on the same device in the same process: the same layers as
torch.nn.Linear under torch.nn.utils.weight_norm, the one-hot concatenated to the input, autograd, torch.optim.Adam(lr=1e-4).
bench.py (the headline workload) is not involved.

  python tools/headtrain_bench.py --out profiles/headtrain_bench.json

Shapes    both heads (dgrad: 7 layers, 265 coefficients; offsets: 3 layers, 59), N = 100 (the shipped training batch) and
          N = 2,048; seeded weights like the synthetic checkpoints'.
Timed     one step = forward(z, ids) + backward(dcoef) + step(), the ids validated once outside the loop, by device events
          around --calls back-to-back steps after a warm-up; median of --reps windows.  The torch route's step is zero_grad,
          forward, backward(dcoef), optimizer.step under the same events.
Launches  counted from the plan (sdfa_amd.headtrain.LAUNCHES), not measured.
Not here  hardware counters, 8 kHz data, the end-to-end wall time of fit_head (the encoder and train_batch dominate it)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))


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


def make_params(head, seed):
    """{name without "_model.": float32 array}: v ~ N(0, gain / fan_in), g = ||v|| uniform(0.8, 1.2), bias ~ N(0, 0.05)."""
    import numpy as np
    from sdfa_amd.headtrain import layer_shapes
    rs = np.random.RandomState(seed)
    out = {}
    for name, p, k in layer_shapes(head):
        v = rs.normal(0, np.sqrt((2.0 if k == 520 else 1.0) / k), (p, k)).astype(np.float32)
        out[name + ".weight_v"] = v
        out[name + ".weight_g"] = (np.sqrt((v.astype(np.float64) ** 2).sum(1)) * rs.uniform(0.8, 1.2, p)).astype(np.float32).reshape(-1, 1)
        out[name + ".bias"] = rs.normal(0, 0.05, p).astype(np.float32)
    return out


def torch_head(head, params):
    """The reference's layers as torch modules on the device, loaded with `params`: forward(z, onehot) -> coef."""
    import torch
    from sdfa_amd.headtrain import layer_shapes

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.names = [n for n, _, _ in layer_shapes(head)]
            self.fc = torch.nn.ModuleList([torch.nn.utils.weight_norm(torch.nn.Linear(k, p), dim=0) for _, p, k in layer_shapes(head)])
            with torch.no_grad():
                for n, m in zip(self.names, self.fc):
                    m.weight_g.copy_(torch.from_numpy(params[n + ".weight_g"]))
                    m.weight_v.copy_(torch.from_numpy(params[n + ".weight_v"]))
                    m.bias.copy_(torch.from_numpy(params[n + ".bias"]))

        def branch(self, x, oh, fcs):
            x = torch.nn.functional.leaky_relu(fcs[0](torch.cat((x, oh), 1)), 0.2)
            return fcs[2](torch.tanh(fcs[1](x)))

        def forward(self, z, oh):
            if head == "dgrad":
                h0 = torch.nn.functional.leaky_relu(self.fc[0](torch.cat((z, oh), 1)), 0.2)
                return torch.cat((self.branch(h0, oh, self.fc[1:4]), self.branch(h0, oh, self.fc[4:7])), 1)
            return self.branch(z, oh, self.fc)

    return Head().cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headtrain_bench.json"))
    args = ap.parse_args()
    import torch
    from sdfa_amd import headtrain as HT
    assert torch.cuda.is_available(), "headtrain_bench needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    report = {"calls_per_window": args.calls, "reps": args.reps, "lr": 1e-4, "torch": torch.__version__, "shapes": []}
    for head in ("dgrad", "offsets"):
        params = make_params(head, 5)
        for N in args.rows:
            tr = HT.HeadTrainer(params, head)
            net = torch_head(head, params)
            opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0)
            z = torch.randn(N, 512, device="cuda", generator=g) * 0.5
            sid = torch.randint(0, 8, (N,), device="cuda", generator=g)
            oh = torch.nn.functional.one_hot(sid, 8).float()
            dcoef = torch.randn(N, tr.coef_dim, device="cuda", generator=g) / N
            coef_ours = tr.forward(z, sid)                      # validates the ids once, with a host synchronisation
            gap = float((coef_ours - net(z, oh).detach()).abs().max() / coef_ours.abs().max())

            def ours():
                tr.forward(z, sid, check_ids=False)
                tr.backward(dcoef)
                tr.step()

            def theirs():
                opt.zero_grad()
                net(z, oh).backward(dcoef)
                opt.step()

            ours_ms, ours_all = timed(ours, args.calls, args.reps)
            base_ms, base_all = timed(theirs, args.calls, args.reps)
            n_launch = HT.LAUNCHES[head]
            report["shapes"].append({
                "head": head, "N": N, "parameters": tr.numel, "workspace_bytes": tr.workspace_bytes(N),
                "launches_per_step": n_launch, "launches_per_step_total": sum(n_launch.values()),
                "step_ms": ours_all, "step_ms_median": ours_ms,
                "torch_route": {"ms": base_all, "ms_median": base_ms, "speedup": base_ms / ours_ms,
                                "max_coef_gap_over_max_coef_before_training": gap}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
