"""Training objective on the MI355X: sdfa_amd.objective.objective -- the four losses, the records and
both coefficient gradients of a collated batch -- on the dgrad head's shapes, against the bytes it must read once and against
the reference's route written as torch operations on the same device tensors in the same process.  bench.py (the headline
workload) is not involved.

  python tools/objective_bench.py --out profiles/objective_bench.json

Shapes    T = 9,976 triangles, Ks / Kr = 85 / 180, seeded bases like the synthetic head's; N = 100 (the shipped training
          batch, B = 50) and N = 2,048.
Timed     one objective() call = the main kernel and its three finishing kernels, workspace and output allocation included
          (the caching allocator's), by device events around --calls back-to-back calls after a warm-up; median of --reps windows.
Floor     (bases + truth, each once) over the copy rate measured here: a device-to-device copy of 1 GiB, read + write bytes
          over its time, same events, same medians.  The coefficients, weights and outputs are not counted.
Baseline  the reference's route: F.linear with each basis, view as triangles, exp of the rotat part, mse_loss, sum, means, the
          weighted batch means, then backward() of the four losses' sum to the coefficients; same timing."""
import argparse
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

T, KS, KR = 9976, 85, 180


def timed(fn, calls, reps):
    """Median over `reps` windows of (device time of `calls` back-to-back calls) / calls, in ms; and the windows."""
    import torch
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


def torch_route(coef, truth, weight, As, ms_, Ar, mr_):
    """get_loss's losses as the reference computes them (float32), and backward() to the coefficients."""
    import torch
    import torch.nn.functional as Fn
    coef = coef.detach().requires_grad_(True)
    N = coef.shape[0]
    B = N // 2
    tri = truth.view(N, 1, -1, 9)
    total = 0
    for x, y in ((Fn.linear(coef[:, :KS], As, ms_).view(N, 1, -1, 6), tri[..., :6]), (Fn.linear(coef[:, KS:], Ar, mr_).view(N, 1, -1, 3), tri[..., 6:])):
        if x.size(-1) == 3:
            x, y = torch.exp(x), torch.exp(y)
        p = Fn.mse_loss(x, y, reduction="none").sum(-1)
        while p.dim() > 1:
            p = p.mean(-1)
        m = Fn.mse_loss(x[B:] - x[:B], y[B:] - y[:B], reduction="none").sum(-1)
        while m.dim() > 1:
            m = m.mean(-1)
        total = total + (p * weight).mean(dim=0) + (m * (weight[B:] + weight[:B])).mean(dim=0)
    total.backward()
    return total.detach(), coef.grad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_bench.json"))
    args = ap.parse_args()
    import torch
    from sdfa_amd import objective as O
    assert torch.cuda.is_available(), "objective_bench needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s, std: torch.randn(*s, device="cuda", generator=g) * std      # noqa: E731
    As, ms_, Ar, mr_ = rnd(6 * T, KS, std=0.02), rnd(6 * T, std=0.01), rnd(3 * T, KR, std=0.02), rnd(3 * T, std=0.01)
    bases = O.Bases(O.LAYOUT_DGRAD, As, ms_, Ar, mr_)

    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_(generator=g)
    dst = torch.empty_like(src)
    copy_ms, copy_all = timed(lambda: dst.copy_(src), 5, args.reps)
    copy_rate = 2.0 * src.numel() * 4 / (copy_ms / 1e3)
    del src, dst
    report = {"T": T, "Ks": KS, "Kr": KR, "calls_per_window": args.calls, "reps": args.reps,
              "copy": {"bytes_read_plus_written": 2.0 * (1 << 30), "ms": copy_all, "ms_median": copy_ms, "bytes_per_s": copy_rate}, "shapes": []}
    for N in args.rows:
        coef = rnd(N, KS + KR, std=5.0)
        truth = (rows_of(rnd(N, KS + KR, std=5.0), As, ms_, Ar, mr_) + rnd(N, 9 * T, std=0.01)).contiguous()
        weight = torch.rand(N, device="cuda", generator=g) * 1.8 + 0.2
        ours_ms, ours_all = timed(lambda: O.objective(coef, truth, weight, bases), args.calls, args.reps)
        loss, rec, grad = O.objective(coef, truth, weight, bases)
        base_ms, base_all = timed(lambda: torch_route(coef, truth, weight, As, ms_, Ar, mr_), max(1, args.calls // 4), args.reps)
        total, gref = torch_route(coef, truth, weight, As, ms_, Ar, mr_)
        torch.cuda.synchronize()
        gsum = grad[0] + grad[1]
        bytes_once = 4.0 * (As.numel() + ms_.numel() + Ar.numel() + mr_.numel() + truth.numel())
        floor_ms = 1e3 * bytes_once / copy_rate
        report["shapes"].append({
            "N": N, "workspace_bytes": O.workspace_bytes(N, 9 * T, KS, KR, O.LAYOUT_DGRAD),
            "objective_ms": ours_all, "objective_ms_median": ours_ms, "bytes_each_once": bytes_once, "floor_ms": floor_ms,
            "ratio_to_floor": ours_ms / floor_ms, "achieved_bytes_per_s": bytes_once / (ours_ms / 1e3),
            "torch_route": {"ms": base_all, "ms_median": base_ms, "speedup": base_ms / ours_ms,
                            "relative_gap_of_the_objective": abs(float(loss.double().sum()) / float(total) - 1),
                            "max_gradient_gap_over_max_gradient": float((gsum - gref).abs().max() / gref.abs().max())}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


def rows_of(coef, As, ms_, Ar, mr_):
    """Interleaved [6 | 3] rows of a prediction: what the truth of the benchmark is built from."""
    import torch
    import torch.nn.functional as Fn
    N = coef.shape[0]
    s = Fn.linear(coef[:, :KS], As, ms_).view(N, -1, 6)
    r = Fn.linear(coef[:, KS:], Ar, mr_).view(N, -1, 3)
    return torch.cat((s, r), dim=-1).view(N, -1)


if __name__ == "__main__":
    main()
