"""One training step of the attention layer on the MI355X: sdfa_amd.attntrain.AttnTrainer -- forward,
backward (with and without dH) and Adam -- against the reference's route written in torch on the same device in the same
process (conv1d stride 3, two linears, tanh, softmax, bmm, autograd, torch.optim.Adam(lr=1e-4)), and against the step's floor.
bench.py (the headline workload) is not involved.

  python tools/attntrain_bench.py --out profiles/attntrain_bench.json

Shapes    N = 100 (the shipped training batch) and N = 2,048 frames of H [N][64][512]; Glorot-sized seeded weights.
Timed     one step = forward(H) + backward(dz) + step(), by device events around --calls back-to-back steps after a warm-up;
          median of --reps windows.  The torch route's step is zero_grad, forward, backward(dz), optimizer.step under the
          same events; with dH it differentiates with respect to H as well.
Floor     30 MFLOP per frame at the 155 TFLOP/s measured fp32-matrix rate, plus H read and dH written
          once at the rate a device-to-device copy of the same bytes reaches here, under the same events.
Launches  counted from the plan (sdfa_amd.attntrain.LAUNCHES), not measured.
Unsplit   the same tool run on a library built with -DSDFA_ATTNTRAIN_BLOCK_FRAMES=32768 (one row block: the dWk contraction as
          one chain per tile) and --tag unsplit gives the backward's time without the split; DESIGN.md records both.
Not here  hardware counters; the wall time of fit_head."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

MFLOP_PER_FRAME = 30.0
MATRIX_TFLOPS = 155.0


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


def make_params(seed):
    import numpy as np
    from sdfa_amd.attntrain import PREFIX
    rs = np.random.RandomState(seed)
    f32 = np.float32
    return {
        PREFIX + "_conv_query.weight": rs.normal(0, np.sqrt(2.0 / 3072), (512, 512, 3)).astype(f32),
        PREFIX + "proj_qry.weight": rs.normal(0, np.sqrt(2.0 / 640), (128, 512)).astype(f32),
        PREFIX + "proj_key.weight": rs.normal(0, np.sqrt(2.0 / 640), (128, 512)).astype(f32),
        PREFIX + "v.weight": rs.normal(0, np.sqrt(2.0 / 129), (1, 128)).astype(f32),
        PREFIX + "b": rs.normal(0, 0.05, (1, 1, 128)).astype(f32),
    }


def torch_attention(params):
    """The reference's layer as torch operations on the device, loaded with `params`: forward(H) -> (z, align)."""
    import torch
    from sdfa_amd.attntrain import PREFIX
    F = torch.nn.functional

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for short in ("_conv_query.weight", "proj_qry.weight", "proj_key.weight", "v.weight", "b"):
                self.register_parameter(short.replace(".", "_"), torch.nn.Parameter(torch.from_numpy(params[PREFIX + short]).clone()))

        def forward(self, H):
            q = F.conv1d(H[:, 31:34].permute(0, 2, 1).contiguous(), self._conv_query_weight, stride=3).permute(0, 2, 1).contiguous()
            s = F.linear(torch.tanh(F.linear(q, self.proj_qry_weight) + F.linear(H, self.proj_key_weight) + self.b), self.v_weight)
            align = torch.softmax(s.view(H.shape[0], 1, 64), dim=-1)
            return torch.bmm(align, H).view(-1, 512), align.view(-1, 64)

    return Attn().cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="shipped", help="written into the report: which build of the library this is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attntrain_bench.json"))
    args = ap.parse_args()
    import torch
    from sdfa_amd import attntrain as AT
    assert torch.cuda.is_available(), "attntrain_bench needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    report = {"build": args.tag, "block_frames_of_the_binding": AT.BLOCK_FRAMES, "calls_per_window": args.calls, "reps": args.reps, "lr": 1e-4, "torch": torch.__version__,
              "mflop_per_frame": MFLOP_PER_FRAME, "matrix_tflops": MATRIX_TFLOPS, "launches": AT.LAUNCHES, "shapes": []}
    params = make_params(5)
    for N in args.frames:
        H = torch.tanh(torch.randn(N, 64, 512, device="cuda", generator=g))
        dz = torch.randn(N, 512, device="cuda", generator=g) / N
        spare = torch.empty_like(H)
        copy_ms, _ = timed(lambda: spare.copy_(H), args.calls, args.reps)          # reads H's bytes, writes as many: H in, dH out
        flop_ms = N * MFLOP_PER_FRAME * 1e6 / (MATRIX_TFLOPS * 1e12) * 1e3
        entry = {"N": N, "parameters": None, "copy_ms": copy_ms, "copy_GBps": 2 * H.numel() * 4 / copy_ms / 1e6,
                 "floor_ms": {"matrix": flop_ms, "with_dH": flop_ms + copy_ms, "without_dH": flop_ms + copy_ms / 2}}
        for want_dH in (True, False):
            tr = AT.AttnTrainer(params)
            net = torch_attention(params)
            opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0)
            Hg = H.clone().requires_grad_(want_dH)
            z_ours, _ = tr.forward(H)
            gap = float((z_ours - net(H)[0].detach()).abs().max() / z_ours.abs().max())

            def ours():
                tr.forward(H)
                tr.backward(dz, want_dH=want_dH)
                tr.step()

            def theirs():
                opt.zero_grad()
                Hg.grad = None
                net(Hg)[0].backward(dz)
                opt.step()

            ours_ms, ours_all = timed(ours, args.calls, args.reps)
            tr.forward(H)
            bwd_ms, _ = timed(lambda: tr.backward(dz, want_dH=want_dH), args.calls, args.reps)       # the backward's launches alone
            base_ms, base_all = timed(theirs, args.calls, args.reps)
            key = "with_dH" if want_dH else "without_dH"
            entry["parameters"] = tr.numel
            entry["workspace_bytes"] = tr.workspace_bytes(N)
            entry[key] = {"launches_per_step": AT.LAUNCHES["forward"] + AT.LAUNCHES["backward" if want_dH else "backward_without_dH"] + AT.LAUNCHES["adam"],
                          "step_ms": ours_all, "step_ms_median": ours_ms, "backward_ms_median": bwd_ms,
                          "torch_route": {"ms": base_all, "ms_median": base_ms, "speedup": base_ms / ours_ms,
                                          "max_z_gap_over_max_z_before_training": gap},
                          "over_floor": ours_ms / entry["floor_ms"][key]}
        report["shapes"].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
