"""What training the frequency LSTM costs on the MI355X: one FreqTrainer step -- forward, backward with and
without dC, Adam -- against the reference's route in torch in the same process (torch.nn.LSTM(64, 128, bidirectional=True) +
Linear(8192, 256) + autograd + torch.optim.Adam(lr=1e-4)); one whole training step of SaberSpeechDrivenAnimation -- train_step,
the summed losses' backward, optimizer_step -- with + freq_lstm next to + bottom (the step before this section); and
sdfa_encoder_conv next to the encoder's other exits on the same input.  bench.py (the headline workload) is not involved.

  python tools/freqtrain_bench.py --out profiles/freqtrain_bench.json

Model     the synthetic offsets checkpoint (sdfa_amd.synth, seed 1234) and a two-clip synthetic TrainSet; a batch of N frames is
          DatasetSlidingWindow.train_batch of N / 2 seeded indices, built once per N and reused, so train_batch is not in the
          timed region.
Timed     by device events around --calls back-to-back calls after two warm-up calls; median of --reps windows.  A training
          step reads its four loss values back once (get_loss), so its time includes that synchronisation and the host work
          between the launches; the wall time of the same window is recorded next to it.
Trainer   ours: FreqTrainer driven directly on a seeded C and dX0 -- forward, backward, Adam, 9 launches; torch: the two modules
          with the same weights on the same C viewed as (64 N, 32, 64), zero_grad, forward, backward(dX0), optimizer.step.  X0
          must agree with torch's to its float32 round-off before anything is timed.  MIOpen refuses an nn.LSTM call of 131,072
          sequences (N = 2,048), so torch's step runs pieces of 32,768 sequences whose gradients accumulate; N = 100 is one call.
Encoder   the four exits on the batch's audio_feat: "conv" ends after the conv stack (+ the copy out through the share map),
          "x0" after the frequency projection, "layer0" after the layer-0 recurrence, "memory" runs the whole encoder.
Not here  hardware counters; a per-kernel split; bilstm_dropout > 0; the dgrad head; 8 kHz data."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bilstm_bench import make_model, timed, train_set  # noqa: E402

BOTTOM = dict(attention=True, bilstm_top=True, bilstm_bottom=True)
CONFIGS = (("head+attention+top+bottom", BOTTOM), ("head+attention+top+bottom+freq_lstm", dict(BOTTOM, freq_lstm=True)))


class TorchFreq:
    """the reference's route: nn.LSTM(64, 128, bidirectional) over the 32 bins, the view to (rows, 8192), Linear(8192, 256)"""

    def __init__(self, params):
        import torch
        from sdfa_amd.freqtrain import PREFIX
        self.lstm = torch.nn.LSTM(64, 128, num_layers=1, bias=True, batch_first=True, bidirectional=True)
        self.proj = torch.nn.Linear(8192, 256, bias=True)
        with torch.no_grad():
            for n, p in self.lstm.named_parameters():
                p.copy_(torch.from_numpy(params[PREFIX + "_lstm." + n]))
            for n, p in self.proj.named_parameters():
                p.copy_(torch.from_numpy(params[PREFIX + "_proj." + n]))
        self.lstm, self.proj = self.lstm.cuda().train(), self.proj.cuda().train()
        self.opt = torch.optim.Adam(list(self.lstm.parameters()) + list(self.proj.parameters()), lr=1e-4, weight_decay=0)

    CHUNK = 32768       # sequences of one nn.LSTM call: MIOpen refuses 131,072 sequences of 32 steps ("Lengths must be > 0")

    def forward(self, C3):
        y, _ = self.lstm(C3)
        return self.proj(y.contiguous().view(C3.shape[0], 8192))

    def step(self, C3, dX0):
        """one optimiser step; a batch beyond CHUNK sequences is run piece by piece, the gradients accumulating"""
        self.opt.zero_grad()
        for r0 in range(0, C3.shape[0], self.CHUNK):
            self.forward(C3[r0:r0 + self.CHUNK]).backward(dX0[r0:r0 + self.CHUNK])
        self.opt.step()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-train-step", action="store_true", help="the trainer and the encoder exits only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freqtrain_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdfa_amd import freqtrain as FT
    from sdfa_amd import synth
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    assert torch.cuda.is_available(), "freqtrain_bench needs the MI355X"
    sd = synth.make_state_dict("offsets", 1234)
    report = {"calls_per_window": args.calls, "reps": args.reps, "lr": 1e-4, "torch": torch.__version__, "head": "offsets", "frames": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in args.frames:
        assert N % 2 == 0, "a training batch holds every sample's window and the next one: an even number of frames"
        entry = {"N": N}
        # the trainer alone against torch's route
        rs = np.random.RandomState(5)
        params = {n: rs.uniform(-1.0, 1.0, s).astype(np.float32) / np.float32(np.sqrt(8192 if "_proj" in n else 128)) for n, s in FT.tensor_shapes().items()}
        C4 = torch.tanh(torch.randn(N, 64, 32, 64, device="cuda", generator=g))
        dX3 = (torch.randn(N, 64, 256, device="cuda", generator=g) + 1.0) / (64 * N)
        C3, dX2 = C4.view(64 * N, 32, 64), dX3.view(64 * N, 256)
        tr, ref = FT.FreqTrainer(params), TorchFreq(params)
        X0_ours = tr.forward(C4).view(64 * N, 256)
        with torch.no_grad():
            X0_torch = torch.cat([ref.forward(C3[r0:r0 + ref.CHUNK]) for r0 in range(0, 64 * N, ref.CHUNK)])
        gap = float((X0_ours - X0_torch).abs().max() / X0_torch.abs().max())
        assert gap < 1e-5, f"X0 differs from torch's by {gap:.3g} of max |X0|: nothing is timed"

        def ours(want_dC):
            tr.forward(C4)
            tr.backward(dX3, want_dC=want_dC)
            tr.step()

        with_ms, with_all, _ = timed(lambda: ours(True), args.calls, args.reps)
        without_ms, without_all, _ = timed(lambda: ours(False), args.calls, args.reps)
        fwd_ms, fwd_all, _ = timed(lambda: tr.forward(C4), args.calls, args.reps)
        base_ms, base_all, _ = timed(lambda: ref.step(C3, dX2), args.calls, args.reps)
        entry["trainer"] = {"launches_per_step": sum(FT.LAUNCHES.values()), "workspace_bytes": tr.workspace_bytes(N),
                            "step_ms_median": without_ms, "step_ms": without_all, "step_with_dC_ms_median": with_ms, "step_with_dC_ms": with_all,
                            "forward_ms_median": fwd_ms, "forward_ms": fwd_all,
                            "torch_route": {"ms_median": base_ms, "ms": base_all, "speedup": base_ms / without_ms, "sequences_per_lstm_call": min(64 * N, ref.CHUNK),
                                            "max_X0_gap_over_max_X0_before_training": gap}}
        del tr, ref
        torch.cuda.empty_cache()
        # the whole step, and the encoder's exits
        batch = None
        entry["train_step"] = {}
        for name, flags in CONFIGS:
            hp, model = make_model(sd, flags)
            if batch is None:
                ts = train_set(model._model._engine.out_dim)
                batch = DSW.train_batch(ts, None, list(np.random.RandomState(3).randint(0, len(ts), N // 2)), np.random.RandomState(4), hparams=hp)
                assert batch["audio_feat"].shape[0] == N

            def step():
                _, losses, _ = model.train_step(batch, 0)
                sum(losses.values()).backward()
                model.optimizer_step()

            if not args.skip_train_step:
                ms, windows, wall = timed(step, args.calls, args.reps)
                entry["train_step"][name] = {"flags": flags, "step_ms_median": ms, "step_ms": windows, "wall_ms_median": wall}
            if name == CONFIGS[-1][0]:
                eng, feat = model._model._engine, batch["audio_feat"].contiguous()
                enc = {}
                for what, fn in (("conv", lambda: eng.encoder_conv(feat)), ("x0", lambda: eng.encoder_x0(feat)), ("layer0", lambda: eng.encoder_layer0(feat)),
                                 ("memory", lambda: eng.encoder_memory(feat, want_z=False, want_align=False))):
                    m, w, _ = timed(fn, args.calls, args.reps)
                    enc[what] = {"ms_median": m, "ms": w}
                entry["encoder_exits"] = enc
            del model
            torch.cuda.empty_cache()
        report["frames"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
