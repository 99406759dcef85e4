"""What training more of the model costs on the MI355X: one whole training step of
SaberSpeechDrivenAnimation -- train_step, the summed losses' backward, optimizer_step -- with the head alone, + attention,
+ the BiLSTM's top layer, + its bottom layer; sdfa_encoder_x0 against sdfa_encoder_layer0 and sdfa_encoder_memory on the same
input; and the two chained LstmTrainers against the reference's route in torch in the same process (torch.nn.LSTM of two
bidirectional layers without biases, autograd, torch.optim.Adam(lr=1e-4)).  bench.py (the headline workload) is not involved.

  python tools/bilstm_bench.py --out profiles/bilstm_bench.json

Model     the synthetic offsets checkpoint (sdfa_amd.synth, seed 1234) and a two-clip synthetic TrainSet; a batch of N frames is
          DatasetSlidingWindow.train_batch of N / 2 seeded indices (every sample brings its window and the next one), built once
          per N and reused, so train_batch is not in the timed region.
Timed     by device events around --calls back-to-back calls after two warm-up calls; median of --reps windows.  A training
          step reads its four loss values back once (get_loss), so its time includes that synchronisation and the host work
          between the launches; the wall time of the same window is recorded next to it.
Encoder   the three exits on the batch's audio_feat: "x0" ends after the frequency projection (+ the expansion and the copy
          out), "layer0" after the layer-0 recurrence, "memory" runs the whole encoder.
Two layers  ours: LstmTrainer(layer=0, want_dX=False) and LstmTrainer(layer=1) driven directly -- forward, forward, backward,
          backward, two Adam steps, 14 launches -- on a seeded X0 and dH; torch: nn.LSTM(256, 256, num_layers=2, bias=False,
          bidirectional=True, dropout=0) with the same weights, zero_grad, forward, backward(dH), optimizer.step.
Not here  hardware counters; a per-kernel split; bilstm_dropout > 0 (one elementwise product more in each direction); the dgrad
          head; 8 kHz data."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

CONFIGS = (("head", {}), ("head+attention", dict(attention=True)), ("head+attention+top", dict(attention=True, bilstm_top=True)),
           ("head+attention+top+bottom", dict(attention=True, bilstm_top=True, bilstm_bottom=True)))


def timed(fn, calls, reps):
    """Median over `reps` windows of (device time of `calls` back-to-back calls) / calls in ms, the windows, and the median wall time."""
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / calls)
        ms.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ms), ms, statistics.median(wall)


def train_set(width, sr=16000):
    """Two synthetic clips with random-walk tracks, as the training tests build them."""
    import numpy as np
    from sdfa_amd import synth
    from speech_anime import hparams as H
    from speech_anime.datasets.sliding_window import SOURCES, TrainSet
    rs = np.random.RandomState(9)
    clips, tracks = [], []
    for L, seed, kind, spk, start_ts, minfi, maxfi in ((9600, 70, "speechlike", "m0", 37.5, 3, 40), (7200, 74, "uniform", "f1", 0.0, 0, 30)):
        c = dict(sr=sr, speaker_id=H.DEFAULTS["dataset_anime"]["speakers"][spk], start_ts=start_ts, anime_minfi=minfi, anime_maxfi=maxfi)
        for si, s in enumerate(SOURCES):
            c[s] = synth.make_pcm(seed + si, L // 2 if s.endswith("_8k") else L, kind)
        clips.append(c)
        n = maxfi - minfi + 1
        track = (np.cumsum(rs.normal(0, 0.01, (n, width)), axis=0) + rs.normal(0, 0.05, (1, width))).astype(np.float32)
        tracks.append((track, rs.uniform(0.0, 0.02, n).astype(np.float32)))
    return TrainSet(clips, tracks, sr)


def make_model(sd, flags):
    from speech_anime import hparams as Hp
    from speech_anime.model.model import SaberSpeechDrivenAnimation
    hp = Hp.configure({"custom_hparams": "offsets"})
    hp.audio.set_key("sample_rate", 16000)
    hp.set_key("loss", dict(ploss_scale=1, mloss_scale=1, dynamic_scalar=True, anime_loss_weight="anime_weight"))
    return hp, SaberSpeechDrivenAnimation(hp).load_state_dict(sd).enable_head_training(sd, **flags)


def torch_two_layers(params):
    import torch
    from sdfa_amd.lstmtrain import PREFIX
    net = torch.nn.LSTM(256, 256, num_layers=2, bias=False, batch_first=True, bidirectional=True, dropout=0.0)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(params[PREFIX + n]))
    return net.cuda().train()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 2048])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilstm_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdfa_amd import lstmtrain as LT
    from sdfa_amd import synth
    from speech_anime.datasets.sliding_window import DatasetSlidingWindow as DSW
    assert torch.cuda.is_available(), "bilstm_bench needs the MI355X"
    sd = synth.make_state_dict("offsets", 1234)
    report = {"calls_per_window": args.calls, "reps": args.reps, "lr": 1e-4, "torch": torch.__version__, "head": "offsets", "frames": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in args.frames:
        assert N % 2 == 0, "a training batch holds every sample's window and the next one: an even number of frames"
        entry = {"N": N, "train_step": {}}
        batch = None
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

            ms, windows, wall = timed(step, args.calls, args.reps)
            entry["train_step"][name] = {"flags": flags, "step_ms_median": ms, "step_ms": windows, "wall_ms_median": wall}
            if name == CONFIGS[-1][0]:
                eng, feat = model._model._engine, batch["audio_feat"].contiguous()
                enc = {}
                for what, fn in (("x0", lambda: eng.encoder_x0(feat)), ("layer0", lambda: eng.encoder_layer0(feat)),
                                 ("memory", lambda: eng.encoder_memory(feat, want_z=False, want_align=False))):
                    m, w, _ = timed(fn, args.calls, args.reps)
                    enc[what] = {"ms_median": m, "ms": w}
                entry["encoder_exits"] = enc
            del model
            torch.cuda.empty_cache()
        # the two layers alone: ours chained directly, torch's two-layer nn.LSTM
        rs = np.random.RandomState(5)
        params = {n: rs.uniform(-1.0 / 16, 1.0 / 16, s).astype(np.float32) for layer in (0, 1) for n, s in LT.tensor_shapes(layer).items()}
        X0 = torch.tanh(torch.randn(N, 64, 256, device="cuda", generator=g))
        dH = torch.randn(N, 64, 512, device="cuda", generator=g) / N
        t0, t1 = LT.LstmTrainer(params, layer=0, want_dX=False), LT.LstmTrainer(params, layer=1)
        net = torch_two_layers(params)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0)
        H_ours = t1.forward(t0.forward(X0))
        gap = float((H_ours - net(X0)[0].detach()).abs().max() / H_ours.abs().max())

        def ours():
            t1.forward(t0.forward(X0))
            t0.backward(t1.backward(dH, want_dX=True), want_dX=False)
            t0.step()
            t1.step()

        def theirs():
            opt.zero_grad()
            net(X0)[0].backward(dH)
            opt.step()

        ours_ms, ours_all, _ = timed(ours, args.calls, args.reps)
        base_ms, base_all, _ = timed(theirs, args.calls, args.reps)
        entry["two_layers"] = {"launches_per_step": 2 * sum(LT.LAUNCHES.values()), "step_ms_median": ours_ms, "step_ms": ours_all,
                               "workspace_bytes": t0.workspace_bytes(N) + t1.workspace_bytes(N),
                               "torch_route": {"ms_median": base_ms, "ms": base_all, "speedup": base_ms / ours_ms,
                                               "max_H_gap_over_max_H_before_training": gap}}
        del t0, t1, net, opt
        torch.cuda.empty_cache()
        report["frames"].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
