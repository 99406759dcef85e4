"""Evaluate-video stage on the MI355X: GPU render time, readback, JPEG encode + AVI write, and the wall time of
`evaluate --save_video` on one 10 s synthetic clip (DESIGN.md "Rendering").  bench.py (the headline workload) is not
involved.

  python tools/render_bench.py --out profiles/render_bench.json

Frames: the FLAME topology of tests/golden/mesh_flame.npz, 600 video frames solved on the GPU from synthetic dgrad rows
(seek + deformation-transfer solve), rendered at 512 x 512 with 1 and 4 samples.  Kernel time: HIP events around one
sdfa_render_frames sequence of all 600 frames, after warm-up, median of --reps runs.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

import torch  # noqa: E402


def _events_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_evaluate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_bench needs the MI355X"

    from sdfa_amd.seek import SeekPlan
    from sdfa_amd.render import Renderer
    from sdfa_amd import synth
    from speech_anime import viewer, video
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_flame.npz"))
    viewer.set_dgrad_static(g["verts"], g["faces"], list(g["cnsts"]))
    fps, n = 60.0, args.frames
    ts = list(range(-117, int(n * 1000 / fps) + 100, 17))
    plan = SeekPlan([ts], fps)
    rs = np.random.RandomState(0)
    rows = torch.from_numpy(rs.normal(0, 0.03, (len(ts), viewer.N_MODEL_TRIS * 9)).astype(np.float32)).cuda()
    verts = viewer.track_to_mesh(rows, plan)[:n].contiguous()
    torch.cuda.synchronize()
    res = dict(frames=n, size=[args.size, args.size], n_verts=int(verts.shape[1]), n_tris=int(len(g["faces"])), reps=args.reps,
               warmup=args.warmup, device=torch.cuda.get_device_name(0))
    W = H = args.size
    for samples in (1, 4):
        r = Renderer(g["verts"], g["faces"], (W, H), samples=samples)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        ms = _events_ms(lambda: r.render(verts, out=out), args.reps, args.warmup)
        host = torch.empty_like(out, device="cpu").pin_memory()
        rb = _events_ms(lambda: host.copy_(out, non_blocking=True), args.reps, 1)
        res[f"s{samples}"] = dict(render_ms_median=statistics.median(ms), render_ms_all=[round(x, 4) for x in ms],
                                  render_us_per_frame=1000 * statistics.median(ms) / n, readback_ms_median=statistics.median(rb),
                                  rgb_bytes=int(out.numel()))
        if samples == 4:
            frames_dev = out
    # host side: JPEG encode + AVI write of the 600 rendered frames (render_chunk returns slices already rendered)
    with tempfile.TemporaryDirectory() as d:
        sound = synth.make_pcm(0, int(n / fps * 44100)) * 0.5
        t0 = time.perf_counter()
        video.write_video(os.path.join(d, "x.avi"), n, lambda i0, i1: frames_dev[i0:i1], W, H, fps, sound=sound)
        res["encode_write_s"] = time.perf_counter() - t0
        res["avi_bytes"] = os.path.getsize(os.path.join(d, "x.avi"))
        t0 = time.perf_counter()
        rend = viewer.renderer((W, H))
        video.write_video(os.path.join(d, "y.avi"), n, lambda i0, i1: rend.render(verts[i0:i1]), W, H, fps, sound=sound)
        res["render_encode_write_s"] = time.perf_counter() - t0
        res["encode_threads"] = min(16, os.cpu_count() or 1)
        if not args.skip_evaluate:
            res["evaluate"] = _evaluate_10s(d, g)
    res["estimate"] = dict(samples_per_clip_s4=n * W * H * 4, note="shape-derived estimate (DESIGN.md): a few ms of GPU time per 600-frame clip")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


def _evaluate_10s(d, g):
    """`evaluate --save_video --template_mesh <FLAME obj>` on one 10 s synthetic clip, in-process (import / first-launch
    costs are paid by a 1 s warm-up run first), against the same command without --save_video."""
    from scipy.io import wavfile
    from sdfa_amd import synth
    from speech_anime import viewer
    from speech_anime.api import evaluate_model
    from speech_anime.datasets import DatasetSlidingWindow
    sr = 16000
    ck = os.path.join(d, "synth.ckpt")
    torch.save({"epoch": 0, "global_step": 0, "state": {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict("dgrad", 1234).items()}}, ck)
    hpj = os.path.join(d, "hparams.json")
    open(hpj, "w").write('{"audio": {"sample_rate": 16000}}')
    obj = os.path.join(d, "flame.obj")
    viewer.write_obj(obj, g["verts"], g["faces"])
    cn = os.path.join(d, "cnsts.txt")
    open(cn, "w").write(" ".join(str(int(i)) for i in g["cnsts"]))
    out = {}
    for name, seconds in (("warmup_1s", 1), ("clip_10s", 10)):
        wav = os.path.join(d, f"{name}.wav")
        wavfile.write(wav, sr, (synth.make_pcm(3, seconds * sr) * 32767).astype(np.int16))
        for sv in (False, True):
            DatasetSlidingWindow.hparams = None
            viewer.clear_template()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate_model(dict(mode="evaluate", load_from=ck, custom_hparams=hpj, output_dir=os.path.join(d, f"o_{name}_{int(sv)}"),
                                eval_input=wav, eval_spk_cond="m1", template_mesh=obj, mesh_constraints=cn, save_video=sv,
                                grid_w=512, grid_h=512))
            torch.cuda.synchronize()
            out[f"{name}_{'save_video' if sv else 'no_video'}_s"] = time.perf_counter() - t0
    return out


if __name__ == "__main__":
    main()
