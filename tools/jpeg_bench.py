"""GPU JPEG encoder on the MI355X (DESIGN.md "GPU JPEG"): device encode time of 600 rendered FLAME frames at 512 x 512,
the bytes read back against the raw RGB, `write_video` wall time with encoder="pil" and encoder="gpu" alternated in one
process, and `evaluate --save_video` on a 10 s clip with each encoder.  bench.py (the headline workload) is not involved.

  python tools/jpeg_bench.py --out profiles/jpeg_bench.json

Frames: tools/render_bench.py's (synthetic dgrad rows, seek + solve on the GPU, 4 samples).  Encode time: HIP events around
one JpegEncoder.submit sequence of all frames (chunks of sdfa_amd.render.CHUNK_FRAMES), after warm-up, median of --reps."""
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
    ap.add_argument("--pairs", type=int, default=3, help="alternated pil / gpu write_video runs")
    ap.add_argument("--skip_evaluate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_bench needs the MI355X"

    from sdfa_amd.seek import SeekPlan
    from sdfa_amd.render import Renderer
    from sdfa_amd.jpeg import JpegEncoder
    from sdfa_amd import synth
    from speech_anime import viewer, video
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_flame.npz"))
    viewer.set_dgrad_static(g["verts"], g["faces"], list(g["cnsts"]))
    fps, n, W = 60.0, args.frames, args.size
    ts = list(range(-117, int(n * 1000 / fps) + 100, 17))
    plan = SeekPlan([ts], fps)
    rs = np.random.RandomState(0)
    rows = torch.from_numpy(rs.normal(0, 0.03, (len(ts), viewer.N_MODEL_TRIS * 9)).astype(np.float32)).cuda()
    verts = viewer.track_to_mesh(rows, plan)[:n].contiguous()
    frames = Renderer(g["verts"], g["faces"], (W, W), samples=4).render(verts)
    torch.cuda.synchronize()
    res = dict(frames=n, size=[W, W], quality=video.JPEG_QUALITY, reps=args.reps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), rgb_bytes=int(frames.numel()))

    enc = JpegEncoder(W, W, video.JPEG_QUALITY)
    res["chunk_frames"] = enc.chunk

    def encode_all():
        return [enc.submit(frames[i0:i0 + enc.chunk]) for i0 in range(0, n, enc.chunk)]
    ms = _events_ms(encode_all, args.reps, args.warmup)
    files = [f for p in encode_all() for f in p.result()]
    host = frames.cpu().numpy()
    res["identical_to_pil_first_8"] = all(files[i] == video.encode_jpeg(host[i]) for i in range(8))
    res["gpu_encode_ms_median"] = statistics.median(ms)
    res["gpu_encode_ms_all"] = [round(x, 4) for x in ms]
    res["gpu_encode_us_per_frame"] = 1000 * statistics.median(ms) / n
    res["jpeg_bytes"] = int(sum(len(f) for f in files))
    t0 = time.perf_counter()
    files2 = enc.encode(frames)
    res["gpu_encode_readback_s"] = time.perf_counter() - t0
    assert files2 == files

    with tempfile.TemporaryDirectory() as d:
        sound = synth.make_pcm(0, int(n / fps * 44100)) * 0.5
        walls = {"pil": [], "gpu": []}
        for _ in range(args.pairs):
            for encoder in ("pil", "gpu"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                video.write_video(os.path.join(d, f"{encoder}.avi"), n, lambda i0, i1: frames[i0:i1], W, W, fps, sound=sound,
                                  encoder=encoder)
                walls[encoder].append(time.perf_counter() - t0)
        res["write_video_s"] = {k: dict(median=statistics.median(v), all=[round(x, 4) for x in v]) for k, v in walls.items()}
        res["write_video_identical"] = open(os.path.join(d, "pil.avi"), "rb").read() == open(os.path.join(d, "gpu.avi"), "rb").read()
        res["encode_threads_pil"] = min(16, os.cpu_count() or 1)
        if not args.skip_evaluate:
            res["evaluate"] = _evaluate_10s(d, g)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


def _evaluate_10s(d, g):
    """`evaluate --save_video` on one 10 s synthetic clip in-process, with each encoder, alternated (a 1 s warm-up run of
    each first), and the same command without --save_video."""
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
        for mode in ("no_video", "pil", "gpu"):
            DatasetSlidingWindow.hparams = None
            viewer.clear_template()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate_model(dict(mode="evaluate", load_from=ck, custom_hparams=hpj, output_dir=os.path.join(d, f"o_{name}_{mode}"),
                                eval_input=wav, eval_spk_cond="m1", template_mesh=obj, mesh_constraints=cn,
                                save_video=mode != "no_video", jpeg_encoder="pil" if mode == "no_video" else mode,
                                grid_w=512, grid_h=512))
            torch.cuda.synchronize()
            out[f"{name}_{mode}_s"] = time.perf_counter() - t0
    a, b = (open(os.path.join(d, f"o_clip_10s_{m}", "clip_10s.avi"), "rb").read() for m in ("pil", "gpu"))
    out["clip_10s_avi_identical"] = a == b
    return out


if __name__ == "__main__":
    main()
