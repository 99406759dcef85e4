"""GPU OBJ text formatter on the MI355X (DESIGN.md "OBJ text"): device time of the vertex blocks of 600 FLAME-size frames,
`viewer.write_obj_frames` wall time against the loop of `viewer.write_obj` calls it replaced (alternated in one process), and
`evaluate --export_mesh_frames` on a 10 s clip with each writer.  bench.py (the headline workload) is not involved.

  python tools/obj_export_bench.py --out profiles/obj_export_bench.json --ab profiles/obj_export_ab.txt

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout -k 10`, one after the other,
and the first that fails ends the run (nothing more is started on the GPU).  Steps:
  frames    synthetic dgrad rows, seek + solve on the GPU (tools/render_bench.py's frames) -> (600, 5023, 3) vertices.  Format time:
            HIP events around one ObjFormatter.submit sequence of all frames, after warm-up, median of --reps.  Wall times: the
            files of all frames into a fresh directory, device writer and host loop alternated --pairs times; the host loop is
            the export stage as it was: vertices to the host, then write_obj per frame.
  evaluate  speech_anime.api.evaluate_model on one 10 s synthetic clip with a FLAME template, export_mesh_frames on, with
            viewer.write_obj_frames as it is and replaced by the host loop, alternated (a 1 s warm-up clip with each first)."""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdfa-2019_amd"))

STEP_TIMEOUT_S = {"frames": 420, "evaluate": 540}


def _host_loop(out_dir, verts, faces):
    """The export stage before the device formatter: the vertices go to the host as floats, write_obj formats every number."""
    from speech_anime import viewer
    host = verts.cpu().numpy()
    for i in range(len(host)):
        viewer.write_obj(os.path.join(out_dir, f"{i:06d}.obj"), host[i], faces)


def _same_files(a, b):
    names = sorted(os.listdir(a))
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    return names == sorted(os.listdir(b)) and not mismatch and not errors


def step_frames(args):
    import torch
    from sdfa_amd.obj import ObjFormatter
    from sdfa_amd.seek import SeekPlan
    from speech_anime import viewer
    assert torch.cuda.is_available(), "obj_export_bench needs the MI355X"
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_flame.npz"))
    viewer.set_dgrad_static(g["verts"], g["faces"], list(g["cnsts"]))
    fps, n = 60.0, args.frames
    ts = list(range(-117, int(n * 1000 / fps) + 100, 17))
    rows = torch.from_numpy(np.random.RandomState(0).normal(0, 0.03, (len(ts), viewer.N_MODEL_TRIS * 9)).astype(np.float32)).cuda()
    verts = viewer.track_to_mesh(rows, SeekPlan([ts], fps))[:n].contiguous()
    torch.cuda.synchronize()
    faces = viewer.template_faces()
    res = dict(frames=n, n_verts=int(verts.shape[1]), n_tris=int(len(faces)), reps=args.reps, warmup=args.warmup, pairs=args.pairs,
               device=torch.cuda.get_device_name(0))

    fmt = ObjFormatter(verts.shape[1])
    res["chunk_frames"] = fmt.chunk

    def format_all():
        return [fmt.submit(verts[i0:i0 + fmt.chunk]) for i0 in range(0, n, fmt.chunk)]
    for _ in range(args.warmup):
        format_all()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pending = format_all()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    blocks = [blk for p in pending for blk in p.result()[0]]
    del pending
    res["format_ms_median"] = statistics.median(ms)
    res["format_ms_all"] = [round(x, 4) for x in ms]
    res["format_us_per_frame"] = 1000 * statistics.median(ms) / n
    res["vertex_block_bytes_per_frame"] = sum(len(b) for b in blocks) / n
    res["file_bytes_per_frame"] = res["vertex_block_bytes_per_frame"] + len(viewer.obj_writer(verts.device).face_block)
    res["format_gb_per_s"] = sum(len(b) for b in blocks) / (statistics.median(ms) * 1e-3) / 1e9

    walls = {"device": [], "host_loop": []}
    with tempfile.TemporaryDirectory() as d:
        viewer.write_obj_frames(d, verts[:8], faces)                          # warm-up of both (first files, pinned buffers)
        _host_loop(d, verts[:8], faces)
    for k in range(args.pairs):
        with tempfile.TemporaryDirectory() as d:
            for name, fn in (("device", viewer.write_obj_frames), ("host_loop", _host_loop)):
                out = os.path.join(d, name)
                os.makedirs(out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(out, verts, faces)
                walls[name].append(time.perf_counter() - t0)
            if k == 0:
                res["files_identical"] = _same_files(os.path.join(d, "device"), os.path.join(d, "host_loop"))
    w = viewer.obj_writer(verts.device)
    res["device_frames"], res["host_frames"] = w.device_frames, w.host_frames
    res["write_frames_s"] = {k: dict(median=statistics.median(v), all=[round(x, 4) for x in v]) for k, v in walls.items()}
    res["write_frames_ms_per_frame"] = {k: 1000 * statistics.median(v) / n for k, v in walls.items()}
    return res


def step_evaluate(args):
    """evaluate_model on one clip in-process, with each writer, alternated (a 1 s warm-up run of each first)."""
    import torch
    from scipy.io import wavfile
    from sdfa_amd import synth
    from speech_anime import viewer
    from speech_anime.api import evaluate_model
    from speech_anime.datasets import DatasetSlidingWindow
    assert torch.cuda.is_available(), "obj_export_bench needs the MI355X"
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_flame.npz"))
    sr = 16000
    device_writer = viewer.write_obj_frames
    out = dict(seconds=args.seconds, pairs=args.eval_pairs, device=torch.cuda.get_device_name(0))
    walls = {"device": [], "host_loop": []}
    with tempfile.TemporaryDirectory() as d:
        ck = os.path.join(d, "synth.ckpt")
        torch.save({"epoch": 0, "global_step": 0, "state": {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state_dict("dgrad", 1234).items()}}, ck)
        hpj = os.path.join(d, "hparams.json")
        open(hpj, "w").write('{"audio": {"sample_rate": 16000}}')
        obj = os.path.join(d, "flame.obj")
        viewer.write_obj(obj, g["verts"], g["faces"])
        cn = os.path.join(d, "cnsts.txt")
        open(cn, "w").write(" ".join(str(int(i)) for i in g["cnsts"]))
        try:
            for name, seconds, pairs in (("warmup", 1, 1), ("clip", args.seconds, args.eval_pairs)):
                wav = os.path.join(d, f"{name}.wav")
                wavfile.write(wav, sr, (synth.make_pcm(3, seconds * sr) * 32767).astype(np.int16))
                for k in range(pairs):
                    for mode in ("device", "host_loop"):
                        viewer.write_obj_frames = device_writer if mode == "device" else _host_loop
                        DatasetSlidingWindow.hparams = None
                        viewer.clear_template()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        evaluate_model(dict(mode="evaluate", load_from=ck, custom_hparams=hpj, output_dir=os.path.join(d, f"o_{name}_{mode}"),
                                            eval_input=wav, eval_spk_cond="m1", template_mesh=obj, mesh_constraints=cn,
                                            export_mesh_frames=True))
                        torch.cuda.synchronize()
                        if name == "clip":
                            walls[mode].append(time.perf_counter() - t0)
        finally:
            viewer.write_obj_frames = device_writer
        a, b = (os.path.join(d, f"o_clip_{m}", "clip") for m in ("device", "host_loop"))
        out["obj_files"] = len([p for p in os.listdir(a) if p.endswith(".obj")])
        out["files_identical"] = _same_files(a, b)
    out["evaluate_s"] = {k: dict(median=statistics.median(v), all=[round(x, 4) for x in v]) for k, v in walls.items()}
    return out


STEPS = {"frames": step_frames, "evaluate": step_evaluate}


def _ab_text(res):
    f, lines = res.get("frames"), []
    lines.append("OBJ export: device formatter (sdfa_amd.obj) against the host loop of viewer.write_obj calls, same process, alternated")
    lines.append(f"device: {res.get('device')}")
    if f:
        w = f["write_frames_s"]
        lines.append(f"{f['frames']} frames of {f['n_verts']} vertices / {f['n_tris']} triangles, {f['file_bytes_per_frame']:.0f} file bytes per frame "
                     f"({f['vertex_block_bytes_per_frame']:.0f} of them the vertex block)")
        lines.append(f"  format on the device (HIP events, median of {f['reps']}): {f['format_ms_median']:.3f} ms = {f['format_us_per_frame']:.2f} us per frame, "
                     f"{f['format_gb_per_s']:.1f} GB/s of text")
        for k in ("device", "host_loop"):
            lines.append(f"  write all files, {k:9s}: median {w[k]['median']:.3f} s ({f['write_frames_ms_per_frame'][k]:.3f} ms per frame), runs {w[k]['all']}")
        lines.append(f"  host_loop / device = {w['host_loop']['median'] / w['device']['median']:.1f}x; files identical: {f['files_identical']}; "
                     f"device_frames {f['device_frames']}, host_frames {f['host_frames']}")
    e = res.get("evaluate")
    if e:
        w = e["evaluate_s"]
        lines.append(f"evaluate --export_mesh_frames, one {e['seconds']} s clip, {e['obj_files']} .obj files")
        for k in ("device", "host_loop"):
            lines.append(f"  {k:9s}: median {w[k]['median']:.3f} s, runs {w[k]['all']}")
        lines.append(f"  host_loop - device = {w['host_loop']['median'] - w['device']['median']:.3f} s; files identical: {e['files_identical']}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON line")
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=2, help="alternated device / host-loop runs over all frames")
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--eval_pairs", type=int, default=2, help="alternated device / host-loop evaluate runs")
    ap.add_argument("--skip_evaluate", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", default=None)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step](args)))
        return 0
    res = {}
    passed = ["--frames", args.frames, "--reps", args.reps, "--warmup", args.warmup, "--pairs", args.pairs, "--seconds", args.seconds,
              "--eval_pairs", args.eval_pairs]
    for step in ("frames",) + (() if args.skip_evaluate else ("evaluate",)):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step] + [str(x) for x in passed]
        sys.stderr.write(f"[obj_export_bench] step {step} (limit {STEP_TIMEOUT_S[step]} s)\n")
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"[obj_export_bench] step {step} ended with status {r.returncode}: nothing more is started\n{r.stdout[-2000:]}\n")
            return r.returncode
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
        res["device"] = res[step]["device"]
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.ab, _ab_text(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fp:
                fp.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
