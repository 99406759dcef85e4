"""`python3 -m speech_anime evaluate ...` -- accepts the flags evaluate.sh passes (speech_anime/__main__.py:8-49)."""
import argparse

from .api import train_model, evaluate_model, jit_trace

# (flag, type or None for a store_true switch, default)
_FLAGS = [
    ("tag", str, None), ("template_mesh", str, None), ("mesh_constraints", str, None), ("mesh_tricorres", str, None),
    ("matplotlib_use", str, "Agg"), ("log_dir", str, None), ("load_from", str, None), ("custom_hparams", str, None),
    ("ensembling_ms", int, None), ("save_video", None, False),
    ("eval_input", str, None), ("eval_spk_cond", str, None), ("export_mesh_frames", None, False), ("output_dir", str, None),
    ("grid_w", int, 512), ("grid_h", int, 512), ("font_size", int, 24),
    ("overwrite_video", None, False), ("with_title", None, False), ("draw_truth", None, False),
    ("draw_align", None, False), ("draw_latent", None, False), ("traced_dump_path", str, None),
]


def _parser():
    ap = argparse.ArgumentParser(prog="speech_anime")
    ap.add_argument("mode", choices=["train", "evaluate", "trace"])
    for name, typ, default in _FLAGS:
        if typ is None:
            ap.add_argument("--" + name, action="store_true")
        else:
            ap.add_argument("--" + name, type=typ, default=default)
    # not a reference flag: who encodes the --save_video frames to JPEG (host PIL threads or the GPU; the same bytes)
    ap.add_argument("--jpeg_encoder", choices=["pil", "gpu"], default="pil")
    # not a reference flag: the FLAME neutral .obj the offsets head's rows are measured from; with it the offsets head is retargeted to
    # --template_mesh (any topology, through --mesh_tricorres) by the deformation transfer the dgrad head uses
    ap.add_argument("--source_mesh", type=str, default=None)
    # not a reference flag: a temporal filter of the animation rows, applied on the GPU where the reference's identity hook _filter_anime
    # sits: gaussian:SIGMA or bilateral:DISTANCE_SIGMA,RANGE_SIGMA,RADIUS[,FACTOR] (sdfa_amd.tfilter.parse_filter)
    ap.add_argument("--filter_anime", type=str, default=None, metavar="SPEC")
    return ap


if __name__ == "__main__":
    ns = _parser().parse_args()
    {"train": train_model, "evaluate": evaluate_model, "trace": jit_trace}[ns.mode](ns)
