"""Frames shared by the JPEG tests (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py): the size, quality and content matrix."""
import numpy as np

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 47), (300, 170), (500, 700), (512, 512), (8192, 16)]   # (W, H)
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
CONTENTS = ["uniform", "noise", "gradient", "primaries"]


def frame(kind, width, height, seed=0):
    """(H, W, 3) uint8.  noise: seeded uniform bytes (many 0xFF data bytes and long codes); gradient: smooth ramps in
    every channel; primaries: saturated red / green / blue / white / black bars."""
    if kind == "uniform":
        return np.full((height, width, 3), (200, 30, 90), np.uint8)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
    y, x = np.mgrid[0:height, 0:width]
    if kind == "gradient":
        return np.stack([x * 255 // max(width - 1, 1), y * 255 // max(height - 1, 1), (x + 2 * y) * 3 % 256], -1).astype(np.uint8)
    if kind == "primaries":
        pal = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0)], np.uint8)
        return pal[((x // 3) + (y // 5)) % len(pal)]
    raise ValueError(kind)


def flame_frame(golden, width=96, height=80):
    """The FLAME fixture's template rendered by the numpy rasterizer (tests/render_oracle.py), 1 sample."""
    import render_oracle as R
    g = golden["mesh_flame"]
    v = g["verts"].astype(np.float32)
    return R.render(v, g["faces"].astype(np.uint32), v, width, height, 1)[0]
