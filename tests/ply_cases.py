"""A PLY writer for the tests of speech_anime.datasets.dgrad's reader and of the dataset step."""
import numpy as np


def write_ply(path, verts, faces):
    """binary_little_endian 1.0 with float x y z and `list uchar int` faces, the layout of the reference's templates."""
    v = np.ascontiguousarray(np.asarray(verts, "<f4").reshape(-1, 3))
    f = np.asarray(faces).reshape(-1, 3)
    rec = np.empty(len(f), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    rec["n"], rec["v"] = 3, f
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fp:
        fp.write(head.encode("ascii") + v.tobytes() + rec.tobytes())
