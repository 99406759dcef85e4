"""Template-mesh state and frame_to_mesh -- the part of speech_anime/viewer/frame.py (:17-141) that turns a
dgrad / offsets frame into vertices, backed by the GPU deformation solve (sdfa_amd.mesh), including retargeting to a
template of another topology through triangle correspondences (--mesh_tricorres) -- and the rendering of those vertices into
images on the GPU (render_frame / render_track, sdfa_amd.render; viewer/render_py.py in the reference)."""
import os

import numpy as np
import torch

from sdfa_amd.mesh import MeshSolver

_template_verts, _template_faces = None, None
_template_c_indices = []
_template_corres = None
_solver = None
_renderers = {}          # (image_size, samples, normals) -> sdfa_amd.render.Renderer of the current template, made on first use
_obj_writers = {}        # device -> sdfa_amd.obj.ObjWriter of the current template (its face block formatted once), made on first use


def read_obj(path):
    """Vertices / triangle faces of a Wavefront OBJ (what saber.mesh.read_mesh returns for the template)."""
    V, F = [], []
    with open(path) as fp:
        for line in fp:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                V.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                F.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(V, np.float32), np.asarray(F, np.uint32)


def write_obj(path, verts, faces):
    with open(path, "w") as fp:
        for v in np.asarray(verts).reshape(-1, 3):
            fp.write("v {:.6f} {:.6f} {:.6f}\n".format(*v))
        for f in np.asarray(faces).reshape(-1, 3):
            fp.write("f {} {} {}\n".format(*(f + 1)))


def obj_writer(device):
    """The .obj writer of the current template on `device` (sdfa_amd.obj.ObjWriter), created on first use."""
    assert _solver is not None, "set_template_mesh first"
    device = torch.device(device)
    if device not in _obj_writers:
        from sdfa_amd.obj import ObjWriter
        _obj_writers[device] = ObjWriter(_template_faces, len(_template_verts), device=device)
    return _obj_writers[device]


def write_obj_frames(out_dir, verts, faces):
    """<out_dir>/NNNNNN.obj for every frame of the (n, V, 3) float32 cuda vertices, each file what write_obj writes for it: the
    numbers are formatted on the device (sdfa_amd.obj), the face block once per template.  `faces` other than the current
    template's get a writer of their own."""
    assert torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 3, "write_obj_frames takes (n, V, 3) cuda vertices"
    if faces is _template_faces and verts.shape[1] == len(_template_verts):
        writer = obj_writer(verts.device)
    else:
        from sdfa_amd.obj import ObjWriter
        writer = ObjWriter(faces, verts.shape[1], device=verts.device)
    writer.write([os.path.join(out_dir, f"{i:06d}.obj") for i in range(verts.shape[0])], verts)
    return writer


N_MODEL_TRIS = 9976      # triangles of the model's FLAME-topology dgrad rows (frame.py:117: 89784 = 9976 * 9)
N_MODEL_VERTS = 5023     # vertices of the model's FLAME-topology offsets rows (15069 = 5023 * 3)

# --source_mesh (not a reference flag): the FLAME neutral the offsets head's rows are measured from.  Set, the offsets head is
# retargeted like the dgrad head -- offsets -> deform_grad(source, source + offsets), non-face triangles zeroed (preload.py:768-779)
# -> the template's solve -- so --template_mesh may be of another topology.  Host copies; the device form is made on first use.
_source = None           # dict(verts, faces, mask) of the validated source mesh
_source_dev = {}         # device -> sdfa_amd.mesh.DeformGrad of it


def set_dgrad_static(verts, faces, c_indices=None, corres=None):
    """frame.py:27-46: template state + deformation.set_target(verts, faces, cnsts, corrs=corr_count).  Without `c_indices` the
    reference pins `non_face.non_face_verts` (frame.py:33) -- 3,762 FLAME vertex indices -- and so does this; a template with
    fewer vertices than those indices address fails here like the reference's native module does on them."""
    global _template_verts, _template_faces, _template_c_indices, _template_corres, _solver
    _renderers.clear()                   # a renderer is prepared lazily for the new template (renderer())
    _obj_writers.clear()                 # and so is the .obj writer (write_obj_frames)
    _template_verts = np.asarray(verts, np.float32).reshape(-1, 3)
    _template_faces = np.asarray(faces, np.uint32).reshape(-1, 3)
    if c_indices is None:
        from .datasets.vocaset_mask import non_face_verts
        c_indices = non_face_verts()
    _template_c_indices = [int(i) for i in c_indices]
    _template_corres = None if corres is None else {k: list(corres[k]) for k in ("corr_count", "corr_faces")}
    if _template_corres is None:
        _solver = MeshSolver(_template_verts, _template_faces, _template_c_indices)
    else:
        _solver = MeshSolver(_template_verts, _template_faces, _template_c_indices, corr_count=_template_corres["corr_count"],
                             corr_faces=_template_corres["corr_faces"], n_src_tris=N_MODEL_TRIS)


def read_tricorres(corres_path, n_faces):
    """The .tricorrs file of --mesh_tricorres (frame.py:57-80): first line = number of records, then `src,dst,...` per
    line; every target triangle `dst` collects its source triangles in file order.  Returns corr_count (per target
    triangle) and corr_faces (concatenated sources, one filler 0 for a triangle without any)."""
    by_target = {}
    with open(corres_path) as fp:
        lines = fp.read().splitlines()
    remaining = int(lines[0].strip()) if lines else 0
    for line in lines[1:]:
        if remaining == 0:
            break
        src, dst = (int(x) for x in line.strip().split(",")[:2])
        by_target.setdefault(dst, []).append(src)
        remaining -= 1
    counts, flat = [], []
    for tri in range(n_faces):
        sources = by_target.get(tri, [])
        counts.append(len(sources))
        flat.extend(sources if sources else [0])
    return dict(corr_count=counts, corr_faces=flat)


def set_template_mesh(template_path, constraints_path=None, corres_path=None):
    verts, faces = read_obj(template_path)
    c_indices = None
    if constraints_path is not None:
        with open(constraints_path) as fp:
            c_indices = [int(x) for x in " ".join(l.strip() for l in fp.readlines()).split()]
    corres = read_tricorres(corres_path, len(faces)) if corres_path is not None else None
    set_dgrad_static(verts, faces, c_indices, corres)


def has_template():
    return _solver is not None


def clear_template():
    """Forget the template mesh (evaluate() then writes the dgrad track only)."""
    global _template_verts, _template_faces, _template_c_indices, _template_corres, _solver
    _template_verts = _template_faces = _template_corres = _solver = None
    _template_c_indices = []
    _renderers.clear()
    _obj_writers.clear()


def template_faces():
    return _template_faces


def set_source_mesh(source):
    """The FLAME-topology source of the offsets head: an .obj path or (verts, faces).  Validated here, before any device work:
    anything but 5,023 vertices and 9,976 triangles is refused."""
    global _source
    verts, faces = read_obj(source) if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__") else source
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if (len(verts), len(faces)) != (N_MODEL_VERTS, N_MODEL_TRIS):
        raise ValueError(f"source mesh must have the FLAME topology of the offsets head ({N_MODEL_VERTS} vertices, {N_MODEL_TRIS} "
                         f"triangles), got {len(verts)} vertices and {len(faces)} triangles")
    if faces.min() < 0 or faces.max() >= N_MODEL_VERTS:
        raise ValueError("source mesh: face index out of range")
    from .datasets.vocaset_mask import non_face_tris
    _source = dict(verts=verts, faces=faces.astype(np.uint32), mask=non_face_tris(faces))
    _source_dev.clear()


def clear_source_mesh():
    global _source
    _source = None
    _source_dev.clear()


def has_source_mesh():
    return _source is not None


def source_dgrad(offsets_rows):
    """(n, 15069) float32 cuda offsets rows -> (n, 89784) float32 dgrad rows on the device, as preload.py:768-779 makes them:
    deform_grad(source, float32(source + offsets)), the non-face triangles zeroed."""
    assert _source is not None, "set_source_mesh first"
    dev = offsets_rows.device
    if dev not in _source_dev:
        from sdfa_amd.mesh import DeformGrad
        _source_dev[dev] = DeformGrad(_source["verts"], _source["faces"], tri_mask=_source["mask"], device=dev)
    return _source_dev[dev](offsets_rows, offsets=True)


def frames_to_mesh(data_frames, face_data_type):
    """Batched frame_to_mesh: (n, 9976, 9) / (n, 89784) dgrad or (n, 15069) offsets -> (verts (n, V, 3) numpy, faces)."""
    assert _solver is not None, "set_template_mesh first"
    x = data_frames if torch.is_tensor(data_frames) else torch.from_numpy(np.asarray(data_frames, np.float32))
    n = x.shape[0]
    if str(face_data_type).endswith("dgrad_3d"):
        verts = _solver.get_mesh(x.reshape(n, -1)).cpu().numpy()
    elif str(face_data_type).endswith("verts_off_3d") and _source is not None:
        verts = _device_verts(x.to(device=_solver.device, dtype=torch.float32), face_data_type).cpu().numpy()
    elif str(face_data_type).endswith("verts_off_3d"):
        verts = x.reshape(n, -1, 3).cpu().numpy() + _template_verts[None]
    else:
        verts = x.reshape(n, -1, 3).cpu().numpy()
    return verts, _template_faces


def track_to_mesh(anime_rows, plan):
    """model.py:204-212 as ONE device stage: the animation-rate dgrad rows (n_frames, 89784) on the GPU and a
    sdfa_amd.seek.SeekPlan -> vertices of every video frame (n_queries, V, 3), cuda."""
    assert _solver is not None, "set_template_mesh first"
    return _solver.get_mesh_seek(anime_rows, plan)


def frame_to_mesh(data_frame, face_data_type):
    x = data_frame if torch.is_tensor(data_frame) else torch.from_numpy(np.asarray(data_frame, np.float32))
    verts, faces = frames_to_mesh(x.reshape(1, -1), face_data_type)
    return verts[0], faces


def renderer(image_size=(512, 512), samples=4, normals="template"):
    """The GPU renderer of the current template (render_py.py:31-39 set_template: scale 0.15 / max|template|), one per
    (image_size, samples, normals), created on first use."""
    assert _solver is not None, "set_template_mesh first"
    key = (tuple(int(x) for x in image_size), int(samples), normals)
    if key not in _renderers:
        from sdfa_amd.render import Renderer
        _renderers[key] = Renderer(_template_verts, _template_faces, image_size=key[0], samples=samples, normals=normals,
                                   device=_solver.device)
    return _renderers[key]


def _device_verts(x, face_data_type):
    """frames_to_mesh without leaving the device: (n, ...) cuda rows -> (n, V, 3) cuda vertices."""
    n = x.shape[0]
    if str(face_data_type).endswith("dgrad_3d"):
        return _solver.get_mesh(x.reshape(n, -1))
    if str(face_data_type).endswith("verts_off_3d") and _source is not None:      # retargeted: offsets -> dgrad -> template solve
        return _solver.get_mesh(source_dgrad(x.reshape(n, -1)))
    if str(face_data_type).endswith("verts_off_3d"):
        return x.reshape(n, -1, 3) + torch.from_numpy(_template_verts).to(x.device)[None]
    return x.reshape(n, -1, 3)


def render_frame(frame, face_data_type, image_size=(512, 512)):
    """frame.py:156 render_frame: one dgrad / offsets / vertex frame -> (H, W, 3) uint8 RGB image (numpy)."""
    assert _solver is not None, "set_template_mesh first"
    x = frame if torch.is_tensor(frame) else torch.from_numpy(np.asarray(frame, np.float32))
    x = x.to(device=_solver.device, dtype=torch.float32).reshape(1, -1)
    return renderer(image_size).render(_device_verts(x, face_data_type))[0].cpu().numpy()


def render_track(anime_rows, plan, image_size=(512, 512), face_data_type="dgrad_3d", n=None, samples=4):
    """model.py:204-223 for one batch of clips as device stages: the animation-rate rows (n_frames, ...) on the GPU and a
    sdfa_amd.seek.SeekPlan -> images of the first `n` (default: all) video frames, (n, H, W, 3) uint8 cuda.  dgrad: seek + solve +
    render; offsets: seek, + template (or, with a source mesh, deform_grad + solve), render -- the vertices never leave the device."""
    assert _solver is not None, "set_template_mesh first"
    if str(face_data_type).endswith("dgrad_3d"):
        verts = _solver.get_mesh_seek(anime_rows, plan)
    else:
        verts = _device_verts(plan.rows(anime_rows.reshape(anime_rows.shape[0], -1)), face_data_type)
    if n is not None:
        verts = verts[:n]
    return renderer(image_size, samples).render(verts)
