"""The refusal transcript of the three training ABIs (include/sdfa_{head,attn,lstm}train.h), pinned word for word: every entry point
that can refuse without a device is driven with a null handle, an unfinalised handle, null data pointers, an unknown tensor name and
another module's, a wrong numel, row / frame counts outside the range, a negative step count and a missing tensor at finalize, and
both the return code and the text of sdfa_last_error() are compared with EXPECTED.  The three share csrc/trainstate.h; the table was
written by this driver (`python tests/test_trainstate_refusals_cpu.py` prints it) against the library as it was before they did, when
each module carried its own copy of the checks, so it holds the order of the refusals and their wording.  The workspace sizes are
pinned the same way: the three layouts take their offsets from one allocator."""
import ctypes as C

import numpy as np

from sdfa_amd import _lib, attntrain, headtrain, lstmtrain

lib = _lib.lib
OTHER = "_audio_encoder._layers.3.weight"          # a tensor of the checkpoint that no trainer owns

# module -> (create argument(s), its tensors in slot order, a row / frame count it accepts, its maximum)
MODULES = {
    "headtrain": ((headtrain.HEAD_DGRAD,), headtrain.tensor_shapes("dgrad"), 2, headtrain.MAX_ROWS),
    "attntrain": ((), attntrain.tensor_shapes(), 1, attntrain.MAX_FRAMES),
    "lstmtrain": ((lstmtrain.IN_DIM[1],), lstmtrain.tensor_shapes(1), 1, lstmtrain.MAX_FRAMES),
}
FOREIGN = {"headtrain": attntrain.PREFIX + "b", "attntrain": lstmtrain.PREFIX + "weight_hh_l1", "lstmtrain": "_output_module._layers.0.bias"}


def step_calls(mod, h, N):
    """forward and backward of `mod` with null pointers everywhere but the handle"""
    f = lambda name: getattr(lib, f"sdfa_{mod}_{name}")
    if mod == "headtrain":
        return (("forward", lambda: f("forward")(h, None, None, N, None, None, 0, None)),
                ("backward", lambda: f("backward")(h, None, N, None, None, 0, None)))
    if mod == "attntrain":
        return (("forward", lambda: f("forward")(h, None, N, None, None, None, 0, None)),
                ("backward", lambda: f("backward")(h, None, None, N, None, None, 0, None)))
    return (("forward", lambda: f("forward")(h, None, N, None, None, 0, None)),
            ("backward", lambda: f("backward")(h, None, None, None, N, None, None, 0, None)))


def transcript():
    out = {}

    def note(case, rc):
        rc = int(rc or 0)
        out[case] = [rc, lib.sdfa_last_error().decode() if rc < 0 else None]

    note("headtrain.create(7)", lib.sdfa_headtrain_create(7) or -1)
    note("lstmtrain.create(384)", lib.sdfa_lstmtrain_create(384) or -1)
    for mod, (args, shapes, N, most) in MODULES.items():
        f = lambda name: getattr(lib, f"sdfa_{mod}_{name}")
        names = [n.encode() for n in shapes]
        good, n = names[0], int(np.prod(shapes[names[0].decode()]))
        buf = np.zeros(n + 1, np.float32)
        p = buf.ctypes.data

        def per_handle(tag, h):
            for fn, call in step_calls(mod, h, N):
                note(f"{mod}.{tag}.{fn}", call())
            note(f"{mod}.{tag}.adam", f("adam")(h, 1e-4, 0.9, 0.999, 1e-8, None))
            note(f"{mod}.{tag}.adam(beta1=1)", f("adam")(h, 1e-4, 1.0, 0.999, 1e-8, None))
            note(f"{mod}.{tag}.zero_grad", f("zero_grad")(h, None))
            note(f"{mod}.{tag}.get_tensor", f("get_tensor")(h, good, 0, p, n))
            note(f"{mod}.{tag}.get_tensor(what=9)", f("get_tensor")(h, good, 9, p, n))
            note(f"{mod}.{tag}.set_state", f("set_state")(h, good, 2, p, n))
            note(f"{mod}.{tag}.set_grad", f("set_grad")(h, good, p, n))

        lib_destroy = f("destroy")
        lib_destroy(None)                                   # a no-op
        per_handle("null", None)
        note(f"{mod}.null.set_tensor", f("set_tensor")(None, good, p, n))
        note(f"{mod}.null.finalize", f("finalize")(None, None))
        note(f"{mod}.null.numel", f("numel")(None))
        note(f"{mod}.null.workspace_bytes", f("workspace_bytes")(None, N))
        note(f"{mod}.null.step_count", f("step_count")(None))
        note(f"{mod}.null.set_step_count", f("set_step_count")(None, 1))
        if mod == "headtrain":
            note("headtrain.null.coef_dim", lib.sdfa_headtrain_coef_dim(None))

        h = C.c_void_p(f("create")(*args))
        assert h
        try:
            per_handle("unfinalised", h)
            for fn, call in step_calls(mod, h, 0):           # an unfinalised handle is refused before its N is looked at
                note(f"{mod}.unfinalised.{fn}(N=0)", call())
            note(f"{mod}.finalize(nothing set)", f("finalize")(h, None))
            for tag, name in (("unknown", OTHER.encode()), ("foreign", FOREIGN[mod].encode()), ("empty", b""), ("model-prefixed", b"_model." + good)):
                note(f"{mod}.set_tensor({tag} name)", f("set_tensor")(h, name, p, n))
                note(f"{mod}.get_tensor({tag} name)", f("get_tensor")(h, name, 0, p, n))
                note(f"{mod}.set_state({tag} name)", f("set_state")(h, name, 0, p, n))
                note(f"{mod}.set_grad({tag} name)", f("set_grad")(h, name, p, n))
            note(f"{mod}.set_tensor(null name)", f("set_tensor")(h, None, p, n))
            note(f"{mod}.set_tensor(null data)", f("set_tensor")(h, good, None, n))
            note(f"{mod}.set_tensor(null data, unknown name)", f("set_tensor")(h, OTHER.encode(), None, n))
            note(f"{mod}.get_tensor(null data)", f("get_tensor")(h, good, 0, None, n))
            note(f"{mod}.set_state(null data)", f("set_state")(h, good, 0, None, n))
            note(f"{mod}.set_grad(null data)", f("set_grad")(h, good, None, n))
            note(f"{mod}.set_tensor(numel - 1)", f("set_tensor")(h, good, p, n - 1))
            note(f"{mod}.set_tensor(numel + 1)", f("set_tensor")(h, good, p, n + 1))
            note(f"{mod}.get_tensor(numel + 1)", f("get_tensor")(h, good, 0, p, n + 1))
            note(f"{mod}.set_state(numel 0)", f("set_state")(h, good, 0, p, 0))
            note(f"{mod}.set_tensor", f("set_tensor")(h, good, p, n))
            note(f"{mod}.workspace_bytes(0)", f("workspace_bytes")(h, 0))
            note(f"{mod}.workspace_bytes(-1)", f("workspace_bytes")(h, -1))
            note(f"{mod}.workspace_bytes(MAX + 1)", f("workspace_bytes")(h, most + 1))
            note(f"{mod}.workspace_bytes(MAX)", min(f("workspace_bytes")(h, most), 1))
            if mod == "headtrain":
                note("headtrain.workspace_bytes(1)", lib.sdfa_headtrain_workspace_bytes(h, 1))
                note("headtrain.workspace_bytes(3)", lib.sdfa_headtrain_workspace_bytes(h, 3))      # an odd count is the forward's to refuse
            note(f"{mod}.set_step_count(-1)", f("set_step_count")(h, -1))
            note(f"{mod}.step_count", f("step_count")(h))
            note(f"{mod}.set_step_count(5)", f("set_step_count")(h, 5))
            note(f"{mod}.step_count after 5", f("step_count")(h))
            # all tensors but the second: finalize names it
            big = np.zeros(max(int(np.prod(s)) for s in shapes.values()), np.float32)
            for i, name in enumerate(names):
                if i != 1:
                    note(f"{mod}.set_tensor[{i}]", f("set_tensor")(h, name, big.ctypes.data, int(np.prod(shapes[name.decode()]))))
            note(f"{mod}.finalize(second missing)", f("finalize")(h, None))
            note(f"{mod}.unfinalised.adam after that", f("adam")(h, 1e-4, 0.9, 0.999, 1e-8, None))
        finally:
            lib_destroy(h)                                  # of an unfinalised handle
    return out


def workspace_bytes():
    out = {}
    for head, code in (("dgrad", headtrain.HEAD_DGRAD), ("offsets", headtrain.HEAD_OFFSETS)):
        h = C.c_void_p(lib.sdfa_headtrain_create(code))
        out[f"headtrain.{head}"] = [int(lib.sdfa_headtrain_workspace_bytes(h, r)) for r in (2, 64, 66)]
        lib.sdfa_headtrain_destroy(h)
    h = C.c_void_p(lib.sdfa_attntrain_create())
    out["attntrain"] = [int(lib.sdfa_attntrain_workspace_bytes(h, r)) for r in (1, 16, 17)]
    lib.sdfa_attntrain_destroy(h)
    for layer, width in lstmtrain.IN_DIM.items():
        h = C.c_void_p(lib.sdfa_lstmtrain_create(width))
        out[f"lstmtrain.l{layer}"] = [int(lib.sdfa_lstmtrain_workspace_bytes(h, r)) for r in (1, 32, 33)]
        lib.sdfa_lstmtrain_destroy(h)
    return out


EXPECTED = {'headtrain.create(7)': [-1, 'headtrain_create: unknown head 7'],
 'lstmtrain.create(384)': [-1, "lstmtrain_create: input width 384; the encoder's BiLSTM has 256 (layer 0) and 512 (layer 1)"],
 'headtrain.null.forward': [-1, 'headtrain_forward: null handle'],
 'headtrain.null.backward': [-1, 'headtrain_backward: null handle'],
 'headtrain.null.adam': [-1, 'headtrain_adam: null handle'],
 'headtrain.null.adam(beta1=1)': [-1, 'headtrain_adam: null handle'],
 'headtrain.null.zero_grad': [-1, 'headtrain_zero_grad: null handle'],
 'headtrain.null.get_tensor': [-1, 'headtrain_get_tensor: null pointer'],
 'headtrain.null.get_tensor(what=9)': [-1, 'headtrain_get_tensor: null pointer'],
 'headtrain.null.set_state': [-1, 'headtrain_set_state: null pointer'],
 'headtrain.null.set_grad': [-1, 'headtrain_set_state: null pointer'],
 'headtrain.null.set_tensor': [-1, 'headtrain_set_tensor: null pointer'],
 'headtrain.null.finalize': [-1, 'headtrain_finalize: null handle'],
 'headtrain.null.numel': [-1, 'headtrain_numel: null handle'],
 'headtrain.null.workspace_bytes': [-1, 'headtrain_workspace_bytes: null handle'],
 'headtrain.null.step_count': [-1, 'headtrain_step_count: null handle'],
 'headtrain.null.set_step_count': [-1, 'headtrain_set_step_count: null handle'],
 'headtrain.null.coef_dim': [-1, 'headtrain_coef_dim: null handle'],
 'headtrain.unfinalised.forward': [-4, 'headtrain_forward: the handle is not finalised'],
 'headtrain.unfinalised.backward': [-4, 'headtrain_backward: the handle is not finalised'],
 'headtrain.unfinalised.adam': [-4, 'headtrain_adam: the handle is not finalised'],
 'headtrain.unfinalised.adam(beta1=1)': [-4, 'headtrain_adam: the handle is not finalised'],
 'headtrain.unfinalised.zero_grad': [-4, 'headtrain_zero_grad: the handle is not finalised'],
 'headtrain.unfinalised.get_tensor': [-4, 'headtrain_get_tensor: the handle is not finalised'],
 'headtrain.unfinalised.get_tensor(what=9)': [-4, 'headtrain_get_tensor: the handle is not finalised'],
 'headtrain.unfinalised.set_state': [-4, 'headtrain_set_state: the handle is not finalised'],
 'headtrain.unfinalised.set_grad': [-4, 'headtrain_set_state: the handle is not finalised'],
 'headtrain.unfinalised.forward(N=0)': [-4, 'headtrain_forward: the handle is not finalised'],
 'headtrain.unfinalised.backward(N=0)': [-4, 'headtrain_backward: the handle is not finalised'],
 'headtrain.finalize(nothing set)': [-4, 'headtrain_finalize: tensor "_output_module._layers.0.weight_g" is missing'],
 'headtrain.set_tensor(unknown name)': [-1, 'headtrain_set_tensor: the head has no tensor "_audio_encoder._layers.3.weight"'],
 'headtrain.get_tensor(unknown name)': [-1, 'headtrain_get_tensor: the head has no tensor "_audio_encoder._layers.3.weight"'],
 'headtrain.set_state(unknown name)': [-1, 'headtrain_set_state: the head has no tensor "_audio_encoder._layers.3.weight"'],
 'headtrain.set_grad(unknown name)': [-1, 'headtrain_set_state: the head has no tensor "_audio_encoder._layers.3.weight"'],
 'headtrain.set_tensor(foreign name)': [-1, 'headtrain_set_tensor: the head has no tensor "_audio_encoder._layers.10.b"'],
 'headtrain.get_tensor(foreign name)': [-1, 'headtrain_get_tensor: the head has no tensor "_audio_encoder._layers.10.b"'],
 'headtrain.set_state(foreign name)': [-1, 'headtrain_set_state: the head has no tensor "_audio_encoder._layers.10.b"'],
 'headtrain.set_grad(foreign name)': [-1, 'headtrain_set_state: the head has no tensor "_audio_encoder._layers.10.b"'],
 'headtrain.set_tensor(empty name)': [-1, 'headtrain_set_tensor: the head has no tensor ""'],
 'headtrain.get_tensor(empty name)': [-1, 'headtrain_get_tensor: the head has no tensor ""'],
 'headtrain.set_state(empty name)': [-1, 'headtrain_set_state: the head has no tensor ""'],
 'headtrain.set_grad(empty name)': [-1, 'headtrain_set_state: the head has no tensor ""'],
 'headtrain.set_tensor(model-prefixed name)': [-1, 'headtrain_set_tensor: the head has no tensor "_model._output_module._layers.0.weight_g"'],
 'headtrain.get_tensor(model-prefixed name)': [-1, 'headtrain_get_tensor: the head has no tensor "_model._output_module._layers.0.weight_g"'],
 'headtrain.set_state(model-prefixed name)': [-1, 'headtrain_set_state: the head has no tensor "_model._output_module._layers.0.weight_g"'],
 'headtrain.set_grad(model-prefixed name)': [-1, 'headtrain_set_state: the head has no tensor "_model._output_module._layers.0.weight_g"'],
 'headtrain.set_tensor(null name)': [-1, 'headtrain_set_tensor: null pointer'],
 'headtrain.set_tensor(null data)': [-1, 'headtrain_set_tensor: null pointer'],
 'headtrain.set_tensor(null data, unknown name)': [-1, 'headtrain_set_tensor: null pointer'],
 'headtrain.get_tensor(null data)': [-1, 'headtrain_get_tensor: null pointer'],
 'headtrain.set_state(null data)': [-1, 'headtrain_set_state: null pointer'],
 'headtrain.set_grad(null data)': [-1, 'headtrain_set_state: null pointer'],
 'headtrain.set_tensor(numel - 1)': [-1, 'headtrain_set_tensor: "_output_module._layers.0.weight_g" has 512 elements, 511 given'],
 'headtrain.set_tensor(numel + 1)': [-1, 'headtrain_set_tensor: "_output_module._layers.0.weight_g" has 512 elements, 513 given'],
 'headtrain.get_tensor(numel + 1)': [-1, 'headtrain_get_tensor: "_output_module._layers.0.weight_g" has 512 elements, 513 given'],
 'headtrain.set_state(numel 0)': [-1, 'headtrain_set_state: "_output_module._layers.0.weight_g" has 512 elements, 0 given'],
 'headtrain.set_tensor': [0, None],
 'headtrain.workspace_bytes(0)': [-1, 'headtrain_workspace_bytes: 0 rows outside 2 .. 2097152'],
 'headtrain.workspace_bytes(-1)': [-1, 'headtrain_workspace_bytes: -1 rows outside 2 .. 2097152'],
 'headtrain.workspace_bytes(MAX + 1)': [-1, 'headtrain_workspace_bytes: 2097153 rows outside 2 .. 2097152'],
 'headtrain.workspace_bytes(MAX)': [1, None],
 'headtrain.workspace_bytes(1)': [-1, 'headtrain_workspace_bytes: 1 rows outside 2 .. 2097152'],
 'headtrain.workspace_bytes(3)': [55552, None],
 'headtrain.set_step_count(-1)': [-1, 'headtrain_set_step_count: -1 is negative'],
 'headtrain.step_count': [0, None],
 'headtrain.set_step_count(5)': [0, None],
 'headtrain.step_count after 5': [5, None],
 'headtrain.set_tensor[0]': [0, None],
 'headtrain.set_tensor[2]': [0, None],
 'headtrain.set_tensor[3]': [0, None],
 'headtrain.set_tensor[4]': [0, None],
 'headtrain.set_tensor[5]': [0, None],
 'headtrain.set_tensor[6]': [0, None],
 'headtrain.set_tensor[7]': [0, None],
 'headtrain.set_tensor[8]': [0, None],
 'headtrain.set_tensor[9]': [0, None],
 'headtrain.set_tensor[10]': [0, None],
 'headtrain.set_tensor[11]': [0, None],
 'headtrain.set_tensor[12]': [0, None],
 'headtrain.set_tensor[13]': [0, None],
 'headtrain.set_tensor[14]': [0, None],
 'headtrain.set_tensor[15]': [0, None],
 'headtrain.set_tensor[16]': [0, None],
 'headtrain.set_tensor[17]': [0, None],
 'headtrain.set_tensor[18]': [0, None],
 'headtrain.set_tensor[19]': [0, None],
 'headtrain.set_tensor[20]': [0, None],
 'headtrain.finalize(second missing)': [-4, 'headtrain_finalize: tensor "_output_module._layers.0.weight_v" is missing'],
 'headtrain.unfinalised.adam after that': [-4, 'headtrain_adam: the handle is not finalised'],
 'attntrain.null.forward': [-1, 'attntrain_forward: null handle'],
 'attntrain.null.backward': [-1, 'attntrain_backward: null handle'],
 'attntrain.null.adam': [-1, 'attntrain_adam: null handle'],
 'attntrain.null.adam(beta1=1)': [-1, 'attntrain_adam: null handle'],
 'attntrain.null.zero_grad': [-1, 'attntrain_zero_grad: null handle'],
 'attntrain.null.get_tensor': [-1, 'attntrain_get_tensor: null pointer'],
 'attntrain.null.get_tensor(what=9)': [-1, 'attntrain_get_tensor: null pointer'],
 'attntrain.null.set_state': [-1, 'attntrain_set_state: null pointer'],
 'attntrain.null.set_grad': [-1, 'attntrain_set_state: null pointer'],
 'attntrain.null.set_tensor': [-1, 'attntrain_set_tensor: null pointer'],
 'attntrain.null.finalize': [-1, 'attntrain_finalize: null handle'],
 'attntrain.null.numel': [-1, 'attntrain_numel: null handle'],
 'attntrain.null.workspace_bytes': [-1, 'attntrain_workspace_bytes: null handle'],
 'attntrain.null.step_count': [-1, 'attntrain_step_count: null handle'],
 'attntrain.null.set_step_count': [-1, 'attntrain_set_step_count: null handle'],
 'attntrain.unfinalised.forward': [-4, 'attntrain_forward: the handle is not finalised'],
 'attntrain.unfinalised.backward': [-4, 'attntrain_backward: the handle is not finalised'],
 'attntrain.unfinalised.adam': [-4, 'attntrain_adam: the handle is not finalised'],
 'attntrain.unfinalised.adam(beta1=1)': [-4, 'attntrain_adam: the handle is not finalised'],
 'attntrain.unfinalised.zero_grad': [-4, 'attntrain_zero_grad: the handle is not finalised'],
 'attntrain.unfinalised.get_tensor': [-4, 'attntrain_get_tensor: the handle is not finalised'],
 'attntrain.unfinalised.get_tensor(what=9)': [-4, 'attntrain_get_tensor: the handle is not finalised'],
 'attntrain.unfinalised.set_state': [-4, 'attntrain_set_state: the handle is not finalised'],
 'attntrain.unfinalised.set_grad': [-4, 'attntrain_set_state: the handle is not finalised'],
 'attntrain.unfinalised.forward(N=0)': [-4, 'attntrain_forward: the handle is not finalised'],
 'attntrain.unfinalised.backward(N=0)': [-4, 'attntrain_backward: the handle is not finalised'],
 'attntrain.finalize(nothing set)': [-4, 'attntrain_finalize: tensor "_audio_encoder._layers.10._conv_query.weight" is missing'],
 'attntrain.set_tensor(unknown name)': [-1, 'attntrain_set_tensor: the attention layer has no tensor "_audio_encoder._layers.3.weight"'],
 'attntrain.get_tensor(unknown name)': [-1, 'attntrain_get_tensor: the attention layer has no tensor "_audio_encoder._layers.3.weight"'],
 'attntrain.set_state(unknown name)': [-1, 'attntrain_set_state: the attention layer has no tensor "_audio_encoder._layers.3.weight"'],
 'attntrain.set_grad(unknown name)': [-1, 'attntrain_set_state: the attention layer has no tensor "_audio_encoder._layers.3.weight"'],
 'attntrain.set_tensor(foreign name)': [-1, 'attntrain_set_tensor: the attention layer has no tensor "_audio_encoder._layers.9.weight_hh_l1"'],
 'attntrain.get_tensor(foreign name)': [-1, 'attntrain_get_tensor: the attention layer has no tensor "_audio_encoder._layers.9.weight_hh_l1"'],
 'attntrain.set_state(foreign name)': [-1, 'attntrain_set_state: the attention layer has no tensor "_audio_encoder._layers.9.weight_hh_l1"'],
 'attntrain.set_grad(foreign name)': [-1, 'attntrain_set_state: the attention layer has no tensor "_audio_encoder._layers.9.weight_hh_l1"'],
 'attntrain.set_tensor(empty name)': [-1, 'attntrain_set_tensor: the attention layer has no tensor ""'],
 'attntrain.get_tensor(empty name)': [-1, 'attntrain_get_tensor: the attention layer has no tensor ""'],
 'attntrain.set_state(empty name)': [-1, 'attntrain_set_state: the attention layer has no tensor ""'],
 'attntrain.set_grad(empty name)': [-1, 'attntrain_set_state: the attention layer has no tensor ""'],
 'attntrain.set_tensor(model-prefixed name)': [-1, 'attntrain_set_tensor: the attention layer has no tensor "_model._audio_encoder._layers.10._conv_query.weight"'],
 'attntrain.get_tensor(model-prefixed name)': [-1, 'attntrain_get_tensor: the attention layer has no tensor "_model._audio_encoder._layers.10._conv_query.weight"'],
 'attntrain.set_state(model-prefixed name)': [-1, 'attntrain_set_state: the attention layer has no tensor "_model._audio_encoder._layers.10._conv_query.weight"'],
 'attntrain.set_grad(model-prefixed name)': [-1, 'attntrain_set_state: the attention layer has no tensor "_model._audio_encoder._layers.10._conv_query.weight"'],
 'attntrain.set_tensor(null name)': [-1, 'attntrain_set_tensor: null pointer'],
 'attntrain.set_tensor(null data)': [-1, 'attntrain_set_tensor: null pointer'],
 'attntrain.set_tensor(null data, unknown name)': [-1, 'attntrain_set_tensor: null pointer'],
 'attntrain.get_tensor(null data)': [-1, 'attntrain_get_tensor: null pointer'],
 'attntrain.set_state(null data)': [-1, 'attntrain_set_state: null pointer'],
 'attntrain.set_grad(null data)': [-1, 'attntrain_set_state: null pointer'],
 'attntrain.set_tensor(numel - 1)': [-1, 'attntrain_set_tensor: "_audio_encoder._layers.10._conv_query.weight" has 786432 elements, 786431 given'],
 'attntrain.set_tensor(numel + 1)': [-1, 'attntrain_set_tensor: "_audio_encoder._layers.10._conv_query.weight" has 786432 elements, 786433 given'],
 'attntrain.get_tensor(numel + 1)': [-1, 'attntrain_get_tensor: "_audio_encoder._layers.10._conv_query.weight" has 786432 elements, 786433 given'],
 'attntrain.set_state(numel 0)': [-1, 'attntrain_set_state: "_audio_encoder._layers.10._conv_query.weight" has 786432 elements, 0 given'],
 'attntrain.set_tensor': [0, None],
 'attntrain.workspace_bytes(0)': [-1, 'attntrain_workspace_bytes: 0 frames outside 1 .. 32768'],
 'attntrain.workspace_bytes(-1)': [-1, 'attntrain_workspace_bytes: -1 frames outside 1 .. 32768'],
 'attntrain.workspace_bytes(MAX + 1)': [-1, 'attntrain_workspace_bytes: 32769 frames outside 1 .. 32768'],
 'attntrain.workspace_bytes(MAX)': [1, None],
 'attntrain.set_step_count(-1)': [-1, 'attntrain_set_step_count: -1 is negative'],
 'attntrain.step_count': [0, None],
 'attntrain.set_step_count(5)': [0, None],
 'attntrain.step_count after 5': [5, None],
 'attntrain.set_tensor[0]': [0, None],
 'attntrain.set_tensor[2]': [0, None],
 'attntrain.set_tensor[3]': [0, None],
 'attntrain.set_tensor[4]': [0, None],
 'attntrain.finalize(second missing)': [-4, 'attntrain_finalize: tensor "_audio_encoder._layers.10.proj_qry.weight" is missing'],
 'attntrain.unfinalised.adam after that': [-4, 'attntrain_adam: the handle is not finalised'],
 'lstmtrain.null.forward': [-1, 'lstmtrain_forward: null handle'],
 'lstmtrain.null.backward': [-1, 'lstmtrain_backward: null handle'],
 'lstmtrain.null.adam': [-1, 'lstmtrain_adam: null handle'],
 'lstmtrain.null.adam(beta1=1)': [-1, 'lstmtrain_adam: null handle'],
 'lstmtrain.null.zero_grad': [-1, 'lstmtrain_zero_grad: null handle'],
 'lstmtrain.null.get_tensor': [-1, 'lstmtrain_get_tensor: null pointer'],
 'lstmtrain.null.get_tensor(what=9)': [-1, 'lstmtrain_get_tensor: null pointer'],
 'lstmtrain.null.set_state': [-1, 'lstmtrain_set_state: null pointer'],
 'lstmtrain.null.set_grad': [-1, 'lstmtrain_set_state: null pointer'],
 'lstmtrain.null.set_tensor': [-1, 'lstmtrain_set_tensor: null pointer'],
 'lstmtrain.null.finalize': [-1, 'lstmtrain_finalize: null handle'],
 'lstmtrain.null.numel': [-1, 'lstmtrain_numel: null handle'],
 'lstmtrain.null.workspace_bytes': [-1, 'lstmtrain_workspace_bytes: null handle'],
 'lstmtrain.null.step_count': [-1, 'lstmtrain_step_count: null handle'],
 'lstmtrain.null.set_step_count': [-1, 'lstmtrain_set_step_count: null handle'],
 'lstmtrain.unfinalised.forward': [-4, 'lstmtrain_forward: the handle is not finalised'],
 'lstmtrain.unfinalised.backward': [-4, 'lstmtrain_backward: the handle is not finalised'],
 'lstmtrain.unfinalised.adam': [-4, 'lstmtrain_adam: the handle is not finalised'],
 'lstmtrain.unfinalised.adam(beta1=1)': [-4, 'lstmtrain_adam: the handle is not finalised'],
 'lstmtrain.unfinalised.zero_grad': [-4, 'lstmtrain_zero_grad: the handle is not finalised'],
 'lstmtrain.unfinalised.get_tensor': [-4, 'lstmtrain_get_tensor: the handle is not finalised'],
 'lstmtrain.unfinalised.get_tensor(what=9)': [-4, 'lstmtrain_get_tensor: the handle is not finalised'],
 'lstmtrain.unfinalised.set_state': [-4, 'lstmtrain_set_state: the handle is not finalised'],
 'lstmtrain.unfinalised.set_grad': [-4, 'lstmtrain_set_state: the handle is not finalised'],
 'lstmtrain.unfinalised.forward(N=0)': [-4, 'lstmtrain_forward: the handle is not finalised'],
 'lstmtrain.unfinalised.backward(N=0)': [-4, 'lstmtrain_backward: the handle is not finalised'],
 'lstmtrain.finalize(nothing set)': [-4, 'lstmtrain_finalize: tensor "_audio_encoder._layers.9.weight_ih_l1" is missing'],
 'lstmtrain.set_tensor(unknown name)': [-1, 'lstmtrain_set_tensor: layer 1 of the BiLSTM has no tensor "_audio_encoder._layers.3.weight"'],
 'lstmtrain.get_tensor(unknown name)': [-1, 'lstmtrain_get_tensor: layer 1 of the BiLSTM has no tensor "_audio_encoder._layers.3.weight"'],
 'lstmtrain.set_state(unknown name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor "_audio_encoder._layers.3.weight"'],
 'lstmtrain.set_grad(unknown name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor "_audio_encoder._layers.3.weight"'],
 'lstmtrain.set_tensor(foreign name)': [-1, 'lstmtrain_set_tensor: layer 1 of the BiLSTM has no tensor "_output_module._layers.0.bias"'],
 'lstmtrain.get_tensor(foreign name)': [-1, 'lstmtrain_get_tensor: layer 1 of the BiLSTM has no tensor "_output_module._layers.0.bias"'],
 'lstmtrain.set_state(foreign name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor "_output_module._layers.0.bias"'],
 'lstmtrain.set_grad(foreign name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor "_output_module._layers.0.bias"'],
 'lstmtrain.set_tensor(empty name)': [-1, 'lstmtrain_set_tensor: layer 1 of the BiLSTM has no tensor ""'],
 'lstmtrain.get_tensor(empty name)': [-1, 'lstmtrain_get_tensor: layer 1 of the BiLSTM has no tensor ""'],
 'lstmtrain.set_state(empty name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor ""'],
 'lstmtrain.set_grad(empty name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor ""'],
 'lstmtrain.set_tensor(model-prefixed name)': [-1, 'lstmtrain_set_tensor: layer 1 of the BiLSTM has no tensor "_model._audio_encoder._layers.9.weight_ih_l1"'],
 'lstmtrain.get_tensor(model-prefixed name)': [-1, 'lstmtrain_get_tensor: layer 1 of the BiLSTM has no tensor "_model._audio_encoder._layers.9.weight_ih_l1"'],
 'lstmtrain.set_state(model-prefixed name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor "_model._audio_encoder._layers.9.weight_ih_l1"'],
 'lstmtrain.set_grad(model-prefixed name)': [-1, 'lstmtrain_set_state: layer 1 of the BiLSTM has no tensor "_model._audio_encoder._layers.9.weight_ih_l1"'],
 'lstmtrain.set_tensor(null name)': [-1, 'lstmtrain_set_tensor: null pointer'],
 'lstmtrain.set_tensor(null data)': [-1, 'lstmtrain_set_tensor: null pointer'],
 'lstmtrain.set_tensor(null data, unknown name)': [-1, 'lstmtrain_set_tensor: null pointer'],
 'lstmtrain.get_tensor(null data)': [-1, 'lstmtrain_get_tensor: null pointer'],
 'lstmtrain.set_state(null data)': [-1, 'lstmtrain_set_state: null pointer'],
 'lstmtrain.set_grad(null data)': [-1, 'lstmtrain_set_state: null pointer'],
 'lstmtrain.set_tensor(numel - 1)': [-1, 'lstmtrain_set_tensor: "_audio_encoder._layers.9.weight_ih_l1" has 524288 elements, 524287 given'],
 'lstmtrain.set_tensor(numel + 1)': [-1, 'lstmtrain_set_tensor: "_audio_encoder._layers.9.weight_ih_l1" has 524288 elements, 524289 given'],
 'lstmtrain.get_tensor(numel + 1)': [-1, 'lstmtrain_get_tensor: "_audio_encoder._layers.9.weight_ih_l1" has 524288 elements, 524289 given'],
 'lstmtrain.set_state(numel 0)': [-1, 'lstmtrain_set_state: "_audio_encoder._layers.9.weight_ih_l1" has 524288 elements, 0 given'],
 'lstmtrain.set_tensor': [0, None],
 'lstmtrain.workspace_bytes(0)': [-1, 'lstmtrain_workspace_bytes: 0 frames outside 1 .. 3072'],
 'lstmtrain.workspace_bytes(-1)': [-1, 'lstmtrain_workspace_bytes: -1 frames outside 1 .. 3072'],
 'lstmtrain.workspace_bytes(MAX + 1)': [-1, 'lstmtrain_workspace_bytes: 3073 frames outside 1 .. 3072'],
 'lstmtrain.workspace_bytes(MAX)': [1, None],
 'lstmtrain.set_step_count(-1)': [-1, 'lstmtrain_set_step_count: -1 is negative'],
 'lstmtrain.step_count': [0, None],
 'lstmtrain.set_step_count(5)': [0, None],
 'lstmtrain.step_count after 5': [5, None],
 'lstmtrain.set_tensor[0]': [0, None],
 'lstmtrain.set_tensor[2]': [0, None],
 'lstmtrain.set_tensor[3]': [0, None],
 'lstmtrain.finalize(second missing)': [-4, 'lstmtrain_finalize: tensor "_audio_encoder._layers.9.weight_ih_l1_reverse" is missing'],
 'lstmtrain.unfinalised.adam after that': [-4, 'lstmtrain_adam: the handle is not finalised']}
WORKSPACE_BYTES = {'headtrain.dgrad': [37120, 1179904, 1217024],
 'headtrain.offsets': [16640, 524544, 541184],
 'attntrain': [340736, 1504256, 1844992],
 'lstmtrain.l0': [9043968, 29360128, 34209792],
 'lstmtrain.l1': [11141120, 31457280, 38404096]}


def test_refusal_transcript():
    got = transcript()
    assert list(got) == list(EXPECTED)
    wrong = {k: (got[k], EXPECTED[k]) for k in got if got[k] != EXPECTED[k]}
    assert not wrong, wrong


def test_workspace_bytes():
    assert workspace_bytes() == WORKSPACE_BYTES


if __name__ == "__main__":
    import pprint
    print("EXPECTED = " + pprint.pformat(transcript(), width=200, sort_dicts=False))
    print("WORKSPACE_BYTES = " + pprint.pformat(workspace_bytes(), width=200, sort_dicts=False))
