"""The refusal transcript of the conv-stack training ABI (include/sdfa_convtrain.h) without a device, call by call: the driver of
tests/test_freqtrain_refusals_cpu.py for the fifth handle over csrc/trainstate.h.  What is expected is not taken from this library:
it is the sibling's pinned table for sdfa_lstmtrain -- the header says the refusals are sdfa_freqtrain.h's, which says they are
that module's -- with this module's words put in place of the BiLSTM's (its name, its noun, its tensors and their sizes, its frame
limit), and then the refusals of the constants (BatchNorm's running statistics), which no sibling has: written out below."""
import ctypes as C

import numpy as np

from sdfa_amd import _lib, convtrain
from test_trainstate_refusals_cpu import EXPECTED as SIBLING, OTHER

lib = _lib.lib
FOREIGN = "_output_module._layers.0.bias"         # the sibling's foreign name for lstmtrain
SHAPES = convtrain.tensor_shapes()
CONSTANTS = convtrain.constant_shapes()
N, MOST = 1, convtrain.MAX_FRAMES


def step_calls(h, n):
    return (("forward", lambda: lib.sdfa_convtrain_forward(h, None, n, None, None, 0, None)),
            ("backward", lambda: lib.sdfa_convtrain_backward(h, None, None, n, None, 0, None)))


def transcript():
    out = {}
    mod = "convtrain"

    def note(case, rc):
        rc = int(rc or 0)
        out[case] = [rc, lib.sdfa_last_error().decode() if rc < 0 else None]

    f = lambda name: getattr(lib, f"sdfa_{mod}_{name}")
    names = [n.encode() for n in SHAPES]
    good, n = names[0], int(np.prod(SHAPES[names[0].decode()]))
    buf = np.zeros(n + 1, np.float32)
    p = buf.ctypes.data

    def per_handle(tag, h):
        for fn, call in step_calls(h, N):
            note(f"{mod}.{tag}.{fn}", call())
        note(f"{mod}.{tag}.adam", f("adam")(h, 1e-4, 0.9, 0.999, 1e-8, None))
        note(f"{mod}.{tag}.adam(beta1=1)", f("adam")(h, 1e-4, 1.0, 0.999, 1e-8, None))
        note(f"{mod}.{tag}.zero_grad", f("zero_grad")(h, None))
        note(f"{mod}.{tag}.get_tensor", f("get_tensor")(h, good, 0, p, n))
        note(f"{mod}.{tag}.get_tensor(what=9)", f("get_tensor")(h, good, 9, p, n))
        note(f"{mod}.{tag}.set_state", f("set_state")(h, good, 2, p, n))
        note(f"{mod}.{tag}.set_grad", f("set_grad")(h, good, p, n))

    f("destroy")(None)                                  # a no-op
    per_handle("null", None)
    note(f"{mod}.null.set_tensor", f("set_tensor")(None, good, p, n))
    note(f"{mod}.null.finalize", f("finalize")(None, None))
    note(f"{mod}.null.numel", f("numel")(None))
    note(f"{mod}.null.workspace_bytes", f("workspace_bytes")(None, N))
    note(f"{mod}.null.step_count", f("step_count")(None))
    note(f"{mod}.null.set_step_count", f("set_step_count")(None, 1))
    h = C.c_void_p(f("create")())
    assert h
    try:
        per_handle("unfinalised", h)
        for fn, call in step_calls(h, 0):                # an unfinalised handle is refused before its N is looked at
            note(f"{mod}.unfinalised.{fn}(N=0)", call())
        note(f"{mod}.finalize(nothing set)", f("finalize")(h, None))
        for tag, name in (("unknown", OTHER.encode()), ("foreign", FOREIGN.encode()), ("empty", b""), ("model-prefixed", b"_model." + good)):
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
        note(f"{mod}.workspace_bytes(MAX + 1)", f("workspace_bytes")(h, MOST + 1))
        note(f"{mod}.workspace_bytes(MAX)", min(f("workspace_bytes")(h, MOST), 1))
        note(f"{mod}.set_step_count(-1)", f("set_step_count")(h, -1))
        note(f"{mod}.step_count", f("step_count")(h))
        note(f"{mod}.set_step_count(5)", f("set_step_count")(h, 5))
        note(f"{mod}.step_count after 5", f("step_count")(h))
        # all tensors but the second: finalize names it
        big = np.zeros(max(int(np.prod(s)) for s in SHAPES.values()), np.float32)
        for i, name in enumerate(names):
            if i != 1:
                note(f"{mod}.set_tensor[{i}]", f("set_tensor")(h, name, big.ctypes.data, int(np.prod(SHAPES[name.decode()]))))
        note(f"{mod}.finalize(second missing)", f("finalize")(h, None))
        note(f"{mod}.unfinalised.adam after that", f("adam")(h, 1e-4, 0.9, 0.999, 1e-8, None))
        # the constants: given like any tensor, required by finalize after the trainable ones, and nothing else
        note(f"{mod}.set_tensor[1]", f("set_tensor")(h, names[1], big.ctypes.data, int(np.prod(SHAPES[names[1].decode()]))))
        note(f"{mod}.finalize(constants missing)", f("finalize")(h, None))
        cn = [c.encode() for c in CONSTANTS]
        note(f"{mod}.constant.set_tensor(numel + 1)", f("set_tensor")(h, cn[0], p, 33))
        note(f"{mod}.constant.set_tensor", f("set_tensor")(h, cn[0], p, 32))
        note(f"{mod}.finalize(second constant missing)", f("finalize")(h, None))
        note(f"{mod}.constant.get_tensor unfinalised", f("get_tensor")(h, cn[0], 0, p, 32))
        for what in (0, 1, 2, 3):
            note(f"{mod}.constant.set_state(what={what})", f("set_state")(h, cn[0], what, p, 32))
        note(f"{mod}.constant.set_grad", f("set_grad")(h, cn[1], p, 32))
    finally:
        f("destroy")(h)                                  # of an unfinalised handle
    return out


def expected():
    """the sibling's lstmtrain table in this module's words, then the constants' lines"""
    first = list(SHAPES)[0]
    n = int(np.prod(SHAPES[first]))
    words = (("_model._audio_encoder._layers.9.weight_ih_l1", "_model." + first),
             ("_audio_encoder._layers.9.weight_ih_l1_reverse", list(SHAPES)[1]),
             ("_audio_encoder._layers.9.weight_ih_l1", first),
             ("layer 1 of the BiLSTM has no tensor", "the conv stack has no tensor"),
             ("lstmtrain", "convtrain"), ("524289", str(n + 1)), ("524288", str(n)), ("524287", str(n - 1)),
             ("3073", str(MOST + 1)), ("3072", str(MOST)))
    out = {}
    for k, (rc, text) in SIBLING.items():
        if not k.startswith("lstmtrain.") or k == "lstmtrain.create(384)":
            continue
        for a, b in words:
            k = k.replace(a, b)
            text = text.replace(a, b) if text is not None else None
        out[k] = [rc, text]
    for i in range(4, len(SHAPES)):                      # 15 tensors, not four
        out[f"convtrain.set_tensor[{i}]"] = [0, None]
    c0, c1 = list(CONSTANTS)[:2]
    is_const = f'convtrain_set_state: "{c0}" is a constant: sdfa_convtrain_set_tensor gives it, before finalize'
    out.update({
        "convtrain.set_tensor[1]": [0, None],
        "convtrain.finalize(constants missing)": [_lib.ESTATE, f'convtrain_finalize: tensor "{c0}" is missing'],
        "convtrain.constant.set_tensor(numel + 1)": [_lib.EINVAL, f'convtrain_set_tensor: "{c0}" has 32 elements, 33 given'],
        "convtrain.constant.set_tensor": [0, None],
        "convtrain.finalize(second constant missing)": [_lib.ESTATE, f'convtrain_finalize: tensor "{c1}" is missing'],
        "convtrain.constant.get_tensor unfinalised": [_lib.ESTATE, "convtrain_get_tensor: the handle is not finalised"],
        **{f"convtrain.constant.set_state(what={w})": [_lib.EINVAL, is_const] for w in (0, 1, 2, 3)},
        "convtrain.constant.set_grad": [_lib.EINVAL, is_const.replace(c0, c1)],
    })
    return out


def test_refusal_transcript():
    got, want = transcript(), expected()
    assert set(got) == set(want), set(got) ^ set(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong
    order = [k for k in got if not k.startswith("convtrain.set_tensor[")]
    assert order == [k for k in want if not k.startswith("convtrain.set_tensor[")]


def test_workspace_bytes():
    """6 MiB kept per frame, the folded weights and dW in the parameter layout, the weight norm's two rows, a partial of the flat
    layout per block of BLOCK_FRAMES frames; every buffer on a 256-byte boundary"""
    h = C.c_void_p(lib.sdfa_convtrain_create())
    try:
        B = convtrain.BLOCK_FRAMES
        got = [int(lib.sdfa_convtrain_workspace_bytes(h, r)) for r in (1, B, B + 1, convtrain.MAX_FRAMES)]
    finally:
        lib.sdfa_convtrain_destroy(h)
    up = lambda floats: -(-floats // 64) * 256
    frame, fixed = 6 * 1024 * 1024, 2 * up(convtrain.NUMEL) + 2 * up(160)
    assert got == [r * frame + fixed + up(-(-r // B) * convtrain.NUMEL) for r in (1, B, B + 1, convtrain.MAX_FRAMES)], got
    assert all(g % 256 == 0 for g in got)
    assert got[-1] < 13 * 2 ** 30
