"""What the three GPU trainers take from their shared base (sdfa_amd/_trainer.py over csrc/trainstate.h): state_dict() of a trainer
after two steps, loaded into a trainer built from other weights and other Adam arguments, makes the two indistinguishable -- a third
forward / backward / step on the same seeded inputs leaves parameters, gradients, both moments and the step count bitwise equal (the
same kernels on the same bits: no tolerance applies).  And a backward after step() without a new forward is refused: the step
invalidates the kept forward, once, in the core.

Shapes: HeadTrainer, both heads, N = 2 (one [a; b] pair); AttnTrainer N = 1 and 17 (one frame past a 16-frame block); LstmTrainer,
both layers, N = 1 and 33 (one frame past a 32-frame block)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [("head", "dgrad", 2), ("head", "offsets", 2), ("attn", None, 1), ("attn", None, 17),
         ("lstm", 0, 1), ("lstm", 0, 33), ("lstm", 1, 1), ("lstm", 1, 33)]


@functools.lru_cache(maxsize=None)
def weights(head, seed):
    from sdfa_amd import synth
    return synth.make_state_dict(head, seed)


def build(kind, arg, seed, **kw):
    from sdfa_amd.attntrain import AttnTrainer
    from sdfa_amd.headtrain import HeadTrainer
    from sdfa_amd.lstmtrain import LstmTrainer
    if kind == "head":
        return HeadTrainer(weights(arg, seed), arg, **kw)
    if kind == "attn":
        return AttnTrainer(weights("offsets", seed), **kw)
    return LstmTrainer(weights("offsets", seed), layer=arg, **kw)


def inputs(kind, tr, N, t):
    """the seeded arguments of forward and of backward in round t"""
    g = torch.Generator().manual_seed(1000 * N + t)
    rand = lambda *shape: torch.randn(*shape, generator=g).cuda()
    if kind == "head":
        return (rand(N, 512), torch.randint(0, 8, (N,), generator=g)), rand(N, tr.coef_dim)
    if kind == "attn":
        return (rand(N, 64, 512),), rand(N, 512)
    return (rand(N, 64, tr.in_dim),), rand(N, 64, 512)


def one_round(kind, tr, N, t):
    fwd, grad = inputs(kind, tr, N, t)
    tr.forward(*fwd)
    tr.backward(grad)
    tr.step()
    return grad


def same_bits(a, b, what):
    assert list(a) == list(b), what
    for name in a:
        assert np.isfinite(a[name]).all(), (what, name)
        assert a[name].dtype == b[name].dtype == np.float32 and a[name].shape == b[name].shape, (what, name)
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), (what, name)


@pytest.mark.parametrize("kind,arg,N", CASES)
def test_loaded_state_continues_bitwise(kind, arg, N):
    from sdfa_amd._lib import SdfaError
    a = build(kind, arg, 11, lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    for t in range(2):
        one_round(kind, a, N, t)
    state = a.state_dict()
    assert state["step"] == a.step_count == 2

    b = build(kind, arg, 12)
    pa, pb = a.parameters(), b.parameters()
    assert all(not np.array_equal(pa[n], pb[n]) for n in pa)          # other weights, default Adam arguments, no step taken
    assert b.step_count == 0 and (b.lr, b.betas, b.eps) != (a.lr, a.betas, a.eps)
    assert b.load_state_dict(state) is b
    assert b.step_count == 2 and (b.lr, b.betas, b.eps) == (a.lr, a.betas, a.eps)
    same_bits(a.parameters(), b.parameters(), "loaded parameters")

    grad = one_round(kind, a, N, 2)
    one_round(kind, b, N, 2)
    assert a.step_count == b.step_count == 3
    same_bits(a.parameters(), b.parameters(), "parameters")
    same_bits(a.grads(), b.grads(), "gradients")
    for ma, mb, what in zip(a.moments(), b.moments(), ("exp_avg", "exp_avg_sq")):
        same_bits(ma, mb, what)
    assert any(np.any(v != 0) for v in a.grads().values()) and any(np.any(v != 0) for v in a.moments()[1].values())

    for tr in (a, b):                                                  # the step has invalidated the kept forward
        with pytest.raises(SdfaError, match="no forward of"):
            tr.backward(grad)
