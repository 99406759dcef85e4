"""Float64 restatement of the masked two-layer BiLSTM training step: layer 0 and layer 1 of the encoder's layer 9 with nn.LSTM's
inter-layer dropout between them and BOTH layers trained, as train_step(bilstm_bottom=True) runs it.
Composed from the layer functions of tests/lstmtrain_ref64.py (`run`, `adam`), which are imported and not edited:

    forward     Y0 = layer0(X0) ;  X1 = Y0 * keep ;  H = layer1(X1)
    backward    layer 1 on dH gives its gradients and dX1 ;  dY0 = dX1 * keep ;  layer 0 on dY0 gives its gradients
    Adam        every tensor of both layers, headtrain_ref64.adam

`keep` is the multiplier the device applies, given as float32: 0 or 1 / (1 - p) (all ones: no dropout).  It is an exact
constant, so kappa passes through it by lstmtrain_ref64's rule for a product with one exact factor: the incoming sigma times
|keep|, plus U |product| for the rounding of the float32 product where there is one -- none where keep is 0 or a power of two,
where the float32 product is exact.  Errors of the inputs enter through `kX0` (X0 as another stage's output), `kdH` (dH as the
attention layer's dH) and `dparams`, as in lstmtrain_ref64.

`flaw` builds deliberately wrong models, the controls: "mask_not_in_backward" (dY0 = dX1, the forward masked),
"mask_twice" (keep applied twice, in both passes), "layer0_untrained" (layer 0's gradients are zero: its parameters stay),
"layer0_dirs_swapped" (layer 0's forward and reverse tensors exchanged, its gradients reported under the exchanged names)."""
import numpy as np

import lstmtrain_ref64 as R
from lstmtrain_ref64 import LAMBDA, U, adam

FLAWS = ("mask_not_in_backward", "mask_twice", "layer0_untrained", "layer0_dirs_swapped")
_SWAP = dict(zip(R.names(0), (R.names(0)[1], R.names(0)[0], R.names(0)[3], R.names(0)[2])))


def names():
    """layer 0's four tensors, then layer 1's, each in the order of the device's flat buffers"""
    return R.names(0) + R.names(1)


def _masked(a, k_a, keep):
    """a * keep and its kappa; the float32 product rounds unless keep is 0 or a power of two"""
    p = a * keep
    rounds = (keep != 0) & (np.frexp(keep)[0] != 0.5)
    return p, k_a * np.abs(keep) + LAMBDA * U * np.abs(p) * rounds


def _swapped(d):
    return None if d is None else {**d, **{_SWAP[n]: d[n] for n in R.names(0)}}


def run(params, X0, keep, dH=None, dparams=None, flaw=None, kX0=None, kdH=None, base=None):
    """float32 inputs -> dict: Y0, X1, H, dX1, dY0, grads {name: array of both layers} in float64 and their kappas k_Y0, k_X1, k_H,
    k_dX1, k_dY0, k_grads; r0, r1: the two layers' runs.  dH None: forward only.  `base`: the right model's run on exactly these
    inputs, whose stages a control takes over where its flaw leaves them as they are (a saving of time, nothing else)."""
    assert flaw is None or flaw in FLAWS, flaw
    if base is not None and flaw in ("mask_not_in_backward", "layer0_untrained"):
        out = dict(base)                                       # the forward and layer 1's backward are the right model's
        if flaw == "layer0_untrained":
            out["grads"] = {n: np.zeros_like(g) if n in R.names(0) else g for n, g in base["grads"].items()}
            return out
        dY0, k_dY0 = base["dX1"], base["k_dX1"]
        r0 = R.run(0, params, X0, dY0, dparams=dparams, kX=kX0, kdY=k_dY0, want_dX=False)
        out.update(dY0=dY0, k_dY0=k_dY0, grads={**r0["grads"], **base["r1"]["grads"]}, k_grads={**r0["k_grads"], **base["r1"]["k_grads"]}, r0=r0)
        return out
    keep = np.asarray(keep, np.float64)
    if flaw == "mask_twice":
        keep = keep * keep
    p0, dp0 = (_swapped(params), _swapped(dparams)) if flaw == "layer0_dirs_swapped" else (params, dparams)
    f0 = R.run(0, p0, X0, dparams=dp0, kX=kX0)
    assert keep.shape == f0["Y"].shape, (keep.shape, f0["Y"].shape)
    X1, k_X1 = _masked(f0["Y"], f0["k_Y"], keep)
    r1 = R.run(1, params, X1, dH, dparams=dparams, kX=k_X1, kdY=kdH)
    out = dict(Y0=f0["Y"], k_Y0=f0["k_Y"], X1=X1, k_X1=k_X1, H=r1["Y"], k_H=r1["k_Y"], r0=f0, r1=r1)
    if dH is None:
        return out
    one = np.ones_like(keep)
    dY0, k_dY0 = _masked(r1["dX"], r1["k_dX"], one if flaw == "mask_not_in_backward" else keep)
    r0 = R.run(0, p0, X0, dY0, dparams=dp0, kX=kX0, kdY=k_dY0, want_dX=False)
    g0, k0 = r0["grads"], r0["k_grads"]
    if flaw == "layer0_dirs_swapped":
        g0, k0 = _swapped(g0), _swapped(k0)
    if flaw == "layer0_untrained":
        g0 = {n: np.zeros_like(g) for n, g in g0.items()}
    out.update(dX1=r1["dX"], k_dX1=r1["k_dX"], dY0=dY0, k_dY0=k_dY0, grads={**g0, **r1["grads"]}, k_grads={**k0, **r1["k_grads"]}, r0=r0)
    return out


def train_steps(params, X0, keep, dH, steps, flaw=None, lr=1e-4, kX0=None, kdH=None):
    """`steps` full steps on the same batch and the same mask in float64, the errors carried from step to step:
    -> (params, exp_avg, exp_avg_sq, k_params, k_exp_avg, k_exp_avg_sq, the first step's run)."""
    nm = names()
    p = {n: np.asarray(params[n], np.float64) for n in nm}
    m, v, ep, em, ev = ({n: np.zeros_like(p[n]) for n in nm} for _ in range(5))
    first = None
    for t in range(1, steps + 1):
        r = run(p, X0, keep, dH, dparams=ep, flaw=flaw, kX0=kX0, kdH=kdH)
        first = first or r
        for n in nm:
            p[n], m[n], v[n], ep[n], em[n], ev[n] = adam(p[n], r["grads"][n], m[n], v[n], t, lr=lr, ep=ep[n], eg=r["k_grads"][n], em=em[n], ev=ev[n])
    return p, m, v, ep, em, ev, first
