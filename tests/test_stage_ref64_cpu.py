"""Pins the float64 stage reference (tests/stage_ref64.py) to the reference project's own outputs before it judges any kernel:
the six stages chained on the 8-frame fixture reproduce every stage the fixture holds, within the bounds that pin the numpy
oracle (tests/test_oracle_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from stage_ref64 import StageRef64

TOL_ACT = 2e-5       # as tests/test_oracle_golden.py
TOL_ALIGN = 1e-6
TOL_DGRAD = 1e-5


@pytest.fixture(scope="module")
def chain(golden, synth_sd):
    g = golden["model_dgrad"]
    ref = StageRef64(synth_sd["dgrad"])
    x = torch.from_numpy(g["audio_feat"])
    st = dict(conv3=ref.conv_stack(x))
    st["freq"] = ref.freq(st["conv3"])
    st["bilstm"] = ref.bilstm(st["freq"])
    st["z"], st["align"] = ref.attention(st["bilstm"])
    st["coef"] = ref.regress(st["z"], torch.full((8,), int(g["speaker"])))
    st["rows"] = ref.expand(st["coef"])
    return g, ref, {k: v.numpy() for k, v in st.items()}


def test_stages_match_the_reference_fixture(chain):
    g, _, st = chain
    assert all(v.dtype == np.float64 for v in st.values())
    assert np.abs(st["conv3"][:2] - g["conv3_f01"]).max() <= TOL_ACT
    assert np.abs(st["freq"] - g["freq"][:, :, 0, :]).max() <= TOL_ACT
    assert np.abs(st["bilstm"] - g["bilstm"]).max() <= TOL_ACT
    assert np.abs(st["align"] - g["align"][:, 0]).max() <= TOL_ALIGN
    assert np.abs(st["align"].sum(-1) - 1).max() <= 1e-12
    assert np.abs(st["z"] - g["z"][:, 0]).max() <= TOL_ACT
    assert np.abs(st["coef"][:, :85] - g["coef_scale"][:, 0]).max() <= TOL_ACT
    assert np.abs(st["coef"][:, 85:] - g["coef_rotat"][:, 0]).max() <= TOL_ACT
    assert st["rows"].shape == (8, 89784)
    assert np.abs(st["rows"][:2] - g["dgrad_f01"]).max() <= TOL_DGRAD
    assert np.abs(st["rows"][:, ::97] - g["dgrad_stride97"]).max() <= TOL_DGRAD


def test_second_speaker(golden, chain):
    g5 = golden["model_dgrad_spk5"]
    _, ref, st = chain
    coef = ref.regress(torch.from_numpy(st["z"][:3]), torch.full((3,), 5)).numpy()
    assert np.abs(coef[:, :85] - g5["coef_scale"][:, 0]).max() <= TOL_ACT
    assert np.abs(ref.expand(torch.from_numpy(coef)).numpy()[:, ::97] - g5["dgrad_stride97"]).max() <= TOL_DGRAD


def test_chunking_does_not_change_a_stage(chain):
    """The stages process frames in chunks to bound their float64 intermediates; a chunk boundary must not show (beyond the
    float64 rounding of another matrix-product blocking)."""
    _, ref, st = chain
    close = lambda a, b: np.abs(a.numpy() - b).max() <= 1e-12
    assert close(ref.freq(torch.from_numpy(st["conv3"][:5]), chunk=2), st["freq"][:5])
    assert close(ref.bilstm(torch.from_numpy(st["freq"]), chunk=3), st["bilstm"])
    z, al = ref.attention(torch.from_numpy(st["bilstm"]), chunk=3)
    assert close(z, st["z"]) and close(al, st["align"])


def test_perturbations_touch_only_what_they_name(chain):
    """The sensitivity controls of the GPU tests: each perturbation changes its stage, and only where it says."""
    _, ref, st = chain
    h = torch.from_numpy(np.concatenate([st["bilstm"]] * 4))              # 32 frames: two 16-frame units
    z0, a0 = ref.attention(h)
    z1, a1 = ref.attention(h, stale=(16, 40))
    d = (z1 - z0).abs().amax(1)
    assert float(d[:16].max()) == 0.0 and float(d[16:].min()) > 1e-5
    b0 = ref.bilstm(torch.from_numpy(st["freq"][:2]))
    b1 = ref.bilstm(torch.from_numpy(st["freq"][:2]), drop_h=(0, 1, 20))
    assert float((b1 - b0).abs().max()) > 1e-3
    j = int(ref.row_means().abs().argmax())
    r1 = ref.expand(torch.from_numpy(st["coef"][:2]), drop_mean=j)
    diff = (r1 - torch.from_numpy(st["rows"][:2])).abs()
    assert abs(float(diff[:, j].min()) - float(ref.row_means()[j].abs())) <= 1e-12
    diff[:, j] = 0
    assert float(diff.max()) <= 1e-12
