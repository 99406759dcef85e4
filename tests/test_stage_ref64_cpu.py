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


def test_bf16_basis_is_off_by_default_and_moves_the_rows(chain):
    """StageRef64.expand(bf16_basis=True), the lost-low-terms control of tests/test_gpu_stage_mixed_ref64.py: the default is bitwise
    what it was, the option moves every frame's rows by about a bf16 rounding of the basis (2^-9 relative per product) and leaves a
    row of zero coefficients -- the means alone -- untouched."""
    _, ref, st = chain
    coef, rows = torch.from_numpy(st["coef"]), torch.from_numpy(st["rows"])
    plain = torch.cat([(coef[:, :85] @ ref.pca_s[0].T + ref.pca_s[1]).reshape(8, -1, 6),
                       (coef[:, 85:] @ ref.pca_r[0].T + ref.pca_r[1]).reshape(8, -1, 3)], -1).reshape(8, -1)
    assert torch.equal(ref.expand(coef), rows) and torch.equal(ref.expand(coef, bf16_basis=False), rows) and torch.equal(plain, rows)
    moved = (ref.expand(coef, bf16_basis=True) - rows).abs().amax(1) / float(rows.abs().max())
    assert 1e-5 < float(moved.min()) and float(moved.max()) < 1e-2, moved
    zero = torch.zeros(1, 265, dtype=torch.float64)
    assert torch.equal(ref.expand(zero, bf16_basis=True), ref.expand(zero))


# ------------------------------------------------------------------------------------------------------------- offsets head
@pytest.fixture(scope="module")
def offsets_chain(golden, synth_sd):
    """The offsets model's stages chained on the fixture's first 4 frames (speaker 2, as tests/test_oracle_golden.py)."""
    g = golden["model_offsets"]
    x = torch.from_numpy(golden["model_dgrad"]["audio_feat"][g["audio_feat_index"]])
    ref = StageRef64(synth_sd["offsets"], head="offsets")
    z, align = ref.attention(ref.bilstm(ref.freq(ref.conv_stack(x))))
    coef = ref.regress(z, torch.full((4,), 2))
    return g, ref, dict(z=z.numpy(), align=align.numpy(), coef=coef.numpy(), rows=ref.expand(coef).numpy())


def test_offsets_head_matches_the_reference_fixture(offsets_chain):
    g, _, st = offsets_chain
    assert st["coef"].dtype == st["rows"].dtype == np.float64
    assert np.abs(st["z"] - g["z"][:, 0]).max() <= TOL_ACT
    assert np.abs(st["align"] - g["align"][:, 0]).max() <= TOL_ALIGN
    assert st["coef"].shape == (4, 59) and np.abs(st["coef"] - g["coef"][:, 0]).max() <= TOL_ACT
    assert st["rows"].shape == (4, 15069)
    assert np.abs(st["rows"][0] - g["offsets_f0"]).max() <= TOL_DGRAD
    assert np.abs(st["rows"][:, ::7] - g["offsets_stride7"]).max() <= TOL_DGRAD
    assert np.abs(st["rows"].sum(1) - g["offsets_sum"]).max() <= 15069 * 1e-6


def test_offsets_regressor_reads_its_speaker(offsets_chain):
    """The one-hot speaker code enters the first FC only; another speaker gives other coefficients."""
    _, ref, st = offsets_chain
    z = torch.from_numpy(st["z"])
    c5 = ref.regress(z, torch.full((4,), 5)).numpy()
    assert np.abs(c5 - st["coef"]).max() > 1e-4
    mixed = ref.regress(z, torch.tensor([2, 5, 2, 5])).numpy()
    assert np.abs(mixed[0::2] - st["coef"][0::2]).max() <= 1e-12 and np.abs(mixed[1::2] - c5[1::2]).max() <= 1e-12


def test_offsets_bf16_basis_is_off_by_default_and_moves_the_rows(offsets_chain):
    _, ref, st = offsets_chain
    coef, rows = torch.from_numpy(st["coef"]), torch.from_numpy(st["rows"])
    assert torch.equal(ref.expand(coef), rows)
    moved = (ref.expand(coef, bf16_basis=True) - rows).abs().amax(1) / float(rows.abs().max())
    assert 1e-5 < float(moved.min()) and float(moved.max()) < 1e-2, moved


def test_offsets_missing_mean_touches_only_its_column(offsets_chain):
    _, ref, st = offsets_chain
    means = ref.row_means()
    assert means.shape == (15069,)
    j = int(means.abs().argmax())
    diff = (ref.expand(torch.from_numpy(st["coef"]), drop_mean=j) - torch.from_numpy(st["rows"])).abs()
    assert abs(float(diff[:, j].min()) - float(means[j].abs())) <= 1e-12
    diff[:, j] = 0
    assert float(diff.max()) <= 1e-12
