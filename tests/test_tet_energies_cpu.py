"""CPU pins for the energy tests: tests/tet_energies_ref.py evaluated in fp32 reproduces what the reference's own
layers/DefTet/deftet.py returned (tests/golden/deftet_module.npz at pow 4, deftet_energies_pows.npz at pow 1..5 and on
inverted tets), and the front ends of A7 / A11 refuse malformed arguments before anything reaches a kernel."""
import os

import numpy as np
import pytest
import torch

from tests import tet_energies_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODULE = os.path.join(GOLDEN, "deftet_module.npz")
POWS = os.path.join(GOLDEN, "deftet_energies_pows.npz")


def _value_and_grad(tet, inv, pow_v, pow_e, col):
    t = torch.from_numpy(tet).clone().requires_grad_(True)
    out = R.energies(t, None if inv is None else torch.from_numpy(inv), pow_v, pow_e, 20.0)[0][:, col]
    (g,) = torch.autograd.grad(out.sum(), t)
    assert out.dtype == torch.float32
    return out.detach().numpy(), g.numpy()


def _pin(name, got, want):
    # the tolerances of test_energies_match_reference_values_and_gradients: rtol 2e-5 on values, 2e-5 of the max on gradients
    assert np.allclose(got[0], want[0], rtol=2e-5, atol=1e-12), (name, got[0], want[0])
    assert np.abs(got[1] - want[1]).max() <= 2e-5 * np.abs(want[1]).max(), name


def test_restatement_fp32_matches_reference_at_pow4():
    g = np.load(MODULE)
    tet, inv = g["tet_bxtx4x3"], g["inverse_v"]
    for col, key in enumerate(("volume_variance", "amips", "edge_length")):
        _pin(key, _value_and_grad(tet, inv, 4, 4, col), (g[key], g["g_" + key]))


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5])
def test_restatement_fp32_matches_reference_at_pow(p):
    g = np.load(POWS)
    tet = g["tet_bxtx4x3"]
    for col, key in ((0, "volume_variance_pow%d" % p), (2, "edge_length_pow%d" % p)):
        _pin(key, _value_and_grad(tet, None, p, p, col), (g[key], g["g_" + key]))


def test_restatement_fp32_matches_reference_defaults_and_inverted_amips():
    g = np.load(POWS)
    tet, inv, inverted = g["tet_bxtx4x3"], g["inverse_v"], g["inverted"]
    # the reference's default exponent of both methods is 2 (deftet.py:239,320)
    assert np.array_equal(g["volume_variance_default"], g["volume_variance_pow2"])
    assert np.array_equal(g["edge_length_default"], g["edge_length_pow2"])
    assert np.array_equal(g["g_edge_length_default"], g["g_edge_length_pow2"])
    _pin("amips", _value_and_grad(tet, inv, 2, 2, 1), (g["amips"], g["g_amips"]))
    # the fixture does hold inverted tets, they are the ones make_tets says, and the reference gave them no gradient
    assert 0 < inverted.sum() < inverted.size
    det = R.amips_per_tet(torch.from_numpy(tet).double(), torch.from_numpy(inv).double(), 20.0)[1].numpy()
    assert np.array_equal(det < 0, np.broadcast_to(inverted, det.shape))
    assert not g["g_amips"][:, inverted].any() and np.abs(g["g_amips"][:, ~inverted]).reshape(-1, 12).max(1).min() > 0
    # ... and masking them is what the value is: the mean over ALL tets of the terms of the upright ones
    e = R.amips_per_tet(torch.from_numpy(tet).double(), torch.from_numpy(inv).double(), 20.0, masked=False)[0].numpy()
    assert np.allclose((e * ~inverted).mean(-1), g["amips"], rtol=2e-5, atol=0)


def test_make_tets_is_well_conditioned():
    for T, invert in ((1, "some"), (5, "some"), (1000, "some"), (64, "all"), (64, "none")):
        tet, inv, inverted = R.make_tets(3, T, seed=T, invert=invert)
        det = R.amips_per_tet(tet.double(), inv.double(), 20.0)[1]
        assert det.abs().min() >= 0.2                                     # 0.6^3 = 0.216
        assert torch.equal(det < 0, inverted[None].expand_as(det))
        edges = (tet[:, :, :, None, :] - tet[:, :, None, :, :]).norm(dim=-1)
        assert edges.max() < 4.0 and edges[edges > 0].min() > 0.2          # edges of order 1


# ---------------------------------------------------------------- front-end argument checks (no GPU is touched: they come first)
def _tet(B=2, T=5):
    return torch.zeros(B, T, 4, 3)


@pytest.mark.parametrize("tet_shape", [(5, 4, 3), (2, 5, 3, 4), (2, 5, 12), (2, 5, 4, 3, 1), (2, 5, 4, 2)])
def test_tet_energies_rejects_tet_shape(tet_shape):
    from deftet_amd import hip_ops
    with pytest.raises(RuntimeError, match=r"tet \[B,T,4,3\]"):
        hip_ops.tet_energies(torch.zeros(tet_shape), None, 4, 4)


@pytest.mark.parametrize("inv_shape", [(4, 3, 3), (6, 3, 3), (5, 9), (5, 3, 2), (1, 5, 3, 3), (0, 3, 3)])
def test_tet_energies_rejects_inverse_v_shape(inv_shape):
    """A short inverse_v would be read out of bounds by the kernels (one 3x3 per tet)."""
    from deftet_amd import hip_ops
    with pytest.raises(RuntimeError, match=r"inverse_v \[5,3,3\]"):
        hip_ops.tet_energies(_tet(), torch.zeros(inv_shape), 4, 4)


@pytest.mark.parametrize("pows", [(0, 4), (4, 0), (17, 4), (4, 17), (-1, 2), (2.5, 2), (2, "4")])
def test_tet_energies_rejects_pow(pows):
    from deftet_amd import hip_ops
    with pytest.raises(RuntimeError, match="pow"):
        hip_ops.tet_energies(_tet(), None, *pows)


def test_checks_come_before_the_device_check():
    """Well-formed CPU tensors get as far as the 'no CPU fallback' error: the shape checks accept them."""
    from deftet_amd import hip_ops
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip_ops.tet_energies(_tet(), torch.zeros(5, 3, 3), 1, 16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip_ops.boundary_index(torch.zeros(7, 3, dtype=torch.long), torch.zeros(7, 2, dtype=torch.long), torch.zeros(2, 5), 2)


@pytest.mark.parametrize("face,tidx,occ,mode,what", [
    ((7, 4), (7, 2), (2, 5), 1, "face"),
    ((21,), (7, 2), (2, 5), 1, "face"),
    ((7, 3), (7, 3), (2, 5), 1, "tet_idx"),
    ((7, 3), (6, 2), (2, 5), 1, "tet_idx"),
    ((7, 3), (14,), (2, 5), 2, "tet_idx"),
    ((7, 3), (7, 2), (5,), 1, "occ"),
    ((7, 3), (7, 2), (2, 5, 1), 2, "occ"),
    ((7, 3), (7, 2), (2, 5), 0, "mode"),
    ((7, 3), (7, 2), (2, 5), 3, "mode"),
    ((7, 3), (7, 2), (2, 5), 1.5, "mode"),
])
def test_boundary_index_rejects(face, tidx, occ, mode, what):
    from deftet_amd import hip_ops
    with pytest.raises(RuntimeError, match=what):
        hip_ops.boundary_index(torch.zeros(face, dtype=torch.long), torch.zeros(tidx, dtype=torch.long), torch.zeros(occ), mode)
