"""GPU tests of the fused per-tet energies (A11, deftet_amd/csrc/tet_ops.hip) beyond the reference's default exponent 4:
every instance of the kernels, both reduction forms, the shapes around a wave / a workgroup / the grid, inverted tets, the
kink of pow_v == 1 and the ticket counters across calls — against tests/tet_energies_ref.py in float64, which
tests/test_tet_energies_cpu.py pins to the reference's own outputs.

Values are compared relative to the size of the terms they were summed from (the restatement's conditioning scales; for
AMIPS, whose terms are all positive, the value itself) with the standing 1e-5 of tests/tol.py; gradients in max-norm with the
1.5e-5 that test_energies_res70_vs_torch_fp64 asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import tet_energies_ref as R
from tests.tol import check_close

pytestmark = pytest.mark.gpu
POWS_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deftet_energies_pows.npz")

VALUE_BOUND, GRAD_BOUND = 1e-5, 1.5e-5
SCALE = 20.0
PAIRS = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 2), (2, 5), (6, 6), (4, 2), (2, 4)]
# below / at / past one wave, around the 1024 threads of a workgroup, one and 4,465 tets past the 65,536 threads of a shape's grid
SIZES = [1, 5, 63, 64, 65, 1023, 1025, 65537, 70001]
GSEL = [[1.0, 0.5, 2.0], [0.3, 1.5, 1.0], [0.7, 1.0, 0.4]]


@functools.lru_cache(maxsize=None)
def _inputs(B, T, invert="some"):
    tet, inv, inverted = R.make_tets(B, T, seed=1000 + T + 7 * B, invert=invert)
    dev = torch.device("cuda:0")
    return tet.to(dev), inv.to(dev), inverted.to(dev)


def _reference(tet, inv, pow_v, pow_e):
    """fp64 restatement on the GPU: (out [B,3], vol_scale, edge_scale, [d out[:,k].sum() / d tet for k in 0..2])."""
    t64 = tet.detach().double().requires_grad_(True)
    out, vs, es = R.energies(t64, None if inv is None else inv.double(), pow_v, pow_e, SCALE)
    grads = [torch.autograd.grad(out[:, k].sum(), t64, retain_graph=True)[0] if (k != 1 or inv is not None) else torch.zeros_like(t64)
             for k in range(3)]
    return out.detach(), vs, es, grads


def _run(hip_ops, tet, inv, pow_v, pow_e, gouts):
    tg = tet.detach().clone().requires_grad_(True)
    out = hip_ops.tet_energies(tg, inv, pow_v, pow_e, SCALE)
    return out.detach(), [torch.autograd.grad(out, tg, g, retain_graph=True)[0] for g in gouts]


def _check_sum(name, got, want, scale):
    """|got - want| / scale per shape, handed to check_close as 1 + error against 1 so that the reported max-norm reading IS
    the error relative to the conditioning scale; a sum of nothing but zeros (scale 0) has to be exact."""
    got, want, scale = got.double(), want.double(), scale.double()
    err = torch.where(scale > 0, (got - want) / torch.where(scale > 0, scale, torch.ones_like(scale)), got - want)
    return check_close(name, 1.0 + err, torch.ones_like(err), VALUE_BOUND)


def _check_values(name, out, want, vs, es, has_inv):
    _check_sum(name + " volume", out[:, 0], want[:, 0], vs)
    _check_sum(name + " edge", out[:, 2], want[:, 2], es)
    if has_inv:
        check_close(name + " amips", out[:, 1], want[:, 1], VALUE_BOUND, elem_rel=VALUE_BOUND, floor=0.0)
    else:
        assert not out[:, 1].any(), name


def _check_against_restatement(hip_ops, name, tet, inv, pow_v, pow_e, columns=True):
    B = tet.shape[0]
    want, vs, es, g64 = _reference(tet, inv, pow_v, pow_e)
    gsel = torch.tensor(GSEL, device=tet.device)[torch.arange(B, device=tet.device) % 3]
    gouts = [gsel]
    if columns:
        gouts += [gsel * torch.eye(3, device=tet.device)[k] for k in range(3)]              # exactly one non-zero column
    out, grads = _run(hip_ops, tet, inv, pow_v, pow_e, gouts)
    _check_values(name, out, want, vs, es, inv is not None)
    for g, gout, tag in zip(grads, gouts, ("gout mixed", "gout volume only", "gout amips only", "gout edge only")):
        w = sum(gout[:, k].double()[:, None, None, None] * g64[k] for k in range(3))
        if tag == "gout amips only" and inv is None:
            assert not g.any(), name                                                        # no AMIPS term: no gradient at all
        else:
            check_close("%s grad, %s" % (name, tag), g, w, GRAD_BOUND)
    return out, grads, gouts


# --------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("pow_v,pow_e", PAIRS)
def test_energies_vs_fp64_restatement(cuda, pow_v, pow_e, T):
    from deftet_amd import hip_ops
    tet3, inv, inverted = _inputs(3, T)
    for B, tet in ((1, tet3[1:2].contiguous()), (3, tet3)):
        for use_inv in (True, False):
            name = "A11 pow (%d,%d) T%d B%d %s" % (pow_v, pow_e, T, B, "inv" if use_inv else "no inv")
            _, grads, _ = _check_against_restatement(hip_ops, name, tet, inv if use_inv else None, pow_v, pow_e)
            if use_inv:
                rows = grads[2].reshape(B, T, 12)                                           # gout: AMIPS column only
                assert not rows[:, inverted].any(), name                                    # det < 0: masked to exactly 0
                assert (rows[:, ~inverted].abs().amax(-1) > 0).all(), name


# --------------------------------------------------------------------------------------------- pow_v == 1 at its kink
def _corner_tets(lengths):
    """[T,4,3]: the corner tet with its x edge stretched to lengths[t] — |V| = lengths[t] / 6, exact in fp32 for multiples of 0.75"""
    t = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]).repeat(len(lengths), 1, 1)
    t[:, 1, 0] = torch.tensor(lengths)
    return t


@pytest.mark.parametrize("T", [3, 130, 1500])
def test_pow1_volume_equal_to_the_mean(cuda, T):
    """d == 0 takes torch.abs's subgradient 0: congruent tets (every d is 0) give value 0 and no volume gradient; a shape
    with volumes (1, 2, 3) / 8 repeated has its middle tets exactly at the mean, the others on either side."""
    from deftet_amd import hip_ops
    same = _corner_tets([1.5] * T)
    mixed = _corner_tets(([0.75, 1.5, 2.25] * T)[:T - T % 3] + [1.5] * (T % 3))
    tet = torch.stack([same, mixed]).to(cuda)
    d64 = R.volumes(tet.double())
    d64 = d64 - d64.mean(-1, keepdim=True)
    assert not d64[0].any() and (d64[1] == 0).sum() == T // 3 + T % 3 and (d64[1] > 0).sum() == (d64[1] < 0).sum() == T // 3
    gout = torch.tensor([[1.0, 0, 0], [1.0, 0, 0]], device=cuda)
    for pow_e in (1, 2):
        out, (g,) = _run(hip_ops, tet, None, 1, pow_e, [gout])
        want, vs, es, g64 = _reference(tet, None, 1, pow_e)
        assert out[0, 0] == 0 and not g[0].any()
        assert not g[1][d64[1] == 0].any()
        _check_values("A11 pow_v 1 at the kink T%d pow_e %d" % (T, pow_e), out, want, vs, es, False)
        check_close("A11 pow_v 1 at the kink T%d pow_e %d grad" % (T, pow_e), g, g64[0], GRAD_BOUND)
        assert (g[1][d64[1] != 0].reshape(-1, 12).abs().amax(-1) > 0).all()


# --------------------------------------------------------------------------------------------- inverted tets
def test_amips_masks_inverted_tets(cuda):
    from deftet_amd import hip_ops
    tet, inv, inverted = _inputs(3, 1000)
    assert 0 < inverted.sum() < 1000
    e = R.amips_per_tet(tet.double(), inv.double(), SCALE, masked=False)[0]
    want = (e * ~inverted).mean(-1)                                                         # the mean over ALL tets of the upright terms
    out = hip_ops.tet_energies(tet, inv, 2, 2, SCALE)
    check_close("A11 amips, inverted tets masked by construction", out[:, 1], want, VALUE_BOUND, elem_rel=VALUE_BOUND, floor=0.0)


@pytest.mark.parametrize("T", [5, 1025])
def test_amips_of_only_inverted_tets_is_zero(cuda, T):
    from deftet_amd import hip_ops
    tet, inv, inverted = _inputs(2, T, "all")
    assert inverted.all()
    gout = torch.tensor([[0.0, 1.0, 0.0], [0.0, 2.0, 0.0]], device=cuda)
    for pows in ((2, 2), (4, 4)):
        out, (g,) = _run(hip_ops, tet, inv, *pows, [gout])
        assert not out[:, 1].any() and not g.any()
    upright = _inputs(2, T, "none")
    assert (hip_ops.tet_energies(upright[0], upright[1], 2, 2, SCALE)[:, 1] > 0).all()


# --------------------------------------------------------------------------------------------- the per-method front ends
def test_front_end_defaults_match_reference(cuda):
    """DefTet's volume_variance / edge_length default to pow = 2 like the reference's (deftet.py:239,320)."""
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    g = np.load(POWS_GOLD)
    D = DefTet()
    tet = torch.from_numpy(g["tet_bxtx4x3"]).to(cuda).requires_grad_(True)

    def pin(y, key):
        assert np.allclose(y.detach().cpu().numpy(), g[key], rtol=2e-5, atol=0), key
        (gr,) = torch.autograd.grad(y.sum(), tet)
        assert np.abs(gr.cpu().numpy() - g["g_" + key]).max() <= 2e-5 * np.abs(g["g_" + key]).max(), key

    vv = D.volume_variance(tet)
    assert torch.equal(vv, hip_ops.tet_energies(tet, None, 2, 4)[:, 0])
    pin(vv, "volume_variance_pow2")
    el = D.edge_length(tet)
    assert torch.equal(el, hip_ops.tet_energies(tet, None, 4, 2)[:, 2])
    pin(el, "edge_length_pow2")
    pin(D.amips_energy(tet, torch.from_numpy(g["inverse_v"]).to(cuda)), "amips")
    empty = torch.zeros(tet.shape[0], 0, 3, dtype=torch.long, device=cuda)
    ret = D.forward(boundary_bxfx3=empty, tet_bxfx4x3=tet, inverse_offset=None)              # volume term at self.pow = 4, no AMIPS
    assert ret[4].shape == ret[3].shape and not ret[4].any()
    pin(ret[3], "volume_variance_pow4")
    D.pow = 2
    ret = D.forward(boundary_bxfx3=empty, tet_bxfx4x3=tet, inverse_offset=None)
    assert not ret[4].any()
    pin(ret[3], "volume_variance_pow2")


# --------------------------------------------------------------------------------------------- the two reduction forms
def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("pow_v,pow_e", [(4, 4), (2, 2), (1, 3)])
def test_counter_free_form_equals_ticket_form(cuda, pow_v, pow_e):
    """B > 1024 shapes reduce without the ticket counters (k_energy_mean / k_energy_final); the first three rows are, bit for
    bit, what the same three shapes give as a batch of their own, which finishes inside the two pass kernels."""
    from deftet_amd import hip_ops
    tet, inv, _ = _inputs(1025, 5)
    gout = torch.rand(1025, 3, generator=torch.Generator().manual_seed(3)).to(cuda) + 0.25
    big_out, (big_g,) = _run(hip_ops, tet, inv, pow_v, pow_e, [gout])
    small_out, (small_g,) = _run(hip_ops, tet[:3].contiguous(), inv, pow_v, pow_e, [gout[:3].contiguous()])
    assert _bits_equal(big_out[:3], small_out) and _bits_equal(big_g[:3], small_g)
    want, vs, es, g64 = _reference(tet, inv, pow_v, pow_e)                                    # ... and all 1025 rows are right
    _check_values("A11 pow (%d,%d) T5 B1025 counter-free" % (pow_v, pow_e), big_out, want, vs, es, True)
    w = sum(gout[:, k].double()[:, None, None, None] * g64[k] for k in range(3))
    check_close("A11 pow (%d,%d) T5 B1025 counter-free grad" % (pow_v, pow_e), big_g, w, GRAD_BOUND)


@pytest.mark.parametrize("pow_v,pow_e", [(4, 4), (2, 2)])
def test_captured_launch_equals_eager(cuda, pow_v, pow_e):
    """A captured launch takes the counter-free form too: replayed twice, the bits of the eager (ticket) call."""
    from deftet_amd import hip_ops
    tet, inv, _ = _inputs(3, 5)
    gout = torch.tensor(GSEL, device=cuda)
    eager_out, (eager_g,) = _run(hip_ops, tet, inv, pow_v, pow_e, [gout])
    x = tet.detach().clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            out = hip_ops.tet_energies(x, inv, pow_v, pow_e, SCALE)
            torch.autograd.grad(out, x, gout)
        del out
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = hip_ops.tet_energies(x, inv, pow_v, pow_e, SCALE)
        (g_s,) = torch.autograd.grad(out_s, x, gout)
    for _ in range(2):
        with torch.no_grad():
            out_s.zero_()
            g_s.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(out_s.detach(), eager_out) and _bits_equal(g_s, eager_g)


# --------------------------------------------------------------------------------------------- the counters across calls
def test_ticket_counters_across_calls(cuda):
    """Every launch leaves its stream's counters at zero: calls of different B and T back to back on one stream are each
    right, the last repeats the first bit for bit, and so does the same call on a side stream."""
    from deftet_amd import hip_ops
    results = []
    for i, (B, T) in enumerate(((3, 5), (1, 70001), (7, 64), (3, 5))):
        tet, inv, _ = _inputs(B, T)
        results.append(_check_against_restatement(hip_ops, "A11 call %d of a sequence, pow (2,3) T%d B%d" % (i, T, B), tet, inv, 2, 3,
                                                  columns=False))
    assert _bits_equal(results[0][0], results[3][0]) and _bits_equal(results[0][1][0], results[3][1][0])
    tet, inv, _ = _inputs(3, 5)
    gouts = results[0][2]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_side, (g_side,) = _run(hip_ops, tet, inv, 2, 3, gouts)
    torch.cuda.current_stream().wait_stream(side)
    assert _bits_equal(out_side, results[0][0]) and _bits_equal(g_side, results[0][1][0])
    tet, inv, _ = _inputs(3, 70001)
    first = _run(hip_ops, tet, inv, 3, 2, gouts)
    second = _run(hip_ops, tet, inv, 3, 2, gouts)
    assert _bits_equal(first[0], second[0]) and _bits_equal(first[1][0], second[1][0])


def test_non_contiguous_tet_and_float64_inverse_v(cuda):
    from deftet_amd import hip_ops
    tet, inv, _ = _inputs(3, 65)
    view = tet.transpose(0, 1).contiguous().transpose(0, 1)                                   # [3,65,4,3], strides of [65,3,4,3]
    assert not view.is_contiguous() and torch.equal(view, tet)
    gout = torch.tensor(GSEL, device=cuda)
    want_out, (want_g,) = _run(hip_ops, tet, inv, 3, 2, [gout])
    x = view.detach().requires_grad_(True)
    out = hip_ops.tet_energies(x, inv.double(), 3, 2, SCALE)
    (g,) = torch.autograd.grad(out, x, gout)
    assert _bits_equal(out.detach(), want_out) and _bits_equal(g, want_g)


# --------------------------------------------------------------------------------------------- argument checks on the device
def test_argument_errors_on_gpu_tensors(cuda):
    from deftet_amd import _lib, hip_ops
    tet, inv, _ = _inputs(3, 5)
    with pytest.raises(RuntimeError, match=r"inverse_v \[5,3,3\]"):
        hip_ops.tet_energies(tet, inv[:4], 2, 2)                                              # short: would be read past its end
    with pytest.raises(RuntimeError, match=r"tet \[B,T,4,3\]"):
        hip_ops.tet_energies(tet.reshape(3, 5, 12), inv, 2, 2)
    with pytest.raises(RuntimeError, match="pow_e"):
        hip_ops.tet_energies(tet, inv, 2, 17)
    with pytest.raises(RuntimeError, match="bad argument"):                                    # T == 0: the library's own check
        hip_ops.tet_energies(tet[:, :0], None, 2, 2)
    # the backward entry point repeats the forward's limit on the exponents (nothing is launched)
    lib = _lib.load()
    stats = torch.zeros(3, 8, dtype=torch.float64, device=cuda)
    gout, grad = torch.ones(3, 3, device=cuda), torch.empty_like(tet)
    for pows in ((17, 2), (2, 17), (0, 2)):
        rc = lib.deftet_tet_energies_bwd_f32(_lib.ptr(tet), None, _lib.ptr(stats), _lib.ptr(gout), _lib.ptr(grad), 3, 5, pows[0], pows[1],
                                             SCALE, _lib.current_stream(cuda))
        assert rc != 0 and b"bad argument" in lib.deftet_last_error()
