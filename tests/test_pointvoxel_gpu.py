"""GPU tests of the point-voxel operators (pointvoxel.hip) against the restatements of tests/pointvoxel_ref.py:
the voxelization bit for bit, the sampler's values and both gradients within the standing 1e-5 max-norm bound of the fp64
restatement, the legacy pair, determinism, the overlay route and the argument errors."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from tests import pointvoxel_ref as ref
from tests.tol import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5


def bits(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rng(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------- voxelization
def _vox_check(feat, coords, R):
    from deftet_amd import hip_ops
    f, c = torch.from_numpy(feat).to(DEV), torch.from_numpy(coords).to(DEV)
    out, ind, cnt = hip_ops.avg_voxelize_fwd(f, c, R)
    want_out, want_ind, want_cnt = ref.avg_voxelize(feat, coords, R)
    assert np.array_equal(ind.cpu().numpy(), want_ind) and np.array_equal(cnt.cpu().numpy(), want_cnt)
    assert np.array_equal(bits(out), bits(want_out))
    gy = torch.randn(out.shape, generator=rng(5)).numpy()
    gx = hip_ops.avg_voxelize_bwd(torch.from_numpy(gy).to(DEV), ind, cnt)
    assert np.array_equal(bits(gx), bits(ref.avg_voxelize_bwd(gy, want_ind, want_cnt)))


@pytest.mark.parametrize("R", [2, 8, 32])
def test_voxelization_is_bit_identical_to_the_restatement(R):
    g = np.random.default_rng(R)
    for B, C, N in itertools.product([1, 3], [1, 3, 65], [1, 63, 64, 65, 257]):
        _vox_check(g.standard_normal((B, C, N)).astype(np.float32), g.integers(0, R, (B, 3, N)).astype(np.int32), R)


def test_voxelization_edge_cases():
    from deftet_amd import hip_ops, pointvoxel
    g = np.random.default_rng(0)
    feat = g.standard_normal((2, 3, 300)).astype(np.float32)
    _vox_check(feat, np.tile(np.array([3, 5, 2], np.int32)[None, :, None], (2, 1, 300)), 8)            # one voxel holds all points
    coords = g.integers(-2, 10, (2, 3, 300)).astype(np.int32)                                           # outside [0,8) and negative
    _vox_check(feat, coords, 8)
    ind = hip_ops.avg_voxelize_fwd(torch.from_numpy(feat).to(DEV), torch.from_numpy(coords).to(DEV), 8)[1].cpu().numpy()
    bad = ((coords < 0) | (coords >= 8)).any(axis=1)
    assert bad.any() and np.all(ind[bad] == -1) and np.all(ind[~bad] >= 0)
    out, ind0, cnt0 = hip_ops.avg_voxelize_fwd(torch.zeros(2, 3, 0, device=DEV), torch.zeros(2, 3, 0, device=DEV, dtype=torch.int32), 4)   # N = 0
    assert out.shape == (2, 3, 64) and not out.any() and not cnt0.any() and ind0.shape == (2, 0)
    # a non-contiguous input and autograd through the public Function
    f = torch.from_numpy(feat).to(DEV).transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    assert not f.is_contiguous()
    c = torch.from_numpy(np.clip(coords, 0, 7)).to(DEV)
    vox = pointvoxel.avg_voxelize(f, c, 8)
    want_out, want_ind, want_cnt = ref.avg_voxelize(feat, np.clip(coords, 0, 7), 8)
    assert vox.shape == (2, 3, 8, 8, 8) and np.array_equal(bits(vox), bits(want_out.reshape(2, 3, 8, 8, 8)))
    gy = torch.randn(2, 3, 8, 8, 8, generator=rng(1))
    vox.backward(gy.to(DEV))
    assert np.array_equal(bits(f.grad), bits(ref.avg_voxelize_bwd(gy.numpy().reshape(2, 3, -1), want_ind, want_cnt)))


# ---------------------------------------------------------------------------- sampler
def uniform_pos(B, N, seed):
    return 1.05 * (torch.rand(B, N, 3, generator=rng(seed)) - 0.5)


def interior_pos(B, N, R, seed, cells=None):
    """every frac(u) in [0.01, 0.99] by construction: u = cell + frac, cell in [0, R-2]"""
    g = rng(seed)
    cell = torch.randint(0, max(R - 1, 1), (B, N, 3), generator=g) if cells is None else cells
    frac = 0.01 + 0.98 * torch.rand(B, N, 3, generator=g)
    return ((cell.double() + frac.double()) / R - 0.5).float()


def _sample_check(name, vols, pos, append_pos=False, check_pos=False):
    from deftet_amd import hip_ops
    v_gpu = [v.to(DEV).requires_grad_(True) for v in vols]
    p_gpu = pos.to(DEV).requires_grad_(check_pos)
    out = hip_ops.voxel_sample(v_gpu, p_gpu, append_pos=append_pos)
    v_ref = [v.double().requires_grad_(True) for v in vols]
    p_ref = pos.double().requires_grad_(True)
    want = ref.voxel_sample(v_ref, p_ref, append_pos=append_pos)
    assert out.shape == want.shape and out.is_contiguous()
    check_close(name + ".values", out, want, BOUND)
    gout = torch.randn(want.shape, generator=rng(11))
    out.backward(gout.to(DEV))
    want.backward(gout.double())
    for k, (a, b) in enumerate(zip(v_gpu, v_ref)):
        check_close("%s.grad_vol%d" % (name, k), a.grad, b.grad, BOUND)
    if check_pos:
        check_close(name + ".grad_pos", p_gpu.grad, p_ref.grad, BOUND)


@pytest.mark.parametrize("C", [1, 7, 64, 130])
@pytest.mark.parametrize("R", [2, 5, 8, 32])
def test_sampler_matches_the_fp64_restatement(R, C):
    for B in (1, 3):
        vol = torch.randn(B, C, R, R, R, generator=rng(C + B))
        for N in (1, 63, 64, 65, 1000):
            tag = "pv.R%d.B%d.C%d.N%d" % (R, B, C, N)
            _sample_check(tag + ".uniform", [vol], uniform_pos(B, N, N))
            _sample_check(tag + ".interior", [vol], interior_pos(B, N, R, N + 1), check_pos=True)


def test_sampler_point_sets_dense_sparse_and_border():
    R, B, N = 8, 2, 1000
    vol = torch.randn(B, 7, R, R, R, generator=rng(3))
    one_cell = torch.tensor([2, 6, 3]).expand(B, N, 3)                # a segment longer than a workgroup
    _sample_check("pv.onecell", [vol], interior_pos(B, N, R, 4, cells=one_cell), check_pos=True)
    for n in (32, 33, 64, 65, 129):                                   # either side of the length at which a wave takes the segment over
        _sample_check("pv.onecell.N%d" % n, [vol], interior_pos(B, n, R, n, cells=one_cell[:, :n]), check_pos=True)
    vol32 = torch.randn(B, 3, 32, 32, 32, generator=rng(5))           # about one point per 20 cells of 31^3 + border cells
    _sample_check("pv.sparse", [vol32], interior_pos(B, N, 32, 6), check_pos=True)
    _sample_check("pv.sparse1500", [vol32], interior_pos(B, 1500, 32, 7), check_pos=True)
    g = rng(8)
    lattice = (torch.randint(0, R, (B, 200, 3), generator=g).float() / R - 0.5)
    edge = torch.tensor([-0.5, 0.5, -0.6, 0.7, 0.5 - 1.0 / R])[torch.randint(0, 5, (B, 200, 3), generator=g)]
    _sample_check("pv.border", [vol], torch.cat([lattice, edge, uniform_pos(B, 100, 9)], 1))


@pytest.mark.parametrize("append_pos", [False, True])
def test_sampler_writes_a_list_of_volumes_into_one_result(append_pos):
    B, N = 2, 257
    vols = [torch.randn(B, 3, 8, 8, 8, generator=rng(1)), torch.randn(B, 5, 4, 4, 4, generator=rng(2)), torch.randn(B, 2, 8, 8, 8, generator=rng(3))]
    g = rng(4)
    cell4 = torch.randint(0, 3, (B, N, 3), generator=g)
    f = 0.01 + 0.475 * torch.rand(B, N, 3, generator=g) + 0.495 * torch.randint(0, 2, (B, N, 3), generator=g)   # frac at R = 4 and R = 8 in [0.01, 0.99]
    pos = ((cell4.double() + f.double()) / 4 - 0.5).float()
    _sample_check("pv.list.append%d" % append_pos, vols, pos, append_pos=append_pos, check_pos=True)
    from deftet_amd import pointvoxel
    out = pointvoxel.sample_f(pos.to(DEV), [v.to(DEV) for v in vols], append_pos=append_pos)
    want = ref.sample_f_composition(pos.to(DEV), [v.to(DEV) for v in vols])      # torch's own path on the GPU, fp32
    check_close("pv.list.vs_torch", out[:, :10], want, BOUND)
    if append_pos:
        assert torch.equal(out[:, 10:], pos.to(DEV).permute(0, 2, 1))


def test_position_gradient_border_and_integer_rules():
    from deftet_amd import hip_ops
    R = 4
    x2 = torch.arange(R, dtype=torch.float32).pow(2).view(1, 1, R, 1, 1).expand(1, 1, R, R, R).contiguous()
    vol = (x2 + x2.permute(0, 1, 3, 2, 4) * 2 + x2.permute(0, 1, 3, 4, 2) * 3).to(DEV)           # x^2 + 2 y^2 + 3 z^2
    pts = torch.tensor([[[-0.5, 0.5, 0.6],                         # u = 0, u past r - 1 twice: held by the clamp
                         [0.25, -0.7, 0.1],                         # u_x = 3 = r - 1 exactly; y below 0
                         [-0.25, 0.0, 0.1]]], device=DEV, requires_grad=True)                     # u_x = 1, u_y = 2: interior integers
    hip_ops.voxel_sample([vol], pts).sum().backward()
    g = pts.grad[0].cpu()
    assert torch.all(g[0] == 0) and g[1, 0] == 0 and g[1, 1] == 0 and g[1, 2] != 0
    assert float(g[2, 0]) == pytest.approx(R * (4 - 1), rel=1e-5)          # the right-hand cell [1,2] of x^2
    assert float(g[2, 1]) == pytest.approx(R * 2 * (9 - 4), rel=1e-5)      # [2,3] of 2 y^2
    u_z = (0.1 + 0.5) * R                                                   # inside [2,3]
    assert float(g[2, 2]) == pytest.approx(R * 3 * (9 - 4), rel=1e-5) and 2 < u_z < 3


def test_trilinear_devoxelize_agrees_with_torch_grid_sample_on_the_gpu():
    from deftet_amd import pointvoxel
    for R, C, N in [(8, 7, 1000), (32, 3, 257), (5, 2, 65)]:
        B = 2
        g = rng(R)
        c = torch.randn(B, C, R, R, R, generator=g)
        cell = torch.randint(0, R - 1, (B, 3, N), generator=g)
        coords = (cell + 0.01 + 0.98 * torch.rand(B, 3, N, generator=g)).float()
        res = []
        for fn in (pointvoxel.trilinear_devoxelize, ref.grid_sample_composition):
            cg, xg = c.to(DEV).requires_grad_(True), coords.to(DEV).requires_grad_(True)
            out = fn(cg, xg, R)
            out.backward(torch.randn(out.shape, generator=rng(2)).to(DEV))
            res.append((out.detach(), cg.grad, xg.grad))
        for a, b, what in zip(res[0], res[1], ("values", "grad_c", "grad_coords")):
            check_close("pv.vs_grid_sample.R%d.%s" % (R, what), a, b, BOUND)


def test_both_backwards_are_bit_reproducible():
    from deftet_amd import hip_ops
    B, N = 2, 3000
    vols = [torch.randn(B, 9, 8, 8, 8, generator=rng(1)).to(DEV), torch.randn(B, 4, 32, 32, 32, generator=rng(2)).to(DEV)]
    pos = (0.3 * torch.randn(B, N, 3, generator=rng(3))).to(DEV)              # clustered: long segments at 8^3
    gout = torch.randn(B, 16, N, generator=rng(4)).to(DEV)
    runs = []
    for _ in range(2):
        v = [x.clone().requires_grad_(True) for x in vols]
        p = pos.clone().requires_grad_(True)
        hip_ops.voxel_sample(v, p, append_pos=True).backward(gout)
        runs.append([x.grad for x in v] + [p.grad])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    feat = torch.randn(B, 5, N, generator=rng(5)).to(DEV)
    coords = torch.randint(0, 4, (B, 3, N), generator=rng(6), dtype=torch.int32).to(DEV)
    gy = torch.randn(B, 5, 64, generator=rng(7)).to(DEV)
    vox = []
    for _ in range(2):
        out, ind, cnt = hip_ops.avg_voxelize_fwd(feat, coords, 4)
        vox.append((out, ind, cnt, hip_ops.avg_voxelize_bwd(gy, ind, cnt)))
    for a, b in zip(*vox):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- the legacy pair
@pytest.mark.parametrize("R,C,N", [(2, 3, 257), (8, 3, 257), (8, 65, 64), (32, 1, 1000)])
def test_legacy_pair_matches_the_restatement(R, C, N):
    from deftet_amd import pointvoxel
    B = 2
    g = np.random.default_rng(R + N)
    coords = g.uniform(0, R - 1, (B, 3, N)).astype(np.float32)
    coords[:, :, :16] = np.round(coords[:, :, :16])                   # d == 0: hi falls back on lo
    coords[:, 0, 16:24] = R - 1
    if N == 1000:
        coords[:, :, 300:] = (np.array([1, 0, 1], np.float32)[None, :, None] + g.uniform(0.01, 0.99, (B, 3, 700))).astype(np.float32)
    feat = g.standard_normal((B, C, R ** 3)).astype(np.float32)
    outs, inds, wgts = pointvoxel.backend.trilinear_devoxelize_forward(R, True, torch.from_numpy(coords).to(DEV), torch.from_numpy(feat).to(DEV))
    w_outs, w_inds, w_wgts = ref.legacy_devoxelize(coords, feat, R)
    assert np.array_equal(inds.cpu().numpy(), w_inds)
    assert np.array_equal(bits(wgts), bits(w_wgts)) and np.array_equal(bits(outs), bits(w_outs))
    gy = g.standard_normal((B, C, N)).astype(np.float32)
    gx = pointvoxel.backend.trilinear_devoxelize_backward(torch.from_numpy(gy).to(DEV), inds, wgts, R)
    assert gx.shape == (B, C, R ** 3)
    check_close("pv.legacy.R%d.grad_x" % R, gx, ref.legacy_devoxelize_bwd(gy, w_inds, w_wgts, R), BOUND)
    o2, i2, w2 = pointvoxel.backend.trilinear_devoxelize_forward(R, False, torch.from_numpy(coords).to(DEV), torch.from_numpy(feat).to(DEV))
    assert torch.equal(o2, outs) and tuple(i2.shape) == (1,) and tuple(w2.shape) == (1,) and not i2.any() and not w2.any()
    # the autograd wrapper of the pair
    f = torch.from_numpy(feat).to(DEV).view(B, C, R, R, R).requires_grad_(True)
    pointvoxel.trilinear_devoxelize_ori(f, torch.from_numpy(coords).to(DEV), R, True).backward(torch.from_numpy(gy).to(DEV))
    assert torch.equal(f.grad.view(B, C, -1), gx)


# ---------------------------------------------------------------------------- through the overlay
def test_reference_shaped_callers_run_through_the_overlay():
    """Voxelization.forward (layers/pv_module/voxelization.py:18-33, normalize=False) and PVConv's devoxelize call
    (pvconv.py:35-37), restated, on the modules `install(point_voxel=True)` registers."""
    from deftet_amd import overlay
    done = overlay.install(kaolin=False, point_voxel=True)
    try:
        _backend = sys.modules["layers.pv_module.functional.backend"]._backend
        dv = sys.modules["layers.pv_module.functional.devoxelization"]

        class AvgVoxelization(torch.autograd.Function):             # functional/voxelization.py:8-37
            @staticmethod
            def forward(ctx, features, coords, resolution):
                features, coords = features.contiguous().float(), coords.int().contiguous()
                b, c, _ = features.shape
                out, indices, counts = _backend.avg_voxelize_forward(features, coords, resolution)
                ctx.save_for_backward(indices, counts)
                return out.view(b, c, resolution, resolution, resolution)

            @staticmethod
            def backward(ctx, grad_output):
                b, c = grad_output.shape[:2]
                indices, counts = ctx.saved_tensors
                return _backend.avg_voxelize_backward(grad_output.contiguous().view(b, c, -1), indices, counts), None, None

        B, C, N, r = 2, 6, 500, 8
        features = torch.randn(B, C, N, generator=rng(1)).to(DEV).requires_grad_(True)
        coords = (0.4 * torch.randn(B, 3, N, generator=rng(2))).to(DEV)
        norm_coords = coords.detach() - coords.detach().mean(2, keepdim=True)
        norm_coords = torch.clamp((norm_coords + 1) / 2.0 * r, 0, r - 1)
        vox_coords = torch.round(norm_coords).to(torch.int32)
        voxel_features = AvgVoxelization.apply(features, vox_coords, r)
        devoxel = dv.trilinear_devoxelize(voxel_features, norm_coords, r, True)
        gout = torch.randn(B, C, N, generator=rng(3)).to(DEV)
        devoxel.backward(gout)
        # the same composition in fp64 on the restatements
        w_out, w_ind, w_cnt = ref.avg_voxelize(features.detach().cpu().numpy(), vox_coords.cpu().numpy(), r)
        assert np.array_equal(bits(voxel_features), bits(w_out.reshape(B, C, r, r, r)))
        vf = torch.from_numpy(w_out).double().view(B, C, r, r, r).requires_grad_(True)
        want = ref.voxel_sample([vf], norm_coords.cpu().double(), voxel_units=True)
        check_close("pv.overlay.values", devoxel, want, BOUND)
        want.backward(gout.cpu().double())
        g_feat = ref.avg_voxelize_bwd(vf.grad.float().numpy().reshape(B, C, -1), w_ind, w_cnt)
        check_close("pv.overlay.grad_features", features.grad, g_feat, BOUND)
    finally:
        overlay.uninstall(done)


# ---------------------------------------------------------------------------- argument errors
def test_argument_errors_raise():
    from deftet_amd import hip_ops, pointvoxel
    vol, pos = torch.zeros(2, 3, 4, 4, 4, device=DEV), torch.zeros(2, 5, 3, device=DEV)
    feat, coords = torch.zeros(2, 3, 5, device=DEV), torch.zeros(2, 3, 5, device=DEV, dtype=torch.int32)
    bad = [lambda: hip_ops.voxel_sample([vol.cpu()], pos), lambda: hip_ops.voxel_sample([vol], pos.cpu()),
           lambda: hip_ops.voxel_sample([vol.double()], pos), lambda: hip_ops.voxel_sample([vol], pos.half()),
           lambda: hip_ops.voxel_sample([vol[:, :, :, :, :3]], pos), lambda: hip_ops.voxel_sample([vol[:1]], pos),
           lambda: pointvoxel.trilinear_devoxelize(vol, pos.permute(0, 2, 1), 8),
           lambda: hip_ops.avg_voxelize_fwd(feat.cpu(), coords, 4), lambda: hip_ops.avg_voxelize_fwd(feat, coords.long(), 4),
           lambda: hip_ops.avg_voxelize_fwd(feat.double(), coords, 4), lambda: hip_ops.avg_voxelize_fwd(feat, coords[:1], 4),
           lambda: hip_ops.trilinear_devoxelize_fwd(3, True, pos.permute(0, 2, 1).contiguous(), vol.view(2, 3, 64)),
           lambda: hip_ops.trilinear_devoxelize_fwd(4, True, pos[:1].permute(0, 2, 1).contiguous(), vol.view(2, 3, 64)),
           lambda: hip_ops.trilinear_devoxelize_bwd(feat, coords.float(), coords.float(), 4)]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail("case %d did not raise" % k)
