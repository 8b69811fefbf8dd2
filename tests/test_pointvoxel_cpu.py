"""CPU tests of the point-voxel operators: the restatements of tests/pointvoxel_ref.py reproduce the recorded
outputs of the reference's kernels (tests/golden/pointvoxel_*.npz, gen_pointvoxel.py), the fp64 sampler equals the reference's
grid_sample composition with its border rule, the C ABI carries the new symbols, and the overlay hook binds them."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import pointvoxel_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["r2", "r8", "onevoxel"]
NEW_SYMBOLS = ["deftet_pointvoxel_workspace_bytes", "deftet_avg_voxelize_fwd_f32", "deftet_avg_voxelize_bwd_f32",
               "deftet_voxel_sample_fwd_f32", "deftet_voxel_cells_f32", "deftet_voxel_cells_from_inds_i32",
               "deftet_voxel_sample_bwd_vol_f32", "deftet_voxel_sample_bwd_pos_f32"]


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "pointvoxel_%s.npz" % name))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_voxelization_restatement_reproduces_the_reference_kernel(name):
    g = golden(name)
    out, ind, cnt = ref.avg_voxelize(g["feat"], g["coords"], int(g["R"]))
    assert np.array_equal(ind, g["ind"]) and np.array_equal(cnt, g["cnt"])
    assert np.array_equal(bits(out), bits(g["out"]))
    assert np.array_equal(bits(ref.avg_voxelize_bwd(g["gy"], ind, cnt)), bits(g["gx"]))


@pytest.mark.parametrize("name", CASES)
def test_legacy_devoxelization_restatement_reproduces_the_reference_kernel(name):
    g = golden(name)
    r = int(g["R"])
    outs, inds, wgts = ref.legacy_devoxelize(g["dv_coords"], g["dv_feat"], r)
    assert np.array_equal(inds, g["dv_inds"])
    assert np.array_equal(bits(wgts), bits(g["dv_wgts"]))
    assert np.array_equal(bits(outs), bits(g["dv_outs"]))
    gx = ref.legacy_devoxelize_bwd(g["dv_gy"], inds, wgts, r)
    scale = np.abs(gx).max()
    assert np.abs(gx - g["dv_gx"]).max() / scale <= 1e-5


def _inputs(R, C, N, seed, B=2):
    gen = torch.Generator().manual_seed(seed)
    vol = torch.randn(B, C, R, R, R, generator=gen, dtype=torch.float64)
    pos = 1.05 * (torch.rand(B, N, 3, generator=gen, dtype=torch.float64) - 0.5)
    pos[:, :4] = torch.tensor([[-0.5, 0.5, 0.6], [0.5, -0.5, -0.7], [0.5 - 1.0 / R, 0.0, 0.25], [0.0, 0.5 - 1.0 / R, -0.5]], dtype=torch.float64)
    return vol, pos


@pytest.mark.parametrize("R", [2, 5, 8, 32])
def test_fp64_sampler_equals_the_grid_sample_composition(R):
    vol, pos = _inputs(R, 3, 200, R)
    gout = torch.randn(2, 3, 200, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    res = []
    for fn in (lambda v, p: ref.voxel_sample([v], p), lambda v, p: ref.sample_f_composition(p, [v])):
        v, p = vol.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        out = fn(v, p)
        out.backward(gout)
        res.append((out.detach(), v.grad, p.grad))
    for a, b, what in zip(res[0], res[1], ("values", "grad_vol", "grad_pos")):
        assert (a - b).abs().max() <= 1e-12 * max(1.0, float(b.abs().max())), what
    # the border rule: a coordinate at -0.5, +0.5, beyond, or at u = r - 1 exactly gets no gradient
    gp = res[0][2]
    assert torch.all(gp[:, 0] == 0) and torch.all(gp[:, 1] == 0)
    assert torch.all(gp[:, 2, 0] == 0) and torch.all(gp[:, 3, 1] == 0) and torch.all(gp[:, 3, 2] == 0)
    if R > 2:
        assert torch.all(gp[:, 2, 1:] != 0)


def test_fp64_sampler_takes_the_right_hand_cell_at_an_interior_integer():
    R = 4
    vol = torch.arange(R, dtype=torch.float64).pow(2).view(1, 1, R, 1, 1).expand(1, 1, R, R, R).contiguous()      # f(x) = x^2
    pos = torch.tensor([[[1.0 / R - 0.5, 0.1, 0.1]]], dtype=torch.float64, requires_grad=True)                    # u_x = 1 exactly
    ref.voxel_sample([vol], pos).sum().backward()
    assert float(pos.grad[0, 0, 0]) == pytest.approx(R * (4.0 - 1.0), rel=1e-12)                                                             # slope of [1,2], times r


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(deftet_\w+)\s*\(", txt))


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from deftet_amd import _lib, build
    build.build()
    syms = header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s), s
    loaded = _lib.load()
    assert loaded.deftet_pointvoxel_workspace_bytes(8, 46656, 32) > 8 * 46656 * 4
    st = loaded.deftet_avg_voxelize_fwd_f32(None, None, None, None, None, 1, 1, 1, 0, None, 0, None)
    assert st == -1 and b"resolution" in loaded.deftet_last_error()
    st = loaded.deftet_voxel_sample_fwd_f32(None, None, None, None, None, 1, 4, 2, 1, 2, 5, 0, 0, None)
    assert st == -1 and b"channel offset" in loaded.deftet_last_error()


def test_overlay_binds_the_point_voxel_modules_only_on_request():
    from deftet_amd import overlay, pointvoxel
    names = ("layers.pv_module.functional.backend", "layers.pv_module.functional.devoxelization")
    saved = {n: sys.modules.pop(n) for n in list(sys.modules) if n in names}
    try:
        done = overlay.install(kaolin=False)
        assert not any(n in sys.modules for n in names)
        overlay.uninstall(done)
        done = overlay.install(kaolin=False, point_voxel=True)
        assert all(n in done for n in names)
        assert sys.modules[names[0]]._backend is pointvoxel.backend
        dv = sys.modules[names[1]]
        assert dv.trilinear_devoxelize is pointvoxel.trilinear_devoxelize and dv.trilinear_devoxelize_ori is pointvoxel.trilinear_devoxelize_ori
        overlay.uninstall(done)
        assert not any(n in sys.modules for n in names)
    finally:
        sys.modules.update(saved)


def test_unimplemented_backend_methods_raise_by_name():
    from deftet_amd import pointvoxel
    assert len(pointvoxel.UNIMPLEMENTED) == 8
    for name in pointvoxel.UNIMPLEMENTED:
        with pytest.raises(NotImplementedError, match=name):
            getattr(pointvoxel.backend, name)(None)
    for name in ("avg_voxelize_forward", "avg_voxelize_backward", "trilinear_devoxelize_forward", "trilinear_devoxelize_backward"):
        assert callable(getattr(pointvoxel.backend, name))


def test_front_ends_refuse_cpu_tensors():
    from deftet_amd import hip_ops, pointvoxel
    with pytest.raises(RuntimeError):
        hip_ops.voxel_sample([torch.zeros(1, 2, 4, 4, 4)], torch.zeros(1, 5, 3))
    with pytest.raises(RuntimeError):
        pointvoxel.avg_voxelize(torch.zeros(1, 2, 5), torch.zeros(1, 3, 5, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError):
        pointvoxel.backend.trilinear_devoxelize_forward(4, True, torch.zeros(1, 3, 5), torch.zeros(1, 2, 64))
