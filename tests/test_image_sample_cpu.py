"""CPU tests of the pixel-aligned image-feature operator: the restatement of tests/image_sample_ref.py against
F.grid_sample in fp64 (values and both gradients, both paddings, both align_corners), the two projection helpers of
deftet_amd/imagefeat.py, the symbols of the C ABI with their workspace check, and the front end's argument errors."""
import ctypes
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import image_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SYMBOLS = ["deftet_image_sample_workspace_bytes", "deftet_image_sample_fwd_f32", "deftet_image_cells_f32", "deftet_image_sample_bwd_map_f32",
           "deftet_image_sample_bwd_uv_f32", "deftet_image_sample_bwd_global_f32"]

_raw = ctypes.create_string_buffer(1 << 12)
P = ctypes.c_void_p((ctypes.addressof(_raw) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib, build
    build.build()
    return _lib.load()


def all_cells_uv(B, H, W, align, g):
    """every cell from -2 to W (and H) inclusive, three points each"""
    cy, cx = torch.meshgrid(torch.arange(-2, H + 1), torch.arange(-2, W + 1), indexing="ij")
    cx, cy = cx.reshape(1, -1).repeat(B, 3), cy.reshape(1, -1).repeat(B, 3)
    return ref.interior_uv(B, cx.shape[1], H, W, align, g, cells=(cx, cy))


@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
@pytest.mark.parametrize("H,W,align", [(H, W, a) for H, W in ((1, 1), (2, 3), (5, 4), (8, 8)) for a in (False, True)
                                       if not (a and min(H, W) == 1)])     # align_corners=True maps -1 .. 1 onto zero pixels at a side of 1
def test_restatement_is_grid_sample_in_fp64(H, W, align, padding_mode):
    g = torch.Generator().manual_seed(H * 10 + W)
    B, C = 2, 3
    uv32 = all_cells_uv(B, H, W, align, g)
    m0 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gout = torch.randn(B, C, uv32.shape[1], generator=g, dtype=torch.float64)
    res = []
    for fn in (lambda m, uv: ref.sample_map(m, uv, padding_mode, align),
               lambda m, uv: F.grid_sample(m, uv.unsqueeze(2), mode="bilinear", padding_mode=padding_mode, align_corners=align).squeeze(3)):
        m, uv = m0.clone().requires_grad_(True), uv32.double().requires_grad_(True)
        out = fn(m, uv)
        out.backward(gout)
        res.append((out.detach(), m.grad, uv.grad))
    for name, a, b in zip(("values", "grad_map", "grad_uv"), *res):
        d = float((a - b).abs().max())
        print("image_sample_ref vs grid_sample %dx%d %s align=%s %s: %.3g" % (H, W, padding_mode, align, name, d))
        assert d <= 1e-12, (name, d)
    if padding_mode == "zeros":                                       # the construction does reach fully-outside points and partial cells
        assert bool((res[0][0] == 0).all(1).any()) and bool((res[0][2] != 0).any())


def test_hostile_coordinates_in_the_restatement():
    g = torch.Generator().manual_seed(1)
    m = torch.randn(1, 2, 4, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    bad = torch.tensor([1e30, -1e30, float("inf"), -float("inf"), float("nan")])
    uv = torch.stack([torch.cat([bad, torch.zeros(5)]), torch.cat([torch.zeros(5), bad])], -1)[None].double().requires_grad_(True)
    out = ref.sample_map(m, uv, "zeros")
    out.sum().backward()
    assert not out.any() and not uv.grad.any() and not m.grad.any()
    m.grad = uv.grad = None
    out = ref.sample_map(m, uv, "border")
    out.sum().backward()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(m.grad).all())
    assert not uv.grad[0, :5, 0].any() and not uv.grad[0, 5:, 1].any()
    assert torch.equal(out[0, :, 4], 0.5 * (m[0, :, 1, 0] + m[0, :, 2, 0]).detach())      # NaN reads pixel 0 along x; v = 0 is row 1.5


def test_layout_of_the_restatement():
    g = torch.Generator().manual_seed(2)
    maps = [torch.randn(2, 3, 4, 4, generator=g), torch.randn(2, 2, 2, 3, generator=g)]
    uv, glob, app = torch.rand(2, 7, 2, generator=g) * 2 - 1, torch.randn(2, 5, generator=g), torch.randn(2, 7, 3, generator=g)
    out = ref.image_sample(maps, uv, glob, app)
    assert out.shape == (2, 5 + 3 + 2 + 3, 7)
    assert torch.equal(out[:, :5], glob[:, :, None].expand(2, 5, 7)) and torch.equal(out[:, 10:], app.permute(0, 2, 1))
    assert torch.equal(out[:, 5:8], ref.sample_map(maps[0], uv)) and torch.equal(out[:, 8:10], ref.sample_map(maps[1], uv))
    assert ref.image_sample([], uv).shape == (2, 0, 7)


# ---------------------------------------------------------------------------- projection helpers
def test_project_to_image_is_perspective_with_y_negated():
    from deftet_amd import imagefeat
    from deftet_amd.render.camera import perspective
    g = torch.Generator().manual_seed(3)
    B, N = 2, 50
    pos = torch.rand(B, N, 3, generator=g, dtype=torch.float64) - 0.5
    rot = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64))[0]
    cam_pos = torch.tensor([[0.1, -0.2, 3.0], [0.0, 0.3, 2.5]], dtype=torch.float64)
    proj = torch.tensor([[2.7], [2.6], [-1.0]], dtype=torch.float64)
    _, xy = perspective(pos, (rot, cam_pos, proj))
    want = xy * torch.tensor([1.0, -1.0], dtype=torch.float64)
    uv = imagefeat.project_to_image(pos, rot, cam_pos, proj)
    assert uv.shape == (B, N, 2) and float((uv - want).abs().max()) <= 1e-12
    assert float((imagefeat.project_to_image(pos, rot, cam_pos, proj, flip_y=False) - xy).abs().max()) <= 1e-12
    p = pos.clone().requires_grad_(True)
    imagefeat.project_to_image(p, rot, cam_pos, proj).sum().backward()
    assert p.grad is not None and bool(p.grad.abs().sum() > 0)


def test_project_with_matrix_is_the_homogeneous_product():
    from deftet_amd import imagefeat
    g = torch.Generator().manual_seed(4)
    B, N = 2, 40
    pos = torch.rand(B, N, 3, generator=g, dtype=torch.float64) - 0.5
    M = torch.randn(B, 4, 4, generator=g, dtype=torch.float64)
    M[:, 3, 2] += 4.0                                                  # keep the divisor away from 0
    uv = imagefeat.project_with_matrix(pos, M)
    assert uv.shape == (B, N, 2)
    for b, n in itertools.product(range(B), range(0, N, 7)):
        h = [float(pos[b, n, 0]), float(pos[b, n, 1]), float(pos[b, n, 2]), 1.0]
        comp = [sum(h[i] * float(M[b, i, j]) for i in range(4)) for j in range(3)]
        assert abs(float(uv[b, n, 0]) - comp[0] / comp[2]) <= 1e-12 and abs(float(uv[b, n, 1]) - comp[1] / comp[2]) <= 1e-12


# ---------------------------------------------------------------------------- the front end and the C ABI
def test_front_end_refuses_cpu_tensors():
    from deftet_amd import hip_ops, imagefeat
    m, uv = torch.zeros(1, 2, 4, 4), torch.zeros(1, 5, 2)
    for call in (lambda: hip_ops.image_sample([m], uv),
                 lambda: hip_ops.image_sample([], uv, global_features=torch.zeros(1, 3)),
                 lambda: imagefeat.extract_point_image_features(m, torch.zeros(1, 5, 3), torch.eye(4)[None]),
                 lambda: imagefeat.sample_f(torch.rand(1, 5, 3), [torch.zeros(1, 3), m], torch.tensor([[0.0, 0.0, 3.0]]), torch.eye(3)[None],
                                            torch.tensor([[2.0], [2.0], [-1.0]]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_header_ctypes_table_and_library_agree_on_the_symbols(lib):
    from deftet_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deftet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", txt))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 360


@pytest.mark.parametrize("B,N,H,W", [(1, 1, 1, 1), (2, 257, 5, 4), (8, 46656, 64, 64)])
def test_workspace_is_the_layout_and_one_byte_short_is_refused(lib, B, N, H, W):
    """both entries that take a workspace carve the same layout: one byte short is refused before any device call, the exact size
    passes on to the pointer checks"""
    want = lib.deftet_image_sample_workspace_bytes(B, N, H, W)
    assert want > 0 and want % 256 == 0
    assert want >= 16 * B * (H + 1) * (W + 1) + 8 * B * N                # a channel of partials and the sort's keys at the least
    assert lib.deftet_image_sample_workspace_bytes(B, 2 * N + 4096, H, W) > want
    cells, bwd = lib.deftet_image_cells_f32, lib.deftet_image_sample_bwd_map_f32
    assert cells(P, P, P, P, B, N, H, W, 0, 0, P, want - 1, None) == EINVAL and b"workspace" in lib.deftet_last_error()
    assert cells(P, P, None, P, B, N, H, W, 0, 0, P, want, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert bwd(P, P, P, P, P, B, 3, H, W, N, 0, 3, P, want - 1, None) == EINVAL and b"workspace" in lib.deftet_last_error()
    assert bwd(P, P, P, P, None, B, 3, H, W, N, 0, 3, P, want, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert cells(P, P, P, P, B, N, H, W, 0, 0, None, want, None) == EINVAL
    assert cells(P, P, P, P, B, N, H, W, 0, 0, ctypes.c_void_p(P.value + 16), want, None) == EINVAL and b"misaligned" in lib.deftet_last_error()


def test_bad_arguments_are_refused_by_name(lib):
    big = 1 << 40
    fwd, uvb, glob = lib.deftet_image_sample_fwd_f32, lib.deftet_image_sample_bwd_uv_f32, lib.deftet_image_sample_bwd_global_f32
    assert fwd(P, P, None, None, P, 1, 2, 0, 4, 5, 0, 0, 0, 2, 0, 0, None) == EINVAL and b"map side" in lib.deftet_last_error()
    assert fwd(P, P, None, None, P, 1, 2, 4, 4, 5, 0, 0, 1, 2, 0, 0, None) == EINVAL and b"exceed the destination" in lib.deftet_last_error()
    assert fwd(P, P, P, None, P, 1, 2, 4, 4, 5, 3, 0, 2, 5, 0, 0, None) == EINVAL and b"overlap" in lib.deftet_last_error()
    assert fwd(P, P, None, None, P, 1, 2, 4, 4, 5, 0, 0, 0, 2, 2, 0, None) == EINVAL and b"0 or 1" in lib.deftet_last_error()
    assert fwd(None, P, None, None, P, 1, 2, 4, 4, 5, 0, 0, 0, 2, 0, 0, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert fwd(P, P, None, None, P, 70000, 2, 4, 4, 5, 0, 0, 0, 2, 0, 0, None) == -4
    assert uvb(P, P, P, None, 1, 2, 4, 4, 5, 0, 2, 0, 0, 0, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert uvb(P, P, P, P, 1, 2, 4, 4, 5, 1, 2, 0, 0, 0, None) == EINVAL and b"exceed the source" in lib.deftet_last_error()
    assert glob(P, None, 2, 3, 5, 10, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert glob(P, P, 2, 11, 5, 10, None) == EINVAL
    assert lib.deftet_image_cells_f32(P, P, P, P, 1, 5, 4, 4, 0, 3, P, big, None) == EINVAL and b"0 or 1" in lib.deftet_last_error()
    assert lib.deftet_image_sample_workspace_bytes(-1, 5, 4, 4) == 0 and lib.deftet_image_sample_workspace_bytes(1, 5, 0, 4) == 0
    # nothing to do: accepted without a device call
    assert fwd(P, P, None, None, P, 0, 2, 4, 4, 5, 0, 0, 0, 2, 0, 0, None) == 0 and fwd(P, P, None, None, P, 1, 2, 4, 4, 0, 0, 0, 0, 2, 0, 0, None) == 0
