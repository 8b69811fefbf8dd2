"""Rendering from the vertices without a GPU: the torch restatement (tests/render_vertices_ref.py) reproduces the arrays the
reference wrote into tests/golden/render_glue.npz; the host construction of the face CSR has the properties the GPU one is held
to; the library exports the new entry points and rejects bad arguments before any device work."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from tests import render_vertices_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
SYMBOLS = ("deftet_face_vertex_csr_workspace_bytes", "deftet_face_vertex_csr_i32", "deftet_project_vertices_fwd_f32",
           "deftet_project_vertices_bwd_f32", "deftet_face_gather_fwd_f32", "deftet_face_gather_bwd_f32")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "render_glue.npz"))


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_restatement_reproduces_the_reference_arrays(gold, dtype):
    t = lambda k: torch.from_numpy(gold[k]).to(dtype if gold[k].dtype == np.float32 else torch.int64)   # noqa: E731
    cam, xy = R.perspective(t("persp_points"), (t("persp_rot"), t("persp_pos"), t("persp_proj")))
    np.testing.assert_allclose(cam.numpy(), gold["persp_cam"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(xy.numpy(), gold["persp_xy"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(R.face_attributes(t("v2f_features"), t("v2f_faces")).numpy(), gold["v2f_out"].astype(cam.numpy().dtype))
    c, v, d = R.alpha_composite(t("peel_ims"), t("peel_depth"))
    np.testing.assert_allclose(c.numpy(), gold["peel_color"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(v.numpy(), gold["peel_vis"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(d.numpy(), gold["peel_dep"], rtol=1e-6, atol=2e-6)
    c2, v2, d2 = R.alpha_composite(t("peel_ims"))
    assert d2 is None
    np.testing.assert_allclose(c2.numpy(), gold["peel_color_nodepth"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(v2.numpy(), gold["peel_vis_nodepth"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("tag,depth", [("d", True), ("n", False)])
def test_restatement_prepares_the_rasterizer_inputs_as_the_reference(gold, tag, depth):
    """rendermeshcolor's three gathers after the sigmoid (the depth channel not squashed) = face_gather of the per-vertex arrays"""
    t = lambda k: torch.from_numpy(gold[k])   # noqa: E731
    feat = t("rmc_feat")
    act = torch.cat([feat[..., :1], torch.sigmoid(feat[..., 1:])], -1) if depth else torch.sigmoid(feat[..., 1:])
    fz, fxy, ff = R.face_gather(t("rmc_points3d")[..., 2], t("rmc_points2d"), act, t("rmc_faces"))
    assert np.array_equal(fz.numpy(), gold["rmc_%s_arg_z" % tag]) and np.array_equal(fxy.numpy(), gold["rmc_%s_arg_img" % tag])
    np.testing.assert_allclose(ff.numpy(), gold["rmc_%s_arg_feat" % tag], rtol=1e-6, atol=1e-7)
    layers = t("rmc_%s_layers" % tag)
    c, v, d = R.alpha_composite(layers[..., 1:], layers[..., :1]) if depth else R.alpha_composite(layers)
    np.testing.assert_allclose(c.numpy(), gold["rmc_%s_color" % tag], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(v.numpy(), gold["rmc_%s_mask" % tag], rtol=1e-6, atol=1e-6)
    if depth:
        np.testing.assert_allclose(d.numpy(), gold["rmc_d_depth"], rtol=1e-6, atol=2e-6)


def test_project_restatement_shares_without_repeating_and_carries_the_depth_channel():
    g = torch.Generator().manual_seed(3)
    p, f = torch.randn(7, 3, generator=g, dtype=torch.float64), torch.randn(7, 4, generator=g, dtype=torch.float64)
    cams = (torch.linalg.qr(torch.randn(2, 3, 3, generator=g, dtype=torch.float64))[0], torch.randn(2, 3, generator=g, dtype=torch.float64) * 3,
            torch.tensor([1.3, 1.7, -1.0], dtype=torch.float64))
    z, xy, act = R.project_vertices(p, f, cams, multiplier=50.0, depth=True)
    z2, xy2, act2 = R.project_vertices(p[None].repeat(2, 1, 1), f[None].repeat(2, 1, 1), cams, multiplier=50.0, depth=True)
    assert torch.equal(z, z2) and torch.equal(xy, xy2) and torch.equal(act, act2)
    assert act.shape == (2, 7, 5) and torch.equal(act[..., 0], z) and torch.equal(act[..., 1:], torch.sigmoid(f).expand(2, -1, -1))
    cam = torch.matmul(p[None] - cams[1][:, None], cams[0].permute(0, 2, 1))
    assert torch.allclose(z, cam[..., 2], rtol=1e-13, atol=1e-13)
    assert torch.allclose(xy, cam[..., :2] * cams[2][:2] / (cam[..., 2:] * cams[2][2]) * 50.0, rtol=1e-12, atol=1e-12)


def test_host_csr_of_a_hand_made_list():
    faces = np.array([[0, 1, 2], [2, 1, 3], [5, 5, 0], [3, 2, 0], [1, 5, 2]])        # vertex 4 has no face, face 2 repeats a vertex
    V, F = 7, faces.shape[0]                                                          # vertices 4 and 6 are unreferenced
    offsets, slots = R.face_vertex_csr(faces, V)
    assert offsets.dtype == np.int32 and slots.dtype == np.int32 and offsets.shape == (V + 1,) and slots.shape == (3 * F,)
    deg = np.diff(offsets)
    assert offsets[0] == 0 and deg.sum() == 3 * F == offsets[-1] and (deg >= 0).all()
    assert deg.tolist() == [3, 3, 4, 2, 0, 3, 0]
    for v in range(V):
        mine = slots[offsets[v]:offsets[v + 1]]
        assert (np.diff(mine) > 0).all()                                              # ascending per vertex
        assert (faces.reshape(-1)[mine] == v).all()
    assert sorted(slots.tolist()) == list(range(3 * F))                               # every (f, corner) once
    assert slots[offsets[5]:offsets[6]].tolist() == [6, 7, 13]
    table, maxdeg = R.slot_table(offsets, slots, V)
    assert maxdeg == 4 and table.shape == (V, 4) and (table[4] == 3 * F).all() and table[2].tolist() == [2, 3, 10, 14]
    g = torch.arange(3 * F * 2, dtype=torch.float32).reshape(1, F, 3, 2)
    s = R.slot_ordered_sum(g, table)
    want = torch.zeros(1, V, 2).index_add_(1, torch.from_numpy(faces.reshape(-1)), g.reshape(1, -1, 2))
    assert torch.equal(s, want)                                                       # (small integers: every order is exact)


def test_library_exports_the_entry_points(lib):
    raw = ctypes.CDLL(importlib.import_module("deftet_amd._lib").LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    assert lib.deftet_version() >= 280
    assert lib.deftet_face_vertex_csr_workspace_bytes(46656, 521850) > 3 * 521850 * 4 * 3
    assert lib.deftet_face_vertex_csr_workspace_bytes(125, 0) == lib.deftet_tet_vertex_csr_workspace_bytes(1, 125, 0)


def _buf(nbytes=1 << 12, align=256, offset=0):
    raw = ctypes.create_string_buffer(nbytes + align * 2)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + align - 1) // align * align + offset)


def test_entry_points_reject_bad_arguments(lib):
    bufs = [_buf() for _ in range(12)]
    a = [b[1] for b in bufs]
    need = lib.deftet_face_vertex_csr_workspace_bytes(9, 4)
    csr = lib.deftet_face_vertex_csr_i32
    assert csr(a[0], a[1], a[2], a[3], -1, 4, a[4], need, None) == EINVAL
    assert csr(a[0], a[1], a[2], None, 9, 4, a[4], need, None) == EINVAL and b"null" in lib.deftet_last_error()
    assert csr(a[0], a[1], a[2], a[3], 1 << 30, 1 << 30, a[4], need, None) == EINVAL and b"too large" in lib.deftet_last_error()
    fwd = lib.deftet_project_vertices_fwd_f32
    ok = [a[0], a[1], a[2], a[3], a[4], 1.0, 0, a[5], a[6], a[7], 2, 9, 4, 1, 2, None]

    def call(fn, args, **kw):
        args = list(args)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return fn(*args)
    for kw in (dict(_10=-1), dict(_11=-2), dict(_12=0), dict(_13=3), dict(_14=0), dict(_0=None), dict(_4=None), dict(_9=None), dict(_10=70000)):
        assert call(fwd, ok, **kw) == EINVAL, kw
        assert lib.deftet_last_error()
    bwd = lib.deftet_project_vertices_bwd_f32
    ok = [a[0], a[1], a[2], a[3], a[4], a[5], a[6], 1.0, 1, a[7], a[8], 2, 9, 4, 2, 1, None]
    for kw in (dict(_11=-1), dict(_13=0), dict(_14=5), dict(_15=3), dict(_2=None), dict(_5=None), dict(_6=None)):
        assert call(bwd, ok, **kw) == EINVAL, kw
    assert call(bwd, ok, _9=None, _10=None) == 0                                      # nothing wanted: nothing launched
    gf = lib.deftet_face_gather_fwd_f32
    ok = [a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 2, 9, 4, 5, None]
    for kw in (dict(_8=-1), dict(_9=-1), dict(_10=-1), dict(_11=0), dict(_3=None), dict(_4=None), dict(_5=None), dict(_6=None), dict(_0=None),
               dict(_1=_buf(offset=4)[1]), dict(_5=_buf(offset=4)[1])):
        assert call(gf, ok, **kw) == EINVAL, kw
    assert call(gf, ok, _10=0) == 0
    gb = lib.deftet_face_gather_bwd_f32
    ok = [a[0], a[1], a[2], a[3], a[4], a[5], 2, 9, 4, 5, None]
    for kw in (dict(_6=-1), dict(_7=-1), dict(_8=-1), dict(_9=0), dict(_2=None), dict(_3=None), dict(_4=None), dict(_5=None)):
        assert call(gb, ok, **kw) == EINVAL, kw
    assert call(gb, ok, _7=0) == 0


def test_front_ends_import_and_refuse_cpu_tensors():
    from deftet_amd import hip_ops
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.render import model_forward, render_vertices
    faces = torch.tensor([[0, 1, 2]])
    with pytest.raises(DefTetHipError):
        hip_ops.FaceTopology(faces, 3)
    cams = (torch.eye(3)[None], torch.zeros(1, 3), torch.tensor([[1.0], [1.0], [-1.0]]))
    with pytest.raises(DefTetHipError):
        hip_ops.project_vertices(torch.zeros(3, 3), torch.zeros(3, 4), cams)
    with pytest.raises(TypeError):
        hip_ops.face_gather(torch.zeros(1, 3), torch.zeros(1, 3, 2), torch.zeros(1, 3, 4), faces)
    with pytest.raises(TypeError):
        render_vertices(torch.zeros(3, 3), torch.zeros(3, 4), faces, cams, torch.zeros(1, 5, 2), torch.zeros(1, 5, 2))
    with pytest.raises(AssertionError, match="viewpoint"):
        model_forward(object(), None, None, None, None, viewpoint=True)

