"""GPU tests of rendering straight from the vertices: the face CSR against a host construction, the gather
against torch indexing and its backward against an exact slot-ordered oracle (bit for bit, fan and degree-0 vertices included),
the projection and its backward against the fp64 restatement, render_vertices against the three operators chained by hand (bit
for bit, gradients too), and model_forward on a stub model."""
import types

import numpy as np
import pytest
import torch

from deftet_amd import grids
from tests import render_vertices_ref as R
from tests.tol import check_close

pytestmark = pytest.mark.gpu

NEAREST, FIRST = 0, 1
FOCAL, MULT = 1111.0 / 800.0 * 2.0, 1000.0


def cameras(B, dev, dtype=torch.float32):
    """B views around the origin at distance 4 looking down -z: cam = R p - (0, 0, 4)"""
    rots = []
    for b in range(B):
        ax, ay = 0.35 + 0.4 * b, 0.5 - 0.9 * b
        rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        rots.append(rx @ ry)
    rot = np.stack(rots).astype(np.float32)
    pos = np.stack([r.T @ np.array([0, 0, 4.0], np.float32) for r in rot]).astype(np.float32)
    proj = np.array([[FOCAL], [FOCAL], [-1.0]], np.float32)
    return tuple(torch.from_numpy(x).to(dev).to(dtype) for x in (rot, pos, proj))


def fan_faces(n):
    i = np.arange(1, n + 1)
    return np.stack([np.zeros(n, np.int64), i, i + 1], 1)                          # vertex 0 has degree n; V = n + 2


@pytest.fixture(scope="module")
def lists(oracle):
    """name -> (faces int64 [F,3], V)"""
    verts, tets = grids.kuhn_grid(8)
    f3 = np.asarray(oracle.tet_to_face(tets, verts.shape[0], with_boundary=True)[0], np.int64)
    assert verts.shape[0] == 125 and np.bincount(f3.reshape(-1)).max() == 36         # a Kuhn interior vertex
    return {"kuhn8": (f3, 125), "fan1500": (fan_faces(1500), 1502), "unreferenced": (f3[::3] + 3, 125 + 70),
            "one_vertex": (np.zeros((2, 3), np.int64), 1), "no_face": (np.zeros((0, 3), np.int64), 5)}


@pytest.fixture(scope="module")
def kuhn_points():
    verts, _ = grids.kuhn_grid(8)
    return ((verts - 0.5) * 2.5 + np.random.default_rng(1).normal(size=verts.shape) * 0.02).astype(np.float32)


def topo(lists, name, dev):
    from deftet_amd import hip_ops
    faces, V = lists[name]
    return hip_ops.FaceTopology(torch.from_numpy(faces).to(dev), V)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["kuhn8", "fan1500", "unreferenced", "one_vertex", "no_face"])
def test_csr_equals_the_host_construction(cuda, lists, name):
    faces, V = lists[name]
    t = topo(lists, name, cuda)
    offsets, slots = R.face_vertex_csr(faces, V)
    assert t.offsets.dtype == torch.int32 and t.slots.dtype == torch.int32
    assert np.array_equal(t.offsets.cpu().numpy(), offsets) and np.array_equal(t.slots.cpu().numpy(), slots)
    assert t.faces.dtype == torch.int64 and np.array_equal(t.faces.cpu().numpy(), faces) and (t.n_vertex, t.n_face) == (V, faces.shape[0])


def test_out_of_range_index_sets_the_flag_and_raises(cuda, lists):
    from deftet_amd import _lib, hip_ops
    faces, V = lists["kuhn8"]
    for bad_value in (-1, V):
        bad = torch.from_numpy(faces).to(cuda).clone()
        bad[7, 1] = bad_value
        with pytest.raises(RuntimeError, match="out of range"):
            hip_ops.FaceTopology(bad, V)
        lib, F = _lib.load(), faces.shape[0]
        offsets, slots = torch.empty(V + 1, device=cuda, dtype=torch.int32), torch.empty(3 * F, device=cuda, dtype=torch.int32)
        flag = torch.zeros(1, device=cuda, dtype=torch.int32)
        ws = _lib.workspace(cuda, lib.deftet_face_vertex_csr_workspace_bytes(V, F))
        _lib.check(lib.deftet_face_vertex_csr_i32(bad.data_ptr(), offsets.data_ptr(), slots.data_ptr(), flag.data_ptr(), V, F, ws.data_ptr(),
                                                  ws.numel(), _lib.current_stream(cuda)), "csr")
        assert flag.item() == 1 and offsets[-1].item() == 3 * F - 1                      # the bad incidence belongs to nobody
        # the gather writes NaN corners for it and sets its own flag, as tet_gather does
        z, xy, act = torch.rand(1, V, device=cuda), torch.rand(1, V, 2, device=cuda), torch.rand(1, V, 4, device=cuda)
        fz, fxy, ff = torch.empty(1, F, 3, device=cuda), torch.empty(1, F, 3, 2, device=cuda), torch.empty(1, F, 3, 4, device=cuda)
        flag.zero_()
        _lib.check(lib.deftet_face_gather_fwd_f32(z.data_ptr(), xy.data_ptr(), act.data_ptr(), bad.data_ptr(), fz.data_ptr(), fxy.data_ptr(),
                                                  ff.data_ptr(), flag.data_ptr(), 1, V, F, 4, _lib.current_stream(cuda)), "gather")
        assert flag.item() == 1
        nan = torch.isnan(fz)
        assert nan[0, 7, 1] and nan.sum() == 1 and torch.isnan(fxy[0, 7, 1]).all() and torch.isnan(ff[0, 7, 1]).all()
        assert torch.isnan(fxy).sum() == 2 and torch.isnan(ff).sum() == 4
    ok = torch.from_numpy(faces).to(cuda)
    t = hip_ops.FaceTopology(ok, V)
    ok[0, 0] = 99                                                                        # the topology holds its own copy
    assert t.faces[0, 0].item() == faces[0, 0]


# ---------------------------------------------------------------------------------------------------------------- 2, 3
def vertex_arrays(B, V, Do, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).to(dev) for s in ((B, V), (B, V, 2), (B, V, Do))]


@pytest.mark.parametrize("B,Do", [(1, 4), (2, 5)])
@pytest.mark.parametrize("name", ["kuhn8", "fan1500", "unreferenced", "one_vertex", "no_face"])
def test_face_gather_equals_torch_indexing_and_the_slot_ordered_oracle(cuda, lists, name, B, Do):
    from deftet_amd import hip_ops
    faces, V = lists[name]
    F = faces.shape[0]
    t = topo(lists, name, cuda)
    z, xy, act = vertex_arrays(B, V, Do, cuda, seed=V + B)
    xy.requires_grad_(True)
    act.requires_grad_(True)
    fz, fxy, ff = hip_ops.face_gather(z, xy, act, t)
    wz, wxy, wf = R.face_gather(z, xy.detach(), act.detach(), torch.from_numpy(faces).to(cuda))
    assert fz.shape == (B, F, 3) and fxy.shape == (B, F, 3, 2) and ff.shape == (B, F, 3, Do)
    assert torch.equal(fz, wz) and torch.equal(fxy, wxy) and torch.equal(ff, wf)
    assert not fz.requires_grad and fxy.requires_grad and ff.requires_grad
    # backward: values of very different magnitude, so that another order of the additions shows in the bits
    g = torch.Generator().manual_seed(F + Do)
    gfxy = (torch.randn(B, F, 3, 2, generator=g) * torch.exp(3 * torch.randn(B, F, 3, 2, generator=g))).to(cuda)
    gff = (torch.randn(B, F, 3, Do, generator=g) * torch.exp(3 * torch.randn(B, F, 3, Do, generator=g))).to(cuda)
    gxy, gact = torch.autograd.grad((fxy, ff), (xy, act), (gfxy, gff), retain_graph=True)
    table, maxdeg = R.slot_table(*R.face_vertex_csr(faces, V), V)
    assert maxdeg == {"kuhn8": 36, "fan1500": 1500, "unreferenced": 16, "one_vertex": 6, "no_face": 0}[name]
    want_xy, want_act = R.slot_ordered_sum(gfxy, table), R.slot_ordered_sum(gff, table)
    assert gxy.dtype == torch.float32 and torch.equal(gxy, want_xy) and torch.equal(gact, want_act)
    gxy2, gact2 = torch.autograd.grad((fxy, ff), (xy, act), (gfxy, gff), retain_graph=True)
    assert torch.equal(gxy, gxy2) and torch.equal(gact, gact2)                          # two runs, the same bits
    deg0 = torch.from_numpy(np.bincount(faces.reshape(-1), minlength=V) == 0).to(cuda)
    assert (gxy[:, deg0] == 0).all() and (gact[:, deg0] == 0).all()
    if name in ("unreferenced", "no_face"):
        assert deg0.any()
    # a gradient for one of the two outputs only: the other sum is zero
    only_act, = torch.autograd.grad(ff, act, gff, retain_graph=True)
    assert torch.equal(only_act, want_act)
    only_xy, = torch.autograd.grad(fxy, xy, gfxy)
    assert torch.equal(only_xy, want_xy)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
@pytest.mark.parametrize("shared_feat", [True, False], ids=["feat_shared", "feat_per_view"])
@pytest.mark.parametrize("shared_pos", [True, False], ids=["pos_shared", "pos_per_view"])
@pytest.mark.parametrize("B", [1, 2])
def test_project_vertices_against_fp64(cuda, kuhn_points, B, shared_pos, shared_feat, depth):
    from deftet_amd import hip_ops
    rng = np.random.default_rng(10 * B + 2 * shared_pos + shared_feat)
    for V in (125, 1):
        p = kuhn_points[:V] if shared_pos else np.stack([kuhn_points[:V] + np.float32(0.05 * b) for b in range(B)])
        f = rng.normal(size=(V, 4) if shared_feat else (B, V, 4)).astype(np.float32) * 2
        p32, f32 = (torch.from_numpy(x).to(cuda).requires_grad_(True) for x in (p, f))
        p64, f64 = (torch.from_numpy(x).to(cuda).double().requires_grad_(True) for x in (p, f))
        z, xy, act = hip_ops.project_vertices(p32, f32, cameras(B, cuda), MULT, depth)
        z64, xy64, act64 = R.project_vertices(p64, f64, cameras(B, cuda, torch.float64), MULT, depth)
        Do = 5 if depth else 4
        assert z.shape == (B, V) and xy.shape == (B, V, 2) and act.shape == (B, V, Do) and not z.requires_grad
        tag = "project_vertices %%s, V=%d B=%d pos %s feat %s depth=%d vs fp64" % (V, B, "shared" if shared_pos else "per view",
                                                                               "shared" if shared_feat else "per view", depth)
        check_close(tag % "z", z, z64, 1e-5, elem_rel=1e-5)
        check_close(tag % "xy", xy, xy64, 1e-5, elem_rel=1e-5)
        check_close(tag % "act", act, act64, 1e-5, elem_rel=1e-5)
        if depth:
            assert torch.equal(act[..., 0], z)
        g = torch.Generator().manual_seed(V + B)
        gxy, gact = torch.randn(B, V, 2, generator=g).to(cuda), torch.randn(B, V, Do, generator=g).to(cuda)
        gp, gf = torch.autograd.grad((xy, act), (p32, f32), (gxy, gact))
        gp64, gf64 = torch.autograd.grad((xy64, act64), (p64, f64), (gxy.double(), gact.double()))
        assert gp.shape == p32.shape and gf.shape == f32.shape and gp.dtype == torch.float32
        check_close(tag % "grad_points", gp, gp64, 1e-5, elem_rel=1e-5)
        check_close(tag % "grad_features", gf, gf64, 1e-5, elem_rel=1e-5)


def test_project_vertices_shared_equals_repeated_forward(cuda, kuhn_points):
    """a shared [V,3] input gives the outputs of the same tensor repeated per view, bit for bit, without the repeat"""
    from deftet_amd import hip_ops
    p = torch.from_numpy(kuhn_points).to(cuda)
    f = torch.randn(125, 4, generator=torch.Generator().manual_seed(2)).to(cuda)
    cams = cameras(2, cuda)
    a = hip_ops.project_vertices(p, f, cams, MULT, True)
    b = hip_ops.project_vertices(p[None].repeat(2, 1, 1), f[None].repeat(2, 1, 1), cams, MULT, True)
    c = hip_ops.project_vertices(p[None], f, cams, MULT, True)
    for x, y, w in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, w)


# ---------------------------------------------------------------------------------------------------------------- 5
def render_scene(cuda, lists, kuhn_points, B, shared, depth):
    t = topo(lists, "kuhn8", cuda)
    g = torch.Generator().manual_seed(11 + B)
    p = torch.from_numpy(kuhn_points).to(cuda)
    f = torch.randn(125, 4, generator=g).to(cuda)
    if not shared:
        p = torch.stack([p + 0.03 * b for b in range(B)])
        f = torch.stack([f - 0.2 * b for b in range(B)])
    pix, rngs = (torch.from_numpy(x).to(cuda) for x in grids.pixel_grid(40))
    return t, p, f, cameras(B, cuda), pix, rngs


@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
@pytest.mark.parametrize("policy", [NEAREST, FIRST], ids=["nearest", "first"])
@pytest.mark.parametrize("B,shared", [(1, True), (2, True), (2, False)])
def test_render_vertices_equals_the_three_operators_chained_by_hand(cuda, lists, kuhn_points, B, shared, policy, depth):
    from deftet_amd import hip_ops
    from deftet_amd.render import deftet_sparse_render_composite, render_vertices
    t, p, f, cams, pix, rngs = render_scene(cuda, lists, kuhn_points, B, shared, depth)
    knum = 8                                                                             # saturates: the policies differ
    p1, f1 = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    colour, cover, dep = render_vertices(p1, f1, t, cams, pix, rngs, multiplier=MULT, knum=knum, policy=policy, depth=depth)
    assert colour.shape == (B, 1600, 3) and cover.shape == (B, 1600, 1) and (dep is None) == (not depth)
    assert 0.05 < (cover > 0).float().mean().item() and cover.max().item() > 0.5        # the mesh is in the picture
    # by hand, every stage on leaves of its own
    p2, f2 = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    z, xy, act = hip_ops.project_vertices(p2, f2, cams, MULT, depth)
    xy_l, act_l = xy.detach().requires_grad_(True), act.detach().requires_grad_(True)
    fz, fxy, ff = hip_ops.face_gather(z, xy_l, act_l, t)
    fxy_l, ff_l = fxy.detach().requires_grad_(True), ff.detach().requires_grad_(True)
    pixB, rngB = pix.expand(B, -1, -1), rngs.expand(B, -1, -1)
    c2, v2, d2, face = deftet_sparse_render_composite(pixB, rngB, fz, fxy_l, ff_l, knum=knum, policy=policy, depth=depth)
    assert (face[..., -1] >= 0).any()
    assert torch.equal(colour, c2) and torch.equal(cover, v2) and (not depth or torch.equal(dep, d2))
    g = torch.Generator().manual_seed(3)
    gc, gv, gd = (torch.randn(*s, generator=g).to(cuda) for s in (colour.shape, cover.shape, cover.shape))
    outs, gouts = ((colour, cover, dep), (gc, gv, gd)) if depth else ((colour, cover), (gc, gv))
    gp, gf = torch.autograd.grad(outs, (p1, f1), gouts)
    outs2 = (c2, v2, d2) if depth else (c2, v2)
    g_fxy, g_ff = torch.autograd.grad(outs2, (fxy_l, ff_l), gouts)
    g_xy, g_act = torch.autograd.grad((fxy, ff), (xy_l, act_l), (g_fxy, g_ff))
    gp2, gf2 = torch.autograd.grad((xy, act), (p2, f2), (g_xy, g_act))
    assert gp.shape == p.shape and gf.shape == f.shape
    assert torch.equal(gp, gp2) and torch.equal(gf, gf2)
    assert torch.isfinite(gp).all() and gp.abs().max() > 0 and gf.abs().max() > 0
    # and again: the whole gradient is reproducible
    p3, f3 = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out3 = render_vertices(p3, f3, t, cams, pix, rngs, multiplier=MULT, knum=knum, policy=policy, depth=depth)
    gp3, gf3 = torch.autograd.grad(out3 if depth else out3[:2], (p3, f3), gouts)
    assert torch.equal(gp, gp3) and torch.equal(gf, gf3)


# ---------------------------------------------------------------------------------------------------------------- 6
class StubModel:
    """the attributes and methods Deftet.forward reads (3_model/deftet.py:205-219, :427-470)"""

    def __init__(self, points, faces, dev, npix=40):
        g = torch.Generator().manual_seed(5)
        self.coef = 1.25
        self.tfpoint_px3 = (torch.from_numpy(points) / self.coef).to(dev)
        self.tfpointmov_px3 = (torch.randn(points.shape, generator=g) * 0.01).to(dev).requires_grad_(True)
        self.tfpointfeat_pxd = torch.randn(points.shape[0], 4, generator=g).to(dev).requires_grad_(True)
        self.tff_fx3 = torch.from_numpy(faces)                                          # a host tensor, as the reference keeps it
        a = (torch.arange(npix) + 0.5) / npix * 2 - 1
        self.xy_px2 = torch.stack(torch.meshgrid(a, a, indexing="xy"), -1).reshape(-1, 2).to(dev)
        self.multiplier = MULT

    def get_point(self, with_coef=False):
        p = self.tfpoint_px3 + self.tfpointmov_px3
        return self.coef * p if with_coef else p

    def get_feat(self):
        return self.tfpointfeat_pxd


@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
def test_model_forward_is_render_vertices_and_follows_the_face_list(cuda, lists, kuhn_points, depth):
    from deftet_amd import hip_ops
    from deftet_amd.render import model_forward, render_vertices
    faces, V = lists["kuhn8"]
    m = StubModel(kuhn_points, faces, cuda)
    sample = torch.arange(0, 1600, 3, device=cuda).reshape(-1, 2)                       # a subset of the pixels, any shape
    cams = cameras(2, cuda)
    out = model_forward(m, sample, *cams, depth=depth)
    assert len(out) == (3 if depth else 2) and out[0].shape == (2, sample.numel(), 3) and out[1].shape == (2, sample.numel(), 1)
    pix = (m.xy_px2[sample.reshape(-1)] * MULT)[None]
    rngs = torch.zeros_like(pix)
    rngs[..., 0] = -1000
    want = render_vertices(m.get_point(True), m.get_feat(), hip_ops.FaceTopology(m.tff_fx3, V, device=cuda), cams, pix, rngs,
                           multiplier=MULT, depth=depth)
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    assert (out[1] > 0).any()
    gm, gf = torch.autograd.grad(out[0].sum() + out[1].sum(), (m.tfpointmov_px3, m.tfpointfeat_pxd))
    assert gm.shape == (V, 3) and gf.shape == (V, 4) and gm.abs().max() > 0
    kept = m._deftet_face_topology[1]
    model_forward(m, sample, *cams, depth=depth)
    assert m._deftet_face_topology[1] is kept                                            # the same list object: kept
    m.tff_fx3 = torch.from_numpy(faces[: faces.shape[0] // 2].copy())                   # a new list object (deletetet): rebuilt
    out2 = model_forward(m, sample, *cams, depth=depth)
    assert m._deftet_face_topology[1] is not kept and m._deftet_face_topology[1].n_face == faces.shape[0] // 2
    want2 = render_vertices(m.get_point(True), m.get_feat(), hip_ops.FaceTopology(m.tff_fx3, V, device=cuda), cams, pix, rngs,
                            multiplier=MULT, depth=depth)
    assert torch.equal(out2[0], want2[0]) and not torch.equal(out2[0], out[0])
    with pytest.raises(AssertionError, match="viewpoint"):
        model_forward(m, sample, *cams, depth=depth, viewpoint=True)
