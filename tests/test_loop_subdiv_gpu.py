"""Loop subdivision on the GPU (hip_ops.LoopTopology, loop_subdivide, loop_limit, loop_subdivide_mesh, loop_subdivide_list and
the subdivide= keyword of the iso-surface helpers) against the float64 restatement tests/loop_subdiv_ref.py on the meshes of
tests/loop_subdiv_cases.py: every topology table bit for bit; positions, limit positions and attributes inside
(nnz_row + 3) 2^-24 (|S| |x|) per component, the gradients inside (nnz_col + 3) 2^-24 (|S|^T |g|) — the forward bound of an fp32
dot product with fp32-rounded weights, computed from the restated matrix; the same bits on every run, for every batch size and
through the ragged list."""
import numpy as np
import pytest
import torch

from tests import loop_subdiv_cases as K
from tests import loop_subdiv_ref as ref
from tests.tol import check_bound

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
DEV = "cuda"
NAMES = tuple(K.CASES)


@pytest.fixture(scope="module")
def ops():
    from deftet_amd import hip_ops
    return hip_ops


_TOPS = {}


def gpu_topology(ops, name):
    if name not in _TOPS:
        v, f = K.case(name)
        _TOPS[name] = ops.LoopTopology(torch.from_numpy(f).to(DEV), v.shape[0])
    return _TOPS[name]


def batch_of(name, B, seed=0):
    """[B,V,3] float32: shape 0 the case's own positions, the others N(0,1) perturbations of them"""
    v, _f = K.case(name)
    rng = np.random.default_rng(seed)
    return np.stack([v] + [(v + rng.normal(size=v.shape)).astype(np.float32) for _ in range(B - 1)])


# ---------------------------------------------------------------------------- topology
@pytest.mark.parametrize("name", NAMES)
def test_topology_tables_equal_the_restatement(ops, name):
    want = K.reference(name)[0]
    top = gpu_topology(ops, name)
    v, f = K.case(name)
    assert (top.n_vertex, top.n_face, top.n_edge, top.n_vertex_out) == (v.shape[0], f.shape[0], want.edges.shape[0], v.shape[0] + want.edges.shape[0])
    for field in ("faces", "edges", "face_edge", "edge_nface", "edge_opp", "vertex_kind", "crease_nbr", "ev_offsets", "ev_slots", "fv_offsets",
                  "fv_slots", "child_faces"):
        got, exp = getattr(top, field).cpu().numpy(), getattr(want, field)
        assert got.dtype == exp.dtype and got.shape == exp.shape, (field, got.dtype, exp.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), field


def test_refusals(ops):
    v, f = K.case("octahedron")
    bad = f.copy()
    bad[3, 1] = 6
    with pytest.raises(IndexError):
        ops.LoopTopology(torch.from_numpy(bad).to(DEV), 6)
    bad[3, 1] = -1
    with pytest.raises(IndexError):
        ops.LoopTopology(torch.from_numpy(bad).to(DEV), 6)
    twice = f.copy()
    twice[5, 2] = twice[5, 0]
    with pytest.raises(ValueError):
        ops.LoopTopology(torch.from_numpy(twice).to(DEV), 6)
    with pytest.raises(ValueError):
        ops.LoopTopology(torch.zeros(0, 3, dtype=torch.int64, device=DEV), 6)
    with pytest.raises(ValueError):
        ops.LoopTopology(torch.from_numpy(f).to(DEV), 0)
    with pytest.raises(TypeError):
        ops.loop_subdivide(torch.zeros(6, 3, device=DEV), ops.FaceTopology(torch.from_numpy(f).to(DEV), 6))


# ---------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_limit_inside_the_dot_product_bound(ops, name):
    _top, S, L = K.reference(name)
    top = gpu_topology(ops, name)
    x = batch_of(name, 2)
    V = x.shape[1]
    a = np.random.default_rng(3).normal(size=(2, V, 5)).astype(np.float32)
    got_v, got_a = ops.loop_subdivide(torch.from_numpy(x).to(DEV), top, torch.from_numpy(a).to(DEV))
    lim_v, lim_a = ops.loop_limit(torch.from_numpy(x).to(DEV), top, torch.from_numpy(a).to(DEV))
    assert got_v.shape == (2, top.n_vertex_out, 3) and got_a.shape == (2, top.n_vertex_out, 5) and lim_v.shape == (2, V, 3)
    for b in range(2):
        for what, M, got, src in (("verts'", S, got_v, x), ("attr'", S, got_a, a), ("limit", L, lim_v, x), ("limit attr", L, lim_a, a)):
            worst = check_bound("%s %s[%d]" % (name, what, b), got[b], M @ src[b].astype(np.float64), ref.forward_bound(M, src[b]))
            print("%s %s[%d]: %.3f of the bound" % (name, what, b, worst))
    only_v, none = ops.loop_subdivide(torch.from_numpy(x[0]).to(DEV), top)
    assert none is None and only_v.shape == (top.n_vertex_out, 3) and torch.equal(only_v, got_v[0])


# ---------------------------------------------------------------------------- backward
@pytest.mark.parametrize("C", (1, 3, 8))
@pytest.mark.parametrize("name", NAMES)
def test_backward_inside_the_transposed_bound(ops, name, C):
    _top, S, L = K.reference(name)
    top = gpu_topology(ops, name)
    B = 2
    V, R = top.n_vertex, top.n_vertex_out
    rng = np.random.default_rng(7 + C)
    x = torch.from_numpy(batch_of(name, B)).to(DEV).requires_grad_(True)
    a = torch.from_numpy(rng.normal(size=(B, V, C)).astype(np.float32)).to(DEV).requires_grad_(True)
    gv, ga = rng.normal(size=(B, R, 3)).astype(np.float32), rng.normal(size=(B, R, C)).astype(np.float32)
    out_v, out_a = ops.loop_subdivide(x, top, a)
    dx, da = torch.autograd.grad([out_v, out_a], [x, a], [torch.from_numpy(gv).to(DEV), torch.from_numpy(ga).to(DEV)])
    lim_v, lim_a = ops.loop_limit(x, top, a)
    lx, la = torch.autograd.grad([lim_v, lim_a], [x, a], [torch.from_numpy(gv[:, :V]).to(DEV), torch.from_numpy(ga[:, :V]).to(DEV)])
    for b in range(B):
        for what, M, got, g in (("grad verts", S, dx, gv), ("grad attr", S, da, ga), ("limit grad verts", L, lx, gv[:, :V]),
                                ("limit grad attr", L, la, ga[:, :V])):
            worst = check_bound("%s %s[%d]" % (name, what, b), got[b], M.T @ g[b].astype(np.float64), ref.backward_bound(M, g[b]))
            print("%s C=%d %s[%d]: %.3f of the bound" % (name, C, what, b, worst))
    # gradients with only verts' or only attr' supplied: the other input's gradient is exactly zero, the supplied one unchanged
    out_v, out_a = ops.loop_subdivide(x, top, a)
    dx1, da1 = torch.autograd.grad([out_v], [x, a], [torch.from_numpy(gv).to(DEV)], allow_unused=True)
    assert torch.equal(dx1, dx) and (da1 is None or not da1.any())
    out_v, out_a = ops.loop_subdivide(x, top, a)
    dx2, da2 = torch.autograd.grad([out_a], [x, a], [torch.from_numpy(ga).to(DEV)], allow_unused=True)
    assert torch.equal(da2, da) and (dx2 is None or not dx2.any())


# ---------------------------------------------------------------------------- the same bits
def _all(ops, x, top, a, gv, ga):
    x, a = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    out = ops.loop_subdivide(x, top, a)
    return out + torch.autograd.grad(list(out), [x, a], [gv, ga])


@pytest.mark.parametrize("name", ("smooth_fan200", "sphere20", "book"))
def test_same_bits_on_every_run_and_for_every_batch(ops, name):
    top = gpu_topology(ops, name)
    V, R = top.n_vertex, top.n_vertex_out
    rng = np.random.default_rng(1)
    x = torch.from_numpy(batch_of(name, 3)).to(DEV)
    a = torch.from_numpy(rng.normal(size=(3, V, 3)).astype(np.float32)).to(DEV)
    gv = torch.from_numpy(rng.normal(size=(3, R, 3)).astype(np.float32)).to(DEV)
    ga = torch.from_numpy(rng.normal(size=(3, R, 3)).astype(np.float32)).to(DEV)
    first, second = _all(ops, x, top, a, gv, ga), _all(ops, x, top, a, gv, ga)
    for p, q in zip(first, second):
        assert torch.equal(p, q)
    for b in range(3):
        alone = _all(ops, x[b:b + 1], top, a[b:b + 1], gv[b:b + 1], ga[b:b + 1])
        for p, q in zip(first, alone):
            assert torch.equal(p[b:b + 1], q)


def test_list_equals_the_per_shape_calls_bit_for_bit(ops):
    names = ("icosahedron", "sphere20", "flat_patch", "book", "smooth_fan200")
    rng = np.random.default_rng(2)
    vs = [torch.from_numpy(K.case(n)[0].copy()).to(DEV) for n in names] + [torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0.5]], device=DEV)]
    fs = [torch.from_numpy(K.case(n)[1].copy()).to(DEV) for n in names] + [torch.tensor([[0, 1, 2]], device=DEV)]
    vs.insert(2, torch.zeros(0, 3, device=DEV))                                       # a shape without faces comes back as it is
    fs.insert(2, torch.zeros(0, 3, dtype=torch.int64, device=DEV))
    ats = [torch.from_numpy(rng.normal(size=(v.shape[0], 4)).astype(np.float32)).to(DEV) for v in vs]
    for levels, limit in ((1, False), (2, True)):
        lv, lf, la = ops.loop_subdivide_list(vs, fs, ats, levels=levels, limit=limit)
        for i in range(len(vs)):
            if fs[i].shape[0] == 0:
                assert lv[i].shape[0] == 0 and lf[i].shape[0] == 0
                continue
            v, f, a = ops.loop_subdivide_mesh(vs[i], fs[i], ats[i], levels=levels, limit=limit)
            assert torch.equal(lv[i], v) and torch.equal(lf[i], f) and torch.equal(la[i], a), (i, levels)
    lv, lf, la = ops.loop_subdivide_list(vs, fs, None)
    assert la is None and lf[-1].shape == (4, 3) and lv[-1].shape == (6, 3)


# ---------------------------------------------------------------------------- two levels
def test_two_levels_on_the_sphere(ops):
    v, f = K.case("sphere20")
    x = torch.from_numpy(v.copy()).to(DEV).requires_grad_(True)
    v2, f2, none = ops.loop_subdivide_mesh(x, torch.from_numpy(f).to(DEV), levels=2)
    w2, g2, S21 = ref.subdivide(v, f, 2)
    assert none is None and f2.shape[0] == 16 * f.shape[0] and np.array_equal(f2.cpu().numpy(), g2)
    n_edge = ref.edge_face_counts(g2).shape[0]
    assert ops.face_edges(f2, v2.shape[0]).shape[0] == 2 * n_edge                     # directed pairs: both directions of every edge
    assert v2.shape[0] - n_edge + f2.shape[0] == 2                                    # still a sphere
    # a directional derivative against the float64 product S2 S1: <g, S d> from the forward of d, <S^T g, d> from the backward
    rng = np.random.default_rng(4)
    g = rng.normal(size=w2.shape).astype(np.float32)
    d = rng.normal(size=v.shape).astype(np.float32)
    (dx,) = torch.autograd.grad([v2], [x], [torch.from_numpy(g).to(DEV)])
    want = float((g.astype(np.float64) * (S21 @ d.astype(np.float64))).sum())
    scale = float((np.abs(g).astype(np.float64) * (abs(S21) @ np.abs(d).astype(np.float64))).sum())
    # two chained fp32 dot products of at most 12 and 8 terms, and the fp32 result rounded once more: (12 + 3 + 8 + 3 + 1) u
    tol = 27 * 2.0 ** -24 * scale
    from_bwd = float((dx.double().cpu().numpy() * d).sum())
    from_fwd = float((ops.loop_subdivide_mesh(torch.from_numpy(d).to(DEV), torch.from_numpy(f).to(DEV), levels=2)[0].double().cpu().numpy() * g).sum())
    print("directional derivative: want %.9g, backward %.9g, forward %.9g, tolerance %.3g" % (want, from_bwd, from_fwd, tol))
    assert abs(from_bwd - want) <= tol and abs(from_fwd - want) <= tol
    check_bound("two levels", v2, w2, 2 * ref.forward_bound(abs(S21), np.abs(v)))


# ---------------------------------------------------------------------------- end to end
class StubModel:
    """the attributes and methods the marching-tetrahedra routes read of a render model"""

    def __init__(self, points, tets):
        self.tfpoint_px3 = torch.from_numpy(points.copy()).to(DEV)
        self.tfpointmov_px3 = torch.zeros_like(self.tfpoint_px3).requires_grad_(True)
        feat = np.random.default_rng(6).normal(size=(points.shape[0], 4)).astype(np.float32)
        self.tfpointfeat_pxd = torch.from_numpy(feat).to(DEV).requires_grad_(True)
        self.tftet_tx4 = torch.from_numpy(tets.copy()).to(DEV)

    def get_point(self, with_coef=False):
        return self.tfpoint_px3 + self.tfpointmov_px3

    def get_feat(self):
        return self.tfpointfeat_pxd


def sphere_process(points, feat):
    return torch.sigmoid((0.3 - points.norm(dim=1, keepdim=True)) * 20 + 0.1 * feat[:, :1]), torch.sigmoid(feat[:, 1:4])


def _finite_nonzero(*grads):
    return all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)


def test_render_marching_tets_subdivide_keyword(ops, tmp_path):
    from deftet_amd.render import export, iso_surface
    from tests import marching_tets_cases as MK
    pos, tets, _e, _te = MK.grid(8, 1)
    model = StubModel(pos[0], tets)
    base = iso_surface.marching_tets(model, 0.25, sphere_process)
    zero = iso_surface.marching_tets(model, 0.25, sphere_process, subdivide=0)
    fine = iso_surface.marching_tets(model, 0.25, sphere_process, subdivide=1)
    assert base.faces.shape[0] > 20
    for x, y in zip(base, zero):
        assert (x is None and y is None) or torch.equal(x, y)
    assert fine.faces.shape[0] == 4 * base.faces.shape[0] and int(fine.faces.max()) == fine.verts.shape[0] - 1
    assert fine.vert_attr.shape == (fine.verts.shape[0], 3) and fine.edge_id is None
    want_v, want_f, want_a = ops.loop_subdivide_mesh(base.verts, base.faces, base.vert_attr)
    assert torch.equal(fine.verts, want_v) and torch.equal(fine.faces, want_f) and torch.equal(fine.vert_attr, want_a)
    gm, gf = torch.autograd.grad(fine.verts.square().sum() + fine.vert_attr.sum(), (model.tfpointmov_px3, model.tfpointfeat_pxd))
    assert _finite_nonzero(gm, gf)
    with pytest.raises(ValueError):
        iso_surface.marching_tets(model, 0.25, sphere_process, return_index=True, subdivide=1)
    plain = iso_surface.marching_tets_normals(model, 0.25, sphere_process)
    smooth = iso_surface.marching_tets_normals(model, 0.25, sphere_process, subdivide=2)
    assert smooth.faces.shape[0] == 16 * plain.faces.shape[0] and smooth.vert_attr.shape == smooth.verts.shape
    assert float((smooth.vert_attr.detach().norm(dim=1) - 1).abs().max()) <= 1e-5
    assert float((smooth.vert_attr * smooth.verts).detach().sum(1).min()) > 0                   # a sphere about the origin: still outward
    nbr = ops.tet_face_neighbours(tets, pos.shape[1], torch.device(DEV))
    w, col = sphere_process(model.get_point(True), model.get_feat())
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    old = export.save_surface_objs(model.get_point(True), (w, col), tets, nbr, str(tmp_path / "a"), "s", thresholds=(0.25,), iso=0.25, normals=True)
    new = export.save_surface_objs(model.get_point(True), (w, col), tets, nbr, str(tmp_path / "b"), "s", thresholds=(0.25,), iso=0.25, normals=True,
                                   subdivide=1)
    count = lambda path, tag: sum(1 for line in open(path) if line.startswith(tag))
    assert [q.rsplit("/", 1)[1] for q in old] == [q.rsplit("/", 1)[1] for q in new]
    for k in (2, 3):
        assert count(new[k], "f ") == 4 * count(old[k], "f ") == 4 * base.faces.shape[0] and count(new[k], "v ") == fine.verts.shape[0]
    assert count(new[2], "vn ") == fine.verts.shape[0]


def test_deftet_iso_surface_subdivide_keyword(ops):
    from deftet_amd.layers.DefTet.deftet import DefTet, clear_topology_cache
    from tests import marching_tets_cases as MK
    pos, tets, _e, _te = MK.grid(8, 1)
    B, V, T = 2, pos.shape[1], tets.shape[0]
    pos = np.repeat(pos, B, axis=0)
    cent = pos[:, tets].mean(2)
    occ = np.stack([np.clip(1.2 - np.linalg.norm(cent[b], axis=1) / (0.3 - 0.05 * b) * 0.7, 0.0, 1.0) for b in range(B)]).astype(np.float32)
    tets_b = torch.from_numpy(np.repeat(tets[None], B, axis=0)).to(DEV)
    layer = DefTet()
    p = torch.from_numpy(pos).to(DEV).requires_grad_(True)
    o = torch.from_numpy(occ[:, :, None]).to(DEV).requires_grad_(True)
    base = layer.iso_surface(p, tets_b, o, iso=0.5)
    zero = layer.iso_surface(p, tets_b, o, iso=0.5, subdivide=0)
    fine = layer.iso_surface(p, tets_b, o, iso=0.5, subdivide=1)
    for b in range(B):
        assert base.faces[b].shape[0] > 20 and base.faces[b].shape[0] != base.faces[1 - b].shape[0]
        assert torch.equal(base.verts[b], zero.verts[b]) and torch.equal(base.faces[b], zero.faces[b])
        assert fine.faces[b].shape[0] == 4 * base.faces[b].shape[0]
        v, f, _a = ops.loop_subdivide_mesh(base.verts[b], base.faces[b])
        assert torch.equal(fine.verts[b], v) and torch.equal(fine.faces[b], f)
    gp, go = torch.autograd.grad(sum(v.square().sum() for v in fine.verts), (p, o))
    assert gp.shape == (B, V, 3) and go.shape == (B, T, 1) and _finite_nonzero(gp, go)
    clear_topology_cache()
