"""GPU tests of the field gradients on the tets (tet_field_grad.hip): tet_field_gradient and tet_field_energies,
forward and backward, within the standing 1e-5 max-norm bound of the fp64 chain of tests/field_grad_ref.py; tet_to_vertex bit for
bit against its fp32 restatement; the same bits on a second run; a vertex of 130 incidences; dead tets; a constant field; the
module routes (DefTet.iso_surface, marching_tets_normals, the OBJ export with normals) and the argument errors."""
import functools

import numpy as np
import pytest
import torch

from tests import field_grad_ref as ref
from tests.tol import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5
MESHES = ["R4", "R6", "T1", "T63", "T64", "T65"]                      # whole grids (T = 48, 162); the first T tets of the R = 6 grid, all 64 vertices kept


def bits(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def host(a):
    return a.detach().cpu().numpy()


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def case(name, B, per_shape):
    """(pos f32 [B,V,3], tets int64 [T,4] or [B,T,4])"""
    pos, tets = ref.mesh(4 if name == "R4" else 6, B, per_shape)
    if name[0] == "T":
        tets = tets[..., : int(name[1:]), :]
    return pos, np.ascontiguousarray(tets)


@functools.lru_cache(maxsize=None)
def csr_of(name, B, per_shape):
    from deftet_amd import hip_ops
    pos, tets = case(name, B, per_shape)
    return hip_ops.tet_vertex_csr(gpu(tets), pos.shape[1])


def grid_params(channels):
    return [pytest.mark.parametrize("per_shape", [False, True], ids=["shared", "per_shape"]), pytest.mark.parametrize("C", channels),
            pytest.mark.parametrize("B", [1, 3]), pytest.mark.parametrize("name", MESHES)]


def over(channels):
    def deco(fn):
        for p in grid_params(channels):
            fn = p(fn)
        return fn
    return deco


# ---------------------------------------------------------------------------- (a) tet_field_gradient
def gradient_run(pos, tets, field, gout, gvol, csr):
    from deftet_amd import hip_ops
    f, p = gpu(field, True), gpu(pos, True)
    g, vol = hip_ops.tet_field_gradient(f, p, gpu(tets), csr=csr, return_volume=True)
    ((g * gpu(gout)).sum() + (vol * gpu(gvol)).sum()).backward()
    return g.detach(), vol.detach(), f.grad, p.grad


def gradient_want(pos, tets, field, gout, gvol):
    f, p = t64(field, True), t64(pos, True)
    g, vol = ref.chain64(f, p, tets, ref.live_mask(pos, tets))
    ((g * t64(gout)).sum() + (vol * t64(gvol)).sum()).backward()
    return g.detach(), vol.detach(), f.grad, p.grad


def check_gradient(tag, pos, tets, C, csr="build"):
    from deftet_amd import hip_ops
    B, V = pos.shape[:2]
    T = tets.shape[-2]
    field, gout, gvol = ref.normal_field((B, V, C)), ref.normal_field((B, T, C, 3))[::-1].copy(), ref.normal_field((B, T))
    if csr == "build":
        csr = hip_ops.tet_vertex_csr(gpu(tets), V)
    got = gradient_run(pos, tets, field, gout, gvol, csr)
    want = gradient_want(pos, tets, field, gout, gvol)
    for what, a, b in zip(("grad", "vol", "grad_field", "grad_pos"), got, want):
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == torch.float32
        check_close("tfg.%s.%s" % (tag, what), a, b, BOUND)
    again = gradient_run(pos, tets, field, gout, gvol, csr)
    assert all(same_bits(a, b) for a, b in zip(got, again))
    return got


@over([1, 3, 4, 5, 33])
def test_gradient_forward_and_backward_against_the_fp64_chain(name, B, C, per_shape):
    pos, tets = case(name, B, per_shape)
    assert ref.live_mask(pos, tets).all()
    g, vol, gf, gp = check_gradient("%s.B%d.C%d.%d" % (name, B, C, per_shape), pos, tets, C, csr_of(name, B, per_shape))
    if name[0] == "T":                                               # a vertex without an incidence gets an exact zero
        used = np.zeros(pos.shape[:2], bool)
        tt = ref.tets_of(tets, B)
        for b in range(B):
            used[b, tt[b].reshape(-1)] = True
        assert not used.all() and np.all(host(gf)[~used] == 0) and np.all(host(gp)[~used] == 0)


def test_gradient_raw_halves_without_volume_and_the_slow_path():
    from deftet_amd import hip_ops
    pos, tets = case("R4", 3, False)
    B, V, T, C = 3, pos.shape[1], tets.shape[0], 4
    field, gout = ref.normal_field((B, V, C)), ref.normal_field((B, T, C, 3))
    csr = csr_of("R4", 3, False)
    g = hip_ops.tet_field_gradient_fwd(gpu(field), gpu(pos), gpu(tets))
    g2, vol = hip_ops.tet_field_gradient_fwd(gpu(field), gpu(pos), gpu(tets.astype(np.int32)), return_volume=True)
    assert same_bits(g, g2) and same_bits(vol, hip_ops.tet_volumes(gpu(pos), gpu(tets)))
    check_close("tfg.raw.vol", vol, ref.gradient(field, pos, tets)[1], BOUND)
    gf, gp = hip_ops.tet_field_gradient_bwd(gpu(gout), None, gpu(field), gpu(pos), gpu(tets), csr)
    only_f, none = hip_ops.tet_field_gradient_bwd(gpu(gout), None, gpu(field), gpu(pos), gpu(tets), csr, want_pos=False)
    assert none is None and same_bits(only_f, gf)
    # csr=None: the slow path gives the same bits; a gradient through the volumes alone
    f, p = gpu(field, True), gpu(pos, True)
    hip_ops.tet_field_gradient(f, p, gpu(tets)).mul(gpu(gout)).sum().backward()
    assert same_bits(f.grad, gf) and same_bits(p.grad, gp)
    p = gpu(pos, True)
    hip_ops.tet_field_gradient(gpu(field), p, gpu(tets), csr=csr, return_volume=True)[1].sum().backward()
    p64 = t64(pos, True)
    ref.chain64(t64(field), p64, tets, ref.live_mask(pos, tets))[1].sum().backward()
    check_close("tfg.raw.grad_pos_of_vol", p.grad, p64.grad, BOUND)                   # (the total volume is fixed: interior rows are ~0)


# ---------------------------------------------------------------------------- (b) tet_field_energies
def energies_run(pos, tets, field, gout, csr, target):
    from deftet_amd import hip_ops
    f, p = gpu(field, True), gpu(pos, True)
    e = hip_ops.tet_field_energies(f, p, gpu(tets), csr=csr, target=target)
    (e * gpu(gout)).sum().backward()
    return e.detach(), f.grad, p.grad


def check_energies(tag, pos, tets, C, csr="build", target=0.75, field=None):
    from deftet_amd import hip_ops
    B, V = pos.shape[:2]
    field = ref.normal_field((B, V, C)) if field is None else field
    gout = ref.normal_field((B, C, 2)) + 2.0
    if csr == "build":
        csr = hip_ops.tet_vertex_csr(gpu(tets), V)
    got = energies_run(pos, tets, field, gout, csr, target)
    f, p = t64(field, True), t64(pos, True)
    e = ref.energies64(f, p, tets, ref.live_mask(pos, tets), target)
    (e * t64(gout)).sum().backward()
    for what, a, b in zip(("energies", "grad_field", "grad_pos"), got, (e.detach(), f.grad, p.grad)):
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == torch.float32
        check_close("tfe.%s.%s" % (tag, what), a, b, BOUND)
    again = energies_run(pos, tets, field, gout, csr, target)
    assert all(same_bits(a, b) for a, b in zip(got, again))
    return got


@over([1, 3, 8])
def test_energies_and_their_backward_against_the_fp64_chain(name, B, C, per_shape):
    pos, tets = case(name, B, per_shape)
    check_energies("%s.B%d.C%d.%d" % (name, B, C, per_shape), pos, tets, C, csr_of(name, B, per_shape))


def test_energies_of_a_linear_field():
    from deftet_amd import hip_ops
    pos, tets = case("R6", 3, False)
    a = np.array([[0.6, -0.8, 0.0], [1.0, 2.0, -2.0]])
    field = (pos.astype(np.float64) @ a.T + np.array([0.25, -0.5])).astype(np.float32)
    g = hip_ops.tet_field_gradient(gpu(field), gpu(pos), gpu(tets))
    check_close("tfg.linear", g, np.broadcast_to(a, g.shape), BOUND)
    for target, want in ((1.0, [[1.0, 0.0], [9.0, 4.0]]), (3.0, [[1.0, 4.0], [9.0, 0.0]])):
        e = host(hip_ops.tet_field_energies(gpu(field), gpu(pos), gpu(tets), target=target))
        assert np.abs(e - np.array(want)[None]).max() < 9e-5, e


# ---------------------------------------------------------------------------- (c) tet_to_vertex
def to_vertex_run(values, on, V, weights, gout, fill):
    from deftet_amd import hip_ops
    x = gpu(values, True)
    out = hip_ops.tet_to_vertex(x, on, V, weights=None if weights is None else gpu(weights), fill=fill)
    out.backward(gpu(gout))
    return out.detach(), x.grad


def check_to_vertex(pos, tets, C, on, weighted):
    B, V = pos.shape[:2]
    T = tets.shape[-2]
    values, gout = ref.normal_field((B, T, C)), ref.normal_field((B, V, C))[:, ::-1].copy()
    weights = ref.gradient(np.zeros((B, V, 1), np.float32), pos, tets)[1] if weighted else None      # the volumes
    got = to_vertex_run(values, on, V, weights, gout, -2.5)
    want, wsum = ref.tet_to_vertex(values, tets, V, weights, fill=-2.5)
    assert same_bits(got[0], want) and same_bits(got[1], ref.tet_to_vertex_bwd(gout, wsum, tets, weights))
    again = to_vertex_run(values, on, V, weights, gout, -2.5)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1])
    return got, wsum


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "volumes"])
@over([1, 3, 4, 5, 33])
def test_to_vertex_bit_identical_to_the_fp32_restatement(name, B, C, per_shape, weighted):
    pos, tets = case(name, B, per_shape)
    (out, _), wsum = check_to_vertex(pos, tets, C, csr_of(name, B, per_shape), weighted)
    if name[0] == "T":
        assert (wsum == 0).any() and np.all(host(out)[wsum == 0] == -2.5)


def test_to_vertex_from_a_tet_list_a_csr_and_a_topology():
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import TetTopology
    pos, tets = case("R6", 3, False)
    B, V, T, C = 3, pos.shape[1], tets.shape[0], 3
    values, gout = ref.normal_field((B, T, C)), ref.normal_field((B, V, C))
    topo = TetTopology(gpu(tets), V)
    runs = [to_vertex_run(values, on, V, None, gout, 0.0) for on in (gpu(tets), gpu(tets.astype(np.int32)), topo.csr, topo)]
    for r in runs[1:]:
        assert same_bits(r[0], runs[0][0]) and same_bits(r[1], runs[0][1])
    x = gpu(values, True)
    topo.to_vertices(x).backward(gpu(gout))
    assert same_bits(x.grad, runs[0][1])
    w = gpu(np.abs(ref.normal_field((B, T))), True)                   # the weights are a constant: no gradient reaches them
    out = hip_ops.tet_to_vertex(gpu(values, True), topo, V, weights=w)
    out.sum().backward()
    assert w.grad is None


# ---------------------------------------------------------------------------- a vertex of 130 incidences
def test_high_valence_hub_and_apex():
    pos, tets = ref.wedge_ring(130)
    counts = np.bincount(tets.reshape(-1))
    assert counts[0] == 130 and counts[1] == 130 and counts[2:].max() == 2
    check_gradient("ring", pos, tets, 3)
    check_energies("ring", pos, tets, 3)
    from deftet_amd import hip_ops
    for weighted in (False, True):
        check_to_vertex(pos, tets, 3, hip_ops.tet_vertex_csr(gpu(tets), pos.shape[1]), weighted)


# ---------------------------------------------------------------------------- dead tets
def test_dead_tets_give_zero_rows_and_take_part_in_nothing():
    from deftet_amd import hip_ops
    pos, tets, dead, lonely = ref.dead_tet_mesh()
    dead = list(dead)
    V, T, C = pos.shape[1], tets.shape[0], 3
    g, vol, gf, gp = check_gradient("dead", pos, tets, C)
    assert np.all(host(g)[0, dead] == 0) and np.all(host(vol)[0, dead] == 0)
    assert np.isfinite(host(gf)).all() and np.isfinite(host(gp)).all() and np.all(host(gf)[0, lonely] == 0) and np.all(host(gp)[0, lonely] == 0)
    e, ef, ep = check_energies("dead", pos, tets, C)
    keep = np.delete(np.arange(T), dead)
    field = ref.normal_field((1, V, C))
    e_live = hip_ops.tet_field_energies(gpu(field), gpu(pos), gpu(tets[keep]), target=0.75)
    check_close("tfe.dead.unchanged", e, e_live, 1e-6)
    assert np.isfinite(host(ef)).all() and np.isfinite(host(ep)).all() and np.all(host(ef)[0, lonely] == 0)
    vg = hip_ops.vertex_field_gradient(gpu(field), gpu(pos), gpu(tets), fill=7.0)
    assert tuple(vg.shape) == (1, V, C, 3) and np.all(host(vg)[0, lonely] == 7.0) and np.all(host(vg)[0, V - 1] == 7.0)
    want, _ = ref.tet_to_vertex(host(g).reshape(1, T, C * 3), tets, V, host(vol), fill=7.0)
    assert same_bits(vg.reshape(1, V, C * 3), want)
    # a NaN position kills the tets around it and nothing else
    bad = pos.copy()
    bad[0, tets[0, 0]] = np.nan
    touched = (tets == tets[0, 0]).any(1)
    g2, vol2 = hip_ops.tet_field_gradient(gpu(field), gpu(bad), gpu(tets), return_volume=True)
    assert np.all(host(g2)[0, touched] == 0) and np.all(host(vol2)[0, touched] == 0) and same_bits(host(g2)[0, ~touched], host(g)[0, ~touched])
    assert np.isfinite(host(hip_ops.tet_field_energies(gpu(field), gpu(bad), gpu(tets)))).all()
    # no live tet at all: zero energies and zero gradients
    f, p = gpu(field, True), gpu(pos, True)
    e0 = hip_ops.tet_field_energies(f, p, gpu(tets[dead]))
    e0.sum().backward()
    assert np.all(host(e0) == 0) and np.all(host(f.grad) == 0) and np.all(host(p.grad) == 0)


# ---------------------------------------------------------------------------- a constant field
def test_constant_field_sits_on_the_eikonal_kink():
    from deftet_amd import hip_ops
    pos, tets = case("R6", 3, True)
    V, C, target = pos.shape[1], 3, 0.75
    field = np.broadcast_to(np.array([0.5, -2.0, 0.0], np.float32), (3, V, C)).copy()
    f, p = gpu(field, True), gpu(pos, True)
    csr = csr_of("R6", 3, True)
    g = hip_ops.tet_field_gradient(f, p, gpu(tets), csr=csr)
    assert np.all(host(g) == 0)
    e = hip_ops.tet_field_energies(f, p, gpu(tets), csr=csr, target=target)
    assert np.all(host(e)[:, :, 0] == 0) and np.abs(host(e)[:, :, 1] - target ** 2).max() <= 1e-6 * target ** 2
    (e * gpu(ref.normal_field((3, C, 2)) + 2.0)).sum().backward()
    assert np.isfinite(host(f.grad)).all() and np.isfinite(host(p.grad)).all() and np.all(host(f.grad) == 0)
    assert np.abs(host(p.grad)).max() < 1e-5


# ---------------------------------------------------------------------------- routes
class StubModel:
    """the attributes and methods the marching-tetrahedra routes read of a render model"""

    def __init__(self, points, tets):
        self.tfpoint_px3 = torch.from_numpy(points.copy()).to(DEV)
        self.tfpointmov_px3 = torch.zeros_like(self.tfpoint_px3).requires_grad_(True)
        self.tfpointfeat_pxd = torch.from_numpy(ref.normal_field((points.shape[0], 4))).to(DEV).requires_grad_(True)
        self.tftet_tx4 = torch.from_numpy(tets.copy()).to(DEV)

    def get_point(self, with_coef=False):
        return self.tfpoint_px3 + self.tfpointmov_px3

    def get_feat(self):
        return self.tfpointfeat_pxd


def closed(faces):
    f = host(faces).astype(np.int64)
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return bool((np.unique(d, axis=0, return_counts=True)[1] == 2).all())


def test_iso_surface_of_a_per_tet_occupancy():
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet, TetTopology, clear_topology_cache
    pos, tets = case("R6", 3, False)
    B, V, T = 3, pos.shape[1], tets.shape[0]
    cent = pos[:, tets].mean(2)                                       # [B,T,3]
    occ = (np.sqrt((cent ** 2).sum(-1)) < 0.3).astype(np.float32)
    assert 4 < occ[0].sum() < T / 2
    clear_topology_cache()
    layer = DefTet()
    tets_b = gpu(np.broadcast_to(tets[None], (B, T, 4)))
    # 18 tets lie inside: the vertex means reach about 0.5 at the two central vertices, 0.28 at the most elsewhere and stay below
    # 0.2 on the grid's boundary, so the level 0.3 is a closed surface about the centre (at 0.5 nothing lies strictly above)
    for weighted, iso in ((True, 0.3), (False, 0.3)):
        o, p = gpu(occ[:, :, None], True), gpu(pos, True)
        mesh = layer.iso_surface(p, tets_b, o, iso=iso, volume_weighted=weighted)
        topo = TetTopology(gpu(tets), V)
        field = topo.to_vertices(gpu(occ[:, :, None]), weights=hip_ops.tet_volumes(gpu(pos), gpu(tets)) if weighted else None)
        want = hip_ops.marching_tets(gpu(pos), field.squeeze(-1), topo.edges(), iso=iso)
        for b in range(B):
            assert mesh.faces[b].shape[0] > 20 and torch.equal(mesh.verts[b], want.verts[b]) and torch.equal(mesh.faces[b], want.faces[b])
            assert closed(mesh.faces[b])
        sum(v.square().sum() for v in mesh.verts).backward()
        assert o.grad.shape == (B, T, 1) and float(o.grad.abs().max()) > 0 and float(p.grad.abs().max()) > 0
        assert np.isfinite(host(o.grad)).all() and np.isfinite(host(p.grad)).all()
    reg = layer.field_regularizers(gpu(pos), tets_b, gpu(ref.normal_field((B, V, 2))), target=0.75)
    assert same_bits(reg, hip_ops.tet_field_energies(gpu(ref.normal_field((B, V, 2))), gpu(pos), gpu(tets), target=0.75))
    f = gpu(ref.normal_field((B, V, 2)))
    assert same_bits(topo.field_energies(f, gpu(pos), target=0.75), reg)
    assert same_bits(topo.field_gradient(f, gpu(pos)), hip_ops.tet_field_gradient(f, gpu(pos), gpu(tets)))
    clear_topology_cache()


def linear_process(a, b):
    def processfunc(points, feat):
        w = points @ torch.tensor(a, dtype=torch.float32, device=points.device)[:, None] + b
        return w, torch.sigmoid(feat[:, 1:4])
    return processfunc


def sphere_process(points, feat):
    return torch.sigmoid((0.3 - points.norm(dim=1, keepdim=True)) * 20 + 0.1 * feat[:, :1]), torch.sigmoid(feat[:, 1:4])


def test_marching_tets_normals():
    from deftet_amd.render import iso_surface
    pos, tets = ref.mesh(8, 1)
    model = StubModel(pos[0], tets)
    mesh = iso_surface.marching_tets_normals(model, 0.25, sphere_process)
    plain = iso_surface.marching_tets(model, 0.25, sphere_process)
    assert mesh.verts.shape[0] > 20 and torch.equal(mesh.verts, plain.verts) and torch.equal(mesh.faces, plain.faces)
    n = host(mesh.vert_attr)
    assert n.shape == (mesh.verts.shape[0], 3) and np.abs(np.sqrt((n.astype(np.float64) ** 2).sum(1)) - 1).max() <= 1e-5
    assert (n * host(mesh.verts)).sum(1).min() > 0                    # a sphere about the origin: outward is away from it
    gm, gf = torch.autograd.grad(mesh.vert_attr[:, 0].sum(), (model.tfpointmov_px3, model.tfpointfeat_pxd))
    assert float(gm.abs().max()) > 0 and float(gf[:, 0].abs().max()) > 0
    kept = model._deftet_tet_csr
    iso_surface.marching_tets_normals(model, 0.25, sphere_process)
    assert model._deftet_tet_csr is kept
    # a linear field: the normal is -a / |a| at every vertex
    a = [0.36, -0.48, 0.8]
    flat = iso_surface.marching_tets_normals(model, 0.05, linear_process(a, 0.05))
    assert flat.verts.shape[0] > 20
    check_close("normals.linear", flat.vert_attr, np.broadcast_to(-np.array(a), tuple(flat.vert_attr.shape)), BOUND)
    # a zero gradient gives a zero normal
    from deftet_amd import hip_ops
    z = hip_ops.unit_normals(torch.tensor([[0.0, 0.0, 0.0], [0.0, -2.0, 0.0]], device=DEV))
    assert host(z).tolist() == [[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]]


def test_obj_export_with_normals(tmp_path):
    from deftet_amd import hip_ops
    from deftet_amd.render import export, iso_surface
    pos, tets = ref.mesh(8, 1)
    V = pos.shape[1]
    model = StubModel(pos[0], tets)
    w, col = sphere_process(model.get_point(True), model.get_feat())
    nbr = hip_ops.tet_face_neighbours(tets, V, torch.device(DEV))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = export.save_surface_objs(model.get_point(True), (w, col), tets, nbr, str(tmp_path / "a"), "s", thresholds=(0.25,), iso=0.25)
    withn = export.save_surface_objs(model.get_point(True), (w, col), tets, nbr, str(tmp_path / "b"), "s", thresholds=(0.25,), iso=0.25,
                                     normals=True)
    assert [p.rsplit("/", 1)[1] for p in plain] == [p.rsplit("/", 1)[1] for p in withn] and len(plain) == 4
    read = lambda p: open(p, "rb").read()
    for k in (0, 1, 3):
        assert read(plain[k]) == read(withn[k])
    # without the flag: the bytes of the writer as it was
    mesh = iso_surface.marching_tets(model, 0.25, sphere_process)
    f = mesh.faces
    assert read(plain[2]) == export.mesh_obj_text(mesh.verts.detach(), f[:, [0, 2, 1]]).encode()
    lines = read(withn[2]).decode().splitlines()
    v = [x for x in lines if x.startswith("v ")]
    vn = [x for x in lines if x.startswith("vn ")]
    fl = [x for x in lines if x.startswith("f ")]
    assert len(v) == mesh.verts.shape[0] and len(vn) == len(v) and len(fl) == f.shape[0] and len(lines) == 2 * len(v) + len(fl)
    assert lines[: len(v)] == read(plain[2]).decode().splitlines()[: len(v)]
    want_n = host(iso_surface.marching_tets_normals(model, 0.25, sphere_process).vert_attr).astype(np.float64)
    assert vn == [("vn %f %f %f" % tuple(r)) for r in want_n]
    fh = host(f) + 1
    assert fl == ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in fh.tolist()]


# ---------------------------------------------------------------------------- argument errors
def test_argument_errors():
    from deftet_amd import hip_ops
    pos, tets = case("R4", 3, False)
    B, V, T = 3, pos.shape[1], tets.shape[0]
    f, p, t = gpu(ref.normal_field((B, V, 2))), gpu(pos), gpu(tets)
    csr = csr_of("R4", 3, False)
    other = csr_of("T63", 3, False)                                   # the CSR of another tet list
    Err = RuntimeError
    for fn in (hip_ops.tet_field_gradient, hip_ops.tet_field_energies, hip_ops.vertex_field_gradient):
        for args in ((f[0], p, t), (f, p[0], t), (f, p[:, :, :2], t), (f, p, t.reshape(-1)), (f, p, t[:, :3]), (f[:2], p, t),
                     (f, p, t.float()), (f.double(), p, t), (f.cpu(), p, t), (f, p.cpu(), t), (f, p, t.cpu())):
            with pytest.raises(Err):
                fn(*args)
        with pytest.raises(Err):
            fn(f, p, t, csr=other)
        with pytest.raises(Err):
            fn(f, p, t, csr=csr[:2])
    for C in (9, 33):                                                 # the energies take 1..8 channels
        with pytest.raises(hip_ops._lib.DefTetHipError, match="DEFTET_EINVAL"):
            hip_ops.tet_field_energies(gpu(ref.normal_field((B, V, C))), p, t)
    with pytest.raises(Err):
        hip_ops.tet_field_energies(f[:, :, :0], p, t)
    x = gpu(ref.normal_field((B, T, 2)))
    for args, kw in (((x[0], csr, V), {}), ((x, other, V), {}), ((x, csr, V + 1), {}), ((x[:, :-1], csr, V), {}), ((x, t[:, :3], V), {}),
                     ((x, t.float(), V), {}), ((x.cpu(), csr, V), {}), ((x, csr, V), dict(weights=x[:, :, 0].cpu())),
                     ((x, csr, V), dict(weights=x[:, :-1, 0])), ((x, csr, V), dict(weights=x)), ((x.double(), csr, V), {})):
        with pytest.raises(Err):
            hip_ops.tet_to_vertex(*args, **kw)
    with pytest.raises(Err):
        hip_ops.tet_field_gradient_bwd(gpu(ref.normal_field((B, T, 2, 2))), None, f, p, t, csr)
    with pytest.raises(Err):
        hip_ops.tet_field_gradient_bwd(gpu(ref.normal_field((B, T, 2, 3))), gpu(ref.normal_field((B, T + 1))), f, p, t, csr)
