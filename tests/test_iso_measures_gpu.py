"""GPU tests of the iso-solid measures on the tets (tet_iso_measure.hip) against the fp64 restatement of
tests/iso_measure_ref.py.  The kernel works in double from the fp32 inputs and rounds once, so every tolerance is derived:

    frac, area                  2^-24 |want| + 2^-40 S + 2^-149          (marching_tets_ref.entry_bound, S = the terms' absolute sum)
    totals, vertex gradients    the same with their own S
    vol                         the bits of hip_ops.tet_volumes.  That volume is formed in fp32 (tet_frame), so against fp64 it
                                carries the roundings of its six products, not one: 10 * 2^-24 S_vol — one rounding per edge
                                component (3), per product and difference of the cross product (3), per product and sum of the dot
                                product (3), one for the division by 6.  Both are asserted.

The fp32 predicates (field > iso, det > 0) are evaluated in fp32 by the restatement, so both sides agree on every tet's case.
"""
import functools

import numpy as np
import pytest
import torch

from tests import field_grad_ref as G
from tests import iso_measure_ref as ref
from tests import marching_tets_cases as cases
from tests import marching_tets_ref as R
from tests.tol import check_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def gpu(a, grad=False):
    return torch.from_numpy(np.array(a)).to(DEV).requires_grad_(grad)


def host(a):
    return a.detach().cpu().numpy()


def same_bits(a, b):
    a, b = (np.ascontiguousarray(host(x) if hasattr(x, "detach") else x, np.float32).view(np.uint32) for x in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def forward(field, pos, tets, iso, **kw):
    from deftet_amd import hip_ops
    return hip_ops.tet_iso_fraction(gpu(field), gpu(pos), gpu(tets), iso=iso, return_area=True, return_volume=True, **kw)


def check_forward(tag, field, pos, tets, iso):
    """frac, area, vol of the library against the restatement, each within its bound; -> (got, want)"""
    from deftet_amd import hip_ops
    frac, area, vol = forward(field, pos, tets, iso)
    p = ref.per_tet(field, pos, tets, iso)
    assert frac.dtype == torch.float32 and tuple(frac.shape) == p.frac.shape == tuple(area.shape) == tuple(vol.shape)
    check_bound(tag + ".frac", frac, p.frac, ref.bound(p.frac, p.S_frac))
    check_bound(tag + ".area", area, p.area, ref.bound(p.area, p.S_area))
    assert same_bits(host(vol)[p.live], host(hip_ops.tet_volumes(gpu(pos), gpu(tets)))[p.live])      # (a dead tet: 0, asserted below)
    check_bound(tag + ".vol", vol, p.vol, 10 * U * p.S_vol + 2.0 ** -149)
    dead = ~p.live
    assert all(np.all(host(x)[dead] == 0) for x in (frac, area, vol))
    return (host(frac), host(area), host(vol)), p


# ---------------------------------------------------------------------------- 1. thin crossings
@pytest.mark.parametrize("iso", cases.ISOS)
def test_thin_crossings(iso):
    pos, tets, edges, _te = cases.grid(8, 2)
    field = cases.thin_batch(pos.shape[1], iso, 100 + 10 * cases.ISOS.index(iso), 2)
    for f in field:
        cases.assert_thin(f, edges, iso)                                 # tau spans six decades
    (frac, area, _vol), p = check_forward("tim.thin@%g" % iso, field, pos, tets, iso)
    cut = (p.code != 0) & (p.code != 15)
    assert cut.sum() > 500 and (p.frac[cut] > 0).all() and frac[cut].min() < 1e-9 and (area[cut] > 0).all()


# ---------------------------------------------------------------------------- 2. corners on the level
@pytest.mark.parametrize("iso", cases.ISOS)
def test_corners_on_the_level(iso):
    pos, tets, _e, _te = cases.grid(8, 2)
    field = np.stack([cases.level(pos.shape[1], iso, 150 + b) for b in range(2)])
    (frac, _area, _vol), p = check_forward("tim.level@%g" % iso, field, pos, tets, iso)
    assert p.live.all() and (p.code == 0).sum() > 20 and (p.code == 15).sum() > 3
    assert np.all(frac[p.code == 0] == 0.0) and np.all(frac[p.code == 15] == 1.0)
    assert (frac >= 0).all() and (frac <= 1).all()


# ---------------------------------------------------------------------------- 3. the mesh of marching_tets on the GPU
def test_agreement_with_marching_tets_on_spheres20():
    """The mesh's vertices are fp32: each component is within forward64's bound vb = 6u (|x_lo| + |x_hi|) of its fp64 value, so a
    vertex moves by at most d = |vb|_2.  A triangle's area changes by at most half its perimeter times the largest move of its
    corners, the closed mesh's volume by at most its area times the largest move (each corner sweeps a third of each of its
    faces).  These margins are added to the kernel's own bound."""
    from deftet_amd import hip_ops
    pos, field = cases.spheres20()
    _p, tets, edges, _te = cases.grid(20, 1)
    T = len(tets)
    mesh = hip_ops.marching_tets(gpu(pos), gpu(field), hip_ops.TetEdges(gpu(tets), pos.shape[1]), iso=0.0, return_index=True)
    _frac, area, _vol = forward(field, pos, tets, 0.0)
    M = host(hip_ops.tet_iso_measures(gpu(field), gpu(pos), gpu(tets)))
    p = ref.per_tet(field, pos, tets, 0.0)
    want, S = ref.totals(field, pos, tets, 0.0)
    for b in range(2):
        v, f, tid = host(mesh.verts[b]).astype(np.float64), host(mesh.faces[b]), host(mesh.tet_id[b])
        assert all(R.closed_and_oriented(f, len(v))[:2])
        _t, (_v64, vb), _a = R.forward64(pos[b], field[b], edges, 0.0)
        move = np.sqrt((vb ** 2).sum(-1))                                # per vertex
        tri = v[f]
        perimeter = sum(np.sqrt(((tri[:, k] - tri[:, (k + 1) % 3]) ** 2).sum(-1)) for k in range(3))
        slack = np.bincount(tid, weights=0.5 * perimeter * move[f].max(1) * (1 + 1e-6), minlength=T)
        by_tet = ref.mesh_area_by_tet(v, f, tid, T)
        check_bound("tim.mesh.area_by_tet.%d" % b, host(area)[b], by_tet, ref.bound(by_tet, p.S_area[b]) + slack)
        check_bound("tim.mesh.area.%d" % b, M[b, 1], by_tet.sum(), ref.bound(by_tet.sum(), S[b, 1]) + slack.sum())
        vol = R.signed_volume(v, f)
        check_bound("tim.mesh.volume.%d" % b, M[b, 0], vol, ref.bound(vol, S[b, 0]) + by_tet.sum() * move.max() * (1 + 1e-6))
    check_bound("tim.mesh.totals", M, want, ref.bound(want, S))


# ---------------------------------------------------------------------------- 4. backward
@functools.lru_cache(maxsize=None)
def bwd_case(B, per_shape, T, kind):
    """(pos, tets [T,4] or [B,T,4], field [B,V], iso) on the res 8 grid: `thin` at the level 0.1, `sphere` at 0"""
    pos, tets = G.mesh(8, B, per_shape)
    tets = np.ascontiguousarray(tets[..., :T, :])
    V = pos.shape[1]
    if kind == "thin":
        return pos, tets, cases.thin_batch(V, 0.1, 300, B), 0.1
    return pos, tets, np.stack([cases.sphere(pos[b], 0.3 + 0.03 * b) for b in range(B)]), 0.0


def upstreams(B, T, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(B, T)).astype(np.float32) for _ in range(3)], rng.normal(size=(B, 5)).astype(np.float32), \
        rng.uniform(0, 1, (B, T)).astype(np.float32)


def fraction_backward(field, pos, tets, iso, g, **kw):
    from deftet_amd import hip_ops
    f, p = gpu(field, True), gpu(pos, True)
    out = hip_ops.tet_iso_fraction(f, p, gpu(tets), iso=iso, return_area=True, return_volume=True, **kw)
    sum((o * gpu(x)).sum() for o, x in zip(out, g)).backward()
    return f.grad, p.grad


def measures_backward(field, pos, tets, iso, go, w, **kw):
    from deftet_amd import hip_ops
    f, p = gpu(field, True), gpu(pos, True)
    m = hip_ops.tet_iso_measures(f, p, gpu(tets), iso=iso, weights=None if w is None else gpu(w), **kw)
    (m * gpu(go)).sum().backward()
    return m.detach(), f.grad, p.grad


def check_backward(tag, field, pos, tets, iso, seed=0, **kw):
    B, V = field.shape
    T = tets.shape[-2]
    g, go, w = upstreams(B, T, seed)
    gf, gp = fraction_backward(field, pos, tets, iso, g, **kw)
    (wf, wp), (Sf, Sp) = ref.fraction_grads(field, pos, tets, iso, *g)
    assert tuple(gf.shape) == (B, V) and tuple(gp.shape) == (B, V, 3) and gf.dtype == torch.float32
    check_bound(tag + ".fraction.grad_field", gf, wf, ref.bound(wf, Sf))
    check_bound(tag + ".fraction.grad_pos", gp, wp, ref.bound(wp, Sp))
    got = [gf, gp]
    for weights in (None, w):
        name = "%s.measures%s" % (tag, "" if weights is None else ".weighted")
        m, mf, mp = measures_backward(field, pos, tets, iso, go, weights, **kw)
        want, S = ref.totals(field, pos, tets, iso, weights)
        check_bound(name, m, want, ref.bound(want, S))
        (wf, wp), (Sf, Sp) = ref.measures_grads(field, pos, tets, iso, go, weights)
        check_bound(name + ".grad_field", mf, wf, ref.bound(wf, Sf))
        check_bound(name + ".grad_pos", mp, wp, ref.bound(wp, Sp))
        got += [m, mf, mp]
    return got


@pytest.mark.parametrize("kind", ["thin", "sphere"])
@pytest.mark.parametrize("B,per_shape,T", [(1, False, 384), (3, True, 321), (3, False, 321), (1, True, 63)])
def test_backward_against_the_fp64_gradients(B, per_shape, T, kind):
    pos, tets, field, iso = bwd_case(B, per_shape, T, kind)
    assert G.mesh(8, 1)[1].shape[0] == 384 and G.live_mask(pos, tets).all()
    if kind == "thin":
        cut = ref.per_tet(field, pos, tets, iso).area > 0
        assert cut.sum() > T / 4                                        # most tets are cut: every case, gaps over six decades
    check_backward("tim.bwd.%s.B%d.%d.T%d" % (kind, B, per_shape, T), field, pos, tets, iso)


def test_the_three_csr_routes_and_two_runs_give_the_same_bits():
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import TetTopology
    for B, per_shape in ((3, False), (3, True)):
        pos, tets, field, iso = bwd_case(B, per_shape, 321, "thin")
        V = pos.shape[1]
        topo = TetTopology(gpu(tets), V)
        routes = [dict(csr=hip_ops.tet_vertex_csr(gpu(tets), V)), dict(topology=topo), dict()]
        runs = [check_backward("tim.routes.%d.%d" % (per_shape, k), field, pos, tets, iso, **kw) for k, kw in enumerate(routes)]
        runs.append(check_backward("tim.routes.%d.again" % per_shape, field, pos, tets, iso, **routes[0]))
        for r in runs[1:]:
            assert all(same_bits(a, b) for a, b in zip(r, runs[0]))
        # the layer's routes and the raw halves
        f, p = gpu(field), gpu(pos)
        assert same_bits(topo.iso_fraction(f, p, iso=iso), hip_ops.tet_iso_fraction(f, p, gpu(tets), iso=iso))
        assert same_bits(topo.iso_measures(f, p, iso=iso), runs[0][2])
        g, _go, _w = upstreams(B, 321, 0)
        frac, area, vol = hip_ops.tet_iso_fraction_fwd(f[:, :, None], p, gpu(tets), iso, return_area=True, return_volume=True)
        assert same_bits(frac, topo.iso_fraction(f, p, iso=iso)) and area is not None and vol is not None
        gf, gp = hip_ops.tet_iso_fraction_bwd(gpu(g[0]), gpu(g[1]), gpu(g[2]), f, p, gpu(tets), routes[0]["csr"], iso)
        assert same_bits(gf, runs[0][0]) and same_bits(gp, runs[0][1])
        only_f, none = hip_ops.tet_iso_fraction_bwd(gpu(g[0]), None, None, f, p, gpu(tets), routes[0]["csr"], iso, want_pos=False)
        assert none is None and tuple(only_f.shape) == (B, V)


# ---------------------------------------------------------------------------- 5. special meshes
def test_a_vertex_with_more_incidences_than_a_wave():
    pos, tets = G.wedge_ring(130)
    counts = np.bincount(tets.reshape(-1))
    assert counts[0] == 130 and counts[1] == 130
    rng = np.random.default_rng(3)
    field = rng.normal(size=(1, pos.shape[1])).astype(np.float32)
    _got, p = check_forward("tim.ring", field, pos, tets, 0.0)
    assert len(set(ref.N_IN[p.code[0]].tolist())) >= 3
    check_backward("tim.ring", field, pos, tets, 0.0)


def test_dead_tets_give_zero_rows_and_take_part_in_nothing():
    from deftet_amd import hip_ops
    pos, tets, dead, lonely = G.dead_tet_mesh()
    dead = list(dead)
    field = G.normal_field((1, pos.shape[1]))
    (frac, area, vol), p = check_forward("tim.dead", field, pos, tets, 0.0)
    assert all(np.all(x[0, dead] == 0) for x in (frac, area, vol)) and not p.live[0, dead].any()
    got = check_backward("tim.dead", field, pos, tets, 0.0)
    for gfield, gpos in ((got[0], got[1]), (got[3], got[4]), (got[6], got[7])):
        assert np.all(host(gfield)[0, lonely] == 0) and np.all(host(gpos)[0, lonely] == 0)
    keep = np.delete(np.arange(len(tets)), dead)
    m = hip_ops.tet_iso_measures(gpu(field), gpu(pos), gpu(tets))
    assert same_bits(m, hip_ops.tet_iso_measures(gpu(field), gpu(pos), gpu(np.ascontiguousarray(tets[keep]))))
    live_volume = ref.per_tet(field, pos, tets[keep], 0.0).vol.sum()
    check_bound("tim.dead.live_volume", host(m)[0, 4], live_volume, ref.bound(live_volume, live_volume))


# ---------------------------------------------------------------------------- 6. non-finite values, one-sided fields
@pytest.mark.parametrize("iso", [0.0, 0.1])
def test_non_finite_corner_values(iso):
    pos, tets, _e, _te = cases.grid(20, 1)
    field, _bad_edge, _bad_vertex = cases.hostile(cases.banded(pos.shape[1], 170), 171, iso)
    field = field[None]
    (frac, area, vol), p = check_forward("tim.hostile@%g" % iso, field, pos, tets, iso)
    bad = ~np.isfinite(field[0][tets]).all(1)
    assert bad.sum() >= 6 * 20 and not p.live[0, bad].any() and p.live[0, ~bad].all()
    assert all(np.all(x[0, bad] == 0) and np.isfinite(x).all() for x in (frac, area, vol))
    got = check_backward("tim.hostile@%g" % iso, field, pos, tets, iso)
    assert all(np.isfinite(host(x)).all() for x in got)


def test_fields_all_inside_and_all_outside():
    """Nothing is cut: no area, the inside volume is the live volume or 0, and nothing reaches the field.  The positions keep
    the gradient of the volumes alone (a mesh that is all inside encloses its own volume); with no upstream on the volumes
    they get exactly 0."""
    pos, tets = G.mesh(8, 2)
    B, V = pos.shape[:2]
    T = len(tets)
    g, go, w = upstreams(B, T, 4)
    for value in (2.0, -1.0):
        field = np.full((B, V), value, np.float32)
        frac, area, _vol = check_forward("tim.flat%+g" % value, field, pos, tets, 0.0)[0]
        assert np.all(area == 0) and np.all(frac == (1.0 if value > 0 else 0.0))
        m, mf, mp = measures_backward(field, pos, tets, 0.0, go, w)
        mh = host(m)
        assert np.all(mh[:, 1] == 0) and np.all(mh[:, 0] == (mh[:, 4] if value > 0 else 0.0)) and np.all(host(mf) == 0)
        gf, gp = fraction_backward(field, pos, tets, 0.0, [g[0], g[1], np.zeros_like(g[2])])
        assert np.all(host(gf) == 0) and np.all(host(gp) == 0)
        area_only = np.zeros_like(go)
        area_only[:, 1] = go[:, 1]
        if value < 0:
            area_only[:, [0, 2]] = go[:, [0, 2]]                         # the inside volume and the intersection are 0 too
        m, mf, mp = measures_backward(field, pos, tets, 0.0, area_only, w)
        assert np.all(host(mf) == 0) and np.all(host(mp) == 0)
        check_backward("tim.flat%+g" % value, field, pos, tets, 0.0)


# ---------------------------------------------------------------------------- 7. IoU and the occupancy route
def test_iou_and_the_occupancy_route():
    """iso_iou forms I / (V + W - I) in fp32 from three fp32 totals: each total carries its bound (relative 2^-24 and the sum's
    2^-40), the union two roundings without cancellation worth speaking of (I <= min(V, W), so the union is at least (V + W) / 2
    and |V| + |W| + |I| <= 3 union), the quotient one: 16 * 2^-24 relative covers it with a factor two to spare."""
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet, clear_topology_cache
    pos, field = cases.spheres20()
    tets = cases.grid(20, 1)[1]
    B, T, V = 2, len(tets), pos.shape[1]
    clear_topology_cache()
    layer = DefTet()
    tets_b = gpu(np.broadcast_to(tets[None], (B, T, 4)))
    occ = layer.field_occupancy(gpu(pos), tets_b, gpu(field))
    assert tuple(occ.shape) == (B, T) and float(occ.min()) >= 0 and float(occ.max()) <= 1
    assert same_bits(occ, hip_ops.tet_iso_fraction(gpu(field), gpu(pos), gpu(tets)))
    hard = (occ > 0.5).float()
    for name, gt in (("half", hard), ("ones", torch.ones_like(hard))):
        iou = layer.field_iou(gpu(pos), tets_b, gpu(field), gt)
        M, _S = ref.totals(field, pos, tets, 0.0, host(gt))
        want = M[:, 2] / (M[:, 0] + M[:, 3] - M[:, 2])
        assert tuple(iou.shape) == (B,) and (want > 0.01).all() and (want < 1).all()
        check_bound("tim.iou." + name, iou, want, 16 * U * want)
    m = layer.field_measures(gpu(pos), tets_b, gpu(field), gt_occ_bxt=hard[:, :, None])
    assert same_bits(m, hip_ops.tet_iso_measures(gpu(field), gpu(pos), gpu(tets), weights=hard))
    assert np.all(host(hip_ops.iso_iou(torch.zeros(2, 5, device=DEV))) == 0)
    # thresholded, the occupancy is a solid like any predicted one: its surface is closed
    nbr = hip_ops.tet_face_neighbours(tets, V, torch.device(DEV))
    soup = hip_ops.surface_extract(hip_ops.tet_gather(gpu(pos), gpu(tets)), hard, nbr, "binary", tet_idx=gpu(tets), return_faces=True)
    for b in range(B):
        faces = host(soup.faces[b])
        assert len(faces) > 200 and R.closed_and_oriented(faces, V)[0]
    # a gradient through the IoU reaches the field and the positions
    f, p = gpu(field, True), gpu(pos, True)
    layer.field_iou(p, tets_b, f, hard).sum().backward()
    assert float(f.grad.abs().max()) > 0 and float(p.grad.abs().max()) > 0 and np.isfinite(host(f.grad)).all()
    clear_topology_cache()


# ---------------------------------------------------------------------------- 8. arguments
def test_bad_arguments_are_refused_before_any_c_entry(monkeypatch):
    from deftet_amd import hip_ops
    pos, tets = G.mesh(4, 3)
    B, V, T = 3, pos.shape[1], len(tets)
    f, p, t = gpu(G.normal_field((B, V))), gpu(pos), gpu(tets)
    csr = hip_ops.tet_vertex_csr(t, V)
    other = hip_ops.tet_vertex_csr(gpu(np.ascontiguousarray(tets[:40])), V)      # the CSR of another mesh (40 of the 48 tets)
    w = gpu(np.ones((B, T), np.float32))

    def reached(name, *_a, **_k):
        raise AssertionError("%s was reached" % name)
    monkeypatch.setattr(hip_ops._lib, "call", reached)
    for fn in (hip_ops.tet_iso_fraction, hip_ops.tet_iso_measures):
        for iso in (float("nan"), float("inf"), -float("inf"), 1e39):
            with pytest.raises(hip_ops._lib.DefTetHipError, match="DEFTET_EINVAL"):
                fn(f, p, t, iso=iso)
        for args in ((f[:, :, None].expand(B, V, 2), p, t), (f[0], p, t), (f[:2], p, t), (f, p[:, :, :2], t), (f, p, t[:, :3]),
                     (f, p, t.float()), (f.double(), p, t), (f, p.double(), t), (f.cpu(), p, t), (f, p.cpu(), t), (f, p, t.cpu())):
            with pytest.raises(RuntimeError):
                fn(*args)
        for bad in (other, csr[:2], (csr[0].cpu(), csr[1].cpu(), csr[2])):
            with pytest.raises(RuntimeError):
                fn(f, p, t, csr=bad)
    for bad in (w[:, :-1], w[0], w.double(), w.cpu()):
        with pytest.raises(RuntimeError):
            hip_ops.tet_iso_measures(f, p, t, weights=bad)
    with pytest.raises(RuntimeError):
        hip_ops.tet_iso_fraction_bwd(w[:, :-1], None, None, f, p, t, csr)
    with pytest.raises(RuntimeError):
        hip_ops.tet_iso_fraction_bwd(w, None, None, f, p, t, other)
