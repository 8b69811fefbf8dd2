"""GPU tests of the tet-mesh argument contract of hip_ops ("A tet mesh as an argument"): the vertex-indexed operators
give the same bits through every way of handing over the mesh; every entry point that takes an incidence CSR refuses one that does
not fit, naming itself, before anything is launched; a TetTopology never has its CSR rebuilt.  Kuhn grids of 2 and 3 cells per
axis (V = 27, T = 48 and V = 64, T = 162: vertices of every incidence degree), B = 2, Q = 64 points in the unit cube, C = 3."""
import functools
import re

import numpy as np
import pytest
import torch

from deftet_amd import grids

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, Q, C = 2, 64, 3
OPS = ("tet_field_sample", "tet_field_gradient", "tet_field_energies", "tet_centroid_sample", "tet_to_vertex", "vertex_field_gradient")
FORMS = ("list", "csr", "topology", "per_shape")


def rand(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def mesh(R):
    """the shared inputs on the grid of R cells per axis (left unchanged by the tests): positions in the unit cube, the tet list
    and each form of it, a field, query points, per-tet values and one volume"""
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import TetTopology
    verts, tets = grids.kuhn_grid(2 * R)
    V, T = verts.shape[0], tets.shape[0]
    pos = torch.from_numpy(grids.jittered_positions(verts, 2 * R, B) + 0.5).to(DEV)
    tets = torch.from_numpy(tets).to(DEV)
    per_shape = tets[None].repeat(B, 1, 1)
    m = dict(V=V, T=T, pos=pos, tets=tets, per_shape=per_shape, csr=hip_ops.tet_vertex_csr(tets, V), per_shape_csr=hip_ops.tet_vertex_csr(per_shape, V),
             topology=TetTopology(tets, V), field=rand(1, B, V, C), pts=rand(2, B, Q, 3), values=rand(3, B, T, C), volume=rand(4, B, C, 4, 4, 4))
    assert m["csr"][2] == 1 and m["per_shape_csr"][2] == B and m["topology"].csr[2] == 1
    return m


def run(op, R, form):
    """[the output, the gradient on every differentiable input] of `op` with the mesh handed over as `form`"""
    from deftet_amd import hip_ops
    m = mesh(R)
    V, T, topo = m["V"], m["T"], m["topology"]
    leaf = lambda name: m[name].clone().requires_grad_(True)
    idx, kw = {"list": (m["tets"], {}), "csr": (m["tets"], dict(csr=m["csr"])), "topology": (topo.tet_idx, dict(topology=topo)),
               "per_shape": (m["per_shape"], dict(csr=m["per_shape_csr"]))}[form]
    method = form == "topology"                                               # a TetTopology through its own methods
    if op == "tet_field_sample":
        leaves = field, pos, pts = leaf("field"), leaf("pos"), leaf("pts")
        out = topo.field_sample(field, pos, pts) if method else hip_ops.tet_field_sample(field, pos, idx, pts, **kw)
    elif op == "tet_field_gradient":
        leaves = field, pos = leaf("field"), leaf("pos")
        g, vol = topo.field_gradient(field, pos, return_volume=True) if method else hip_ops.tet_field_gradient(field, pos, idx, return_volume=True, **kw)
        out = torch.cat([g.reshape(B, T, -1), vol[:, :, None]], 2)
    elif op == "tet_field_energies":
        leaves = field, pos = leaf("field"), leaf("pos")
        out = topo.field_energies(field, pos, target=0.5) if method else hip_ops.tet_field_energies(field, pos, idx, target=0.5, **kw)
    elif op == "tet_centroid_sample":                                         # K = T: every tet, in order
        leaves = pos, volume = leaf("pos"), leaf("volume")
        out = topo.centroid_sample([volume], pos) if method else hip_ops.tet_centroid_sample([volume], pos, idx, **kw)
    elif op == "tet_to_vertex":
        leaves = values, = leaf("values"),
        weights = rand(5, B, T)
        how = {"list": m["tets"], "csr": m["csr"], "topology": topo, "per_shape": m["per_shape_csr"]}[form]
        out = topo.to_vertices(values, weights=weights) if method else hip_ops.tet_to_vertex(values, how, V, weights=weights)
    else:
        leaves = field, pos = leaf("field"), leaf("pos")
        out = hip_ops.vertex_field_gradient(field, pos, idx, **kw)
    out.backward(rand(6, *out.shape))
    assert all(x.grad is not None for x in leaves)
    return [out.detach()] + [x.grad for x in leaves]


@pytest.mark.parametrize("R", (2, 3))
@pytest.mark.parametrize("op", OPS)
def test_same_bits_through_every_front_door(op, R):
    want = run(op, R, "list")
    assert all(torch.isfinite(w).all() for w in want) and all(bool(w.abs().max() > 0) for w in want)
    for form in FORMS[1:]:
        got = run(op, R, form)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(g, w), "%s, mesh as %s: tensor %d differs from the plain list's" % (op, form, k)


def csr_sites(m):
    """every entry point that takes an incidence CSR, as (caller it must name, call taking the CSR, whether it reads the index
    list beside the CSR)"""
    from deftet_amd import hip_ops
    V, T, pos, tets, field, pts, values = m["V"], m["T"], m["pos"], m["tets"], m["field"], m["pts"], m["values"]
    tet = pos[:, tets.long()]                                                 # [B,T,4,3] by torch: nothing of the library runs
    cond, bary = torch.zeros(B, Q, 1, device=DEV), rand(7, B, Q, 4)
    return [
        ("tet_gather_bwd", lambda c: hip_ops.tet_gather_bwd(tet, c, V), False),
        ("point_in_tet_bwd_to_vertices", lambda c: hip_ops.point_in_tet_bwd_to_vertices(tet, pts, cond, bary, c, V), False),
        ("point_in_tet_indexed_bwd_to_vertices", lambda c: hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, tets, pts, cond, bary, c), True),
        ("tet_centroid_sample_bwd_vertices", lambda c: hip_ops.tet_centroid_sample_bwd_vertices(rand(8, B, T, 3), c, V, T), False),
        ("tet_centroid_sample", lambda c: hip_ops.tet_centroid_sample([m["volume"]], pos, tets, csr=c), False),     # (its backward reads the CSR alone)
        ("tet_field_sample_bwd_field", lambda c: hip_ops.tet_field_sample_bwd_field(rand(9, B, Q, C), cond, bary, c, V, T), False),
        ("tet_field_sample", lambda c: hip_ops.tet_field_sample(field, pos, tets, pts, csr=c), True),
        ("tet_field_gradient_bwd", lambda c: hip_ops.tet_field_gradient_bwd(rand(10, B, T, C, 3), None, field, pos, tets, c), True),
        ("tet_field_gradient", lambda c: hip_ops.tet_field_gradient(field, pos, tets, csr=c), True),
        ("tet_field_energies", lambda c: hip_ops.tet_field_energies(field, pos, tets, csr=c), True),
        ("vertex_field_gradient", lambda c: hip_ops.vertex_field_gradient(field, pos, tets, csr=c), True),
        ("tet_to_vertex", lambda c: hip_ops.tet_to_vertex(values, c, V), False),
    ]


@pytest.mark.parametrize("R", (2, 3))
def test_csr_contract_at_every_site(R, monkeypatch):
    from deftet_amd import hip_ops
    m = mesh(R)
    V, T, tets = m["V"], m["T"], m["tets"]
    wrong = {"another T": hip_ops.tet_vertex_csr(tets[:-1], V), "another V": hip_ops.tet_vertex_csr(tets, V + 1),
             "idx_batch 3 with B = 2": hip_ops.tet_vertex_csr(tets[None].repeat(3, 1, 1), V),
             "int64": (m["csr"][0].long(), m["csr"][1].long(), 1), "on the host": (m["csr"][0].cpu(), m["csr"][1].cpu(), 1),
             "two elements": m["csr"][:2]}
    sites = csr_sites(m)
    monkeypatch.setattr(hip_ops._lib, "call", lambda *a, **k: pytest.fail("%s was launched" % a[0]))
    for caller, call, knows_list in sites:
        cases = dict(wrong)
        if knows_list:
            cases["idx_batch of another list"] = m["per_shape_csr"]           # B lists; the mesh was handed over as one shared list
        for what, csr in cases.items():
            with pytest.raises(RuntimeError, match=re.escape(caller + ":")):
                call(csr)
                pytest.fail("%s took a CSR built for %s" % (caller, what))
    monkeypatch.undo()
    for caller, call, _ in sites:                                             # and each takes the CSR that fits
        call(m["csr"])
    torch.cuda.synchronize()


def test_a_topology_never_rebuilds_its_csr(monkeypatch):
    from deftet_amd import hip_ops
    m = mesh(3)
    topo, V = m["topology"], m["V"]
    calls = []
    real = hip_ops.tet_vertex_csr
    monkeypatch.setattr(hip_ops, "tet_vertex_csr", lambda *a, **k: calls.append(1) or real(*a, **k))
    for op in OPS:
        run(op, 3, "topology")
        assert calls == [], "%s rebuilt the CSR of a TetTopology" % op
    for op in ("tet_field_gradient", "tet_field_energies", "vertex_field_gradient"):      # the slow path is still there, once a backward
        run(op, 3, "list")
        assert calls == [1], op
        calls.clear()
    run("tet_to_vertex", 3, "list")                                           # (in the call itself)
    assert calls == [1]
