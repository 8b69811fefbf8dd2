"""Marching tetrahedra on the GPU against the numpy restatement (tests/marching_tets_ref.py): every output of every shape bit
for bit; the gradients against float64 autograd within the project's bound (tests/tol.py, maxnorm 1e-5), bit-identical between
two runs and exactly zero away from the surface; then, with no condition on the crossing gaps, the forward and every gradient
entry against float64 within bounds derived from the arithmetic (thin crossings, nonzero iso, every attribute width), and the
containment of NaN and infinite field values; the model path and the OBJ export."""
import numpy as np
import pytest
import torch

from tests import marching_tets_cases as K
from tests import marching_tets_ref as R
from tests.tol import check_bound, check_close

pytestmark = pytest.mark.gpu
MAXNORM = 1e-5


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def topology(cuda, tets, n_vertex, edges, tet_edge):
    from deftet_amd import hip_ops
    top = hip_ops.TetEdges(torch.from_numpy(np.array(tets)).to(cuda), n_vertex)
    assert top.edges.dtype == torch.int32 and same(top.edges.cpu().numpy().astype(np.int64), edges)
    assert top.tet_edge.dtype == torch.int32 and same(top.tet_edge.cpu().numpy().astype(np.int64), tet_edge)
    off, slots = R.edge_vertex_csr(edges, n_vertex)
    assert same(top.offsets.cpu().numpy(), off) and same(top.slots.cpu().numpy(), slots)
    assert (top.n_vertex, top.n_tet, top.n_edge) == (n_vertex, tets.shape[0], edges.shape[0])
    return top


def run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, iso, attr=None):
    """every output of hip_ops.marching_tets for the batch against the restatement, shape by shape; returns (got, [want])"""
    from deftet_amd import hip_ops
    dev = lambda x: None if x is None else torch.from_numpy(np.array(x)).to(cuda)
    got = hip_ops.marching_tets(dev(pos), dev(field), top, iso=iso, attr=dev(attr), return_index=True)
    wants = []
    for b in range(pos.shape[0]):
        w = R.marching_tets(pos[b], field[b], tets, iso, attr=None if attr is None else attr[b], edges=edges, tet_edge=tet_edge)
        wants.append(w)
        for name in ("verts", "faces", "edge_id", "t", "tet_id"):
            assert same(getattr(got, name)[b].cpu().numpy(), getattr(w, name)), (b, name)
        assert got.faces[b].dtype == torch.int64 and got.edge_id[b].dtype == torch.int64 and got.tet_id[b].dtype == torch.int64
        if attr is None:
            assert got.vert_attr is None
        else:
            assert same(got.vert_attr[b].cpu().numpy(), w.vert_attr), (b, "vert_attr")
    plain = hip_ops.marching_tets(dev(pos), dev(field), top, iso=iso)
    assert plain.edge_id is None and plain.t is None and plain.tet_id is None and plain.vert_attr is None
    assert all(torch.equal(a, b) for a, b in zip(plain.verts, got.verts)) and all(torch.equal(a, b) for a, b in zip(plain.faces, got.faces))
    return got, wants


def watertight(mesh):
    two, once, euler = R.closed_and_oriented(mesh.faces, mesh.verts.shape[0])
    return two and once and euler == 2 and R.signed_volume(mesh.verts, mesh.faces) > 0 and (mesh.t >= 0).all() and (mesh.t <= 1).all()


# ------------------------------------------------------------------------------------------------------------ forward
def test_all_sixteen_codes_in_both_orientations(cuda):
    tets = np.array([[0, 1, 2, 3]], np.int64)
    edges, tet_edge = R.tet_edges(tets)
    top = topology(cuda, tets, 4, edges, tet_edge)
    rng = np.random.default_rng(0)
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    pos, field = np.empty((32, 4, 3), np.float32), np.empty((32, 4), np.float32)
    for s in range(32):
        p = base + rng.uniform(-0.1, 0.1, (4, 3)).astype(np.float32)
        pos[s] = p[[0, 1, 3, 2]] if s >= 16 else p                                   # corners 2 and 3 swapped: a negative tet
        ins = np.array([(s & 15) >> k & 1 for k in range(4)], bool)
        field[s] = np.where(ins, rng.uniform(0.2, 1.0, 4), -rng.uniform(0.2, 1.0, 4))
    attr = K.attrs(32, 4, 3, 1)
    got, wants = run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, 0.0, attr)
    for s, w in enumerate(wants):
        code, n_in = s & 15, bin(s & 15).count("1")
        assert w.faces.shape[0] == (0, 1, 2, 1, 0)[n_in] and w.verts.shape[0] == (0, 3, 4, 3, 0)[n_in]
        if w.faces.shape[0]:
            ins = field[s] > 0
            out_dir = pos[s][~ins].mean(0) - pos[s][ins].mean(0)
            v = got.verts[s].cpu().numpy()[got.faces[s].cpu().numpy()]
            dots = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) @ out_dir
            assert (dots > 0).all() if s < 16 else (dots < 0).all(), (code, s)          # the negative tet comes out flipped


@pytest.fixture(scope="module")
def kuhn4(cuda):
    pos, tets, edges, tet_edge = K.grid(4, 3)
    return pos, tets, edges, tet_edge, topology(cuda, tets, pos.shape[1], edges, tet_edge)


def test_values_on_the_iso_level(cuda, kuhn4):
    pos, tets, edges, tet_edge, top = kuhn4
    assert tets.shape[0] == 48 and pos.shape[1] == 27
    rng = np.random.default_rng(5)
    field = rng.choice(np.array([-1, 0, 1], np.float32), (3, 27))
    _got, wants = run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, 0.0, K.attrs(3, 27, 2, 2))
    assert any((w.t == 0).any() for w in wants) and any((w.t == 1).any() for w in wants)  # an end ON the level is outside: t = 0 or 1
    field = rng.choice(np.array([0, 1], np.float32), (3, 27))
    _got, wants = run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, 0.5)
    assert all(w.verts.shape[0] > 0 and (w.t == 0.5).all() for w in wants)             # every vertex an exact midpoint


@pytest.fixture(scope="module")
def kuhn8(cuda):
    pos, tets, edges, tet_edge = K.grid(8, 4)
    return pos, tets, edges, tet_edge, topology(cuda, tets, pos.shape[1], edges, tet_edge), K.field8(pos)


@pytest.mark.parametrize("C", [8, 1])
def test_batch_with_empty_shapes_between_full_ones(cuda, kuhn8, C):
    pos, tets, edges, tet_edge, top, field = kuhn8
    assert tets.shape[0] == 384
    got, wants = run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, 0.0, K.attrs(4, pos.shape[1], C, 4))
    assert [w.faces.shape[0] > 0 for w in wants] == [False, True, False, True]
    assert got.verts[0].shape == (0, 3) and got.faces[2].shape == (0, 3) and got.vert_attr[0].shape == (0, C)
    assert watertight(wants[1])
    code = ((field[3] > 0)[tets] << np.arange(4)).sum(1)
    assert ((code != 0) & (code != 15)).mean() > 0.8                                   # the random field: nearly every tet is mixed


def test_arbitrary_numbering_and_a_subdivided_list(cuda):
    from deftet_amd import hip_ops
    pos, tets, _e, _te = K.grid(8, 1)
    rng = np.random.default_rng(9)
    tets = tets[rng.permutation(tets.shape[0])]
    tets = np.take_along_axis(tets, np.argsort(rng.random(tets.shape), axis=1), axis=1)
    edges, tet_edge = R.tet_edges(tets)
    top = topology(cuda, tets, pos.shape[1], edges, tet_edge)
    field = K.sphere(pos[0], 0.3)[None]
    _got, wants = run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, 0.0, K.attrs(1, pos.shape[1], 3, 6))
    two, once, euler = R.closed_and_oriented(wants[0].faces, wants[0].verts.shape[0])
    assert two and euler == 2 and not once                                             # closed; mixed orientations: not consistently wound
    p2, _f2, t2 = hip_ops.subdivide(torch.from_numpy(tets).to(cuda), torch.from_numpy(pos[0].copy()).to(cuda),
                                    torch.from_numpy(field[0][:, None].copy()).to(cuda))
    p2, t2 = p2.cpu().numpy()[None], t2.cpu().numpy()
    assert t2.shape[0] == 8 * tets.shape[0]
    edges2, tet_edge2 = R.tet_edges(t2)
    top2 = topology(cuda, t2, p2.shape[1], edges2, tet_edge2)
    _got, wants = run_and_compare(cuda, top2, p2, K.sphere(p2[0], 0.3)[None], t2, edges2, tet_edge2, 0.0, K.attrs(1, p2.shape[1], 2, 8))
    assert wants[0].faces.shape[0] > 200 and R.closed_and_oriented(wants[0].faces, wants[0].verts.shape[0])[0]


@pytest.fixture(scope="module")
def kuhn20(cuda):
    pos, tets, edges, tet_edge = K.grid(20, 5)
    return pos, tets, edges, tet_edge, topology(cuda, tets, pos.shape[1], edges, tet_edge), K.field20(pos)


def test_past_the_block_boundaries(cuda, kuhn20):
    """B (E + T) + 1 = 69,651 counts: past the one-workgroup scan of prims.hpp (kScanSmall = 8,192 elements — the single-block
    limit meant) and 35 of its 2,048-element tiles; B T = 30,000 and B E = 39,650 each exceed it too.  The CSR sorts 2 E =
    15,860 keys: eight tiles."""
    pos, tets, edges, tet_edge, top, field = kuhn20
    assert tets.shape[0] == 6000 and pos.shape[1] == 1331 and 5 * edges.shape[0] > 8192 and 2 * edges.shape[0] > 4 * 2048
    _got, wants = run_and_compare(cuda, top, pos, field, tets, edges, tet_edge, 0.0, K.attrs(5, 1331, 3, 10))
    assert all(watertight(w) for w in wants)


# ------------------------------------------------------------------------------------------------------------ backward
def backward_case(cuda, top, pos, field, edges, C, seed):
    from deftet_amd import hip_ops
    B, V = field.shape
    for b in range(B):
        assert K.crossing_gap(field[b], edges) > K.GAP, b                                # the input's condition, not the code's
    attr = K.attrs(B, V, C, seed)
    leaves = [torch.from_numpy(np.array(x)).to(cuda).requires_grad_(True) for x in (pos, field, attr)]
    rng = np.random.default_rng(seed)
    normal = lambda x: torch.from_numpy(rng.normal(size=tuple(x.shape)).astype(np.float32)).to(cuda)
    m = hip_ops.marching_tets(*leaves[:2], top, iso=0.0, attr=leaves[2], return_index=True)
    assert not any(t.requires_grad for t in m.faces + m.edge_id + m.tet_id + m.t)
    gv, ga = [normal(v) for v in m.verts], [normal(a) for a in m.vert_attr]              # N(0,1) gradients of both outputs

    def grads_of(mesh):
        loss = sum((v * g).sum() for v, g in zip(mesh.verts, gv)) + sum((a * g).sum() for a, g in zip(mesh.vert_attr, ga))
        return torch.autograd.grad(loss, leaves)
    grads = grads_of(m)
    for b in range(B):
        want = R.grads64(pos[b], field[b], edges, 0.0, gv[b].cpu().numpy(), attr[b], ga[b].cpu().numpy())
        untouched = np.ones(V, bool)
        untouched[edges[m.edge_id[b].cpu().numpy()].reshape(-1)] = False
        for name, g, w in zip(("grad_pos", "grad_field", "grad_attr"), grads, want):
            check_close("%s[%d]" % (name, b), g[b], w, MAXNORM)
            assert not g[b].cpu().numpy()[untouched].any(), (name, b)                     # exact zeros away from the surface
    again = grads_of(hip_ops.marching_tets(*leaves[:2], top, iso=0.0, attr=leaves[2]))   # a second run: the same bits
    assert all(torch.equal(a, b) for a, b in zip(grads, again))
    return grads


@pytest.mark.parametrize("C", [3, 8])
def test_backward_on_the_sphere_and_the_random_field(cuda, kuhn8, C):
    pos, _tets, edges, _te, top, field = kuhn8
    grads = backward_case(cuda, top, pos, field, edges, C, 21)
    assert not grads[0][0].any() and not grads[1][2].any()                               # the empty shapes: all zero
    assert grads[0][1].abs().max() > 0 and grads[1][3].abs().max() > 0 and grads[2][3].abs().max() > 0


def test_backward_past_the_block_boundaries(cuda, kuhn20):
    pos, _tets, edges, _te, top, field = kuhn20
    backward_case(cuda, top, pos, field, edges, 2, 22)


def test_backward_of_one_output_and_without_attributes(cuda, kuhn8):
    """only verts (no attr), only vert_attr, and a [V,3] position: the gradients of the parts equal the parts of the whole"""
    from deftet_amd import hip_ops
    pos, _tets, edges, _te, top, field = kuhn8
    p = torch.from_numpy(pos[1].copy()).to(cuda).requires_grad_(True)                    # [V,3]: one shape
    f = torch.from_numpy(field[1].copy()).to(cuda).requires_grad_(True)
    a = torch.from_numpy(K.attrs(1, pos.shape[1], 3, 30)[0]).to(cuda).requires_grad_(True)
    m = hip_ops.marching_tets(p, f, top, attr=a)
    assert len(m.verts) == 1
    gv, ga = torch.randn_like(m.verts[0]), torch.randn_like(m.vert_attr[0])
    whole = torch.autograd.grad((m.verts[0] * gv).sum() + (m.vert_attr[0] * ga).sum(), (p, f, a))
    assert whole[0].shape == p.shape and whole[1].shape == f.shape and whole[2].shape == a.shape
    m = hip_ops.marching_tets(p, f, top, attr=a)
    only_v = torch.autograd.grad((m.verts[0] * gv).sum(), (p, f, a), allow_unused=True)
    m = hip_ops.marching_tets(p, f, top, attr=a)
    only_a = torch.autograd.grad((m.vert_attr[0] * ga).sum(), (p, f, a), allow_unused=True)
    assert torch.equal(only_v[0], whole[0]) and torch.equal(only_a[2], whole[2])
    assert not only_a[0].any() and not only_v[2].any()
    want = R.grads64(pos[1], field[1], edges, 0.0, gv.cpu().numpy(), a.detach().cpu().numpy(), ga.cpu().numpy())
    check_close("grad_field of the parts", (only_v[1] + only_a[1]), want[1], MAXNORM)
    m = hip_ops.marching_tets(p, f, top)
    no_attr = torch.autograd.grad((m.verts[0] * gv).sum(), (p, f))
    assert torch.equal(no_attr[0], whole[0]) and torch.equal(no_attr[1], only_v[1])


# ------------------------------------------------------------------------------------------------------------ per entry
# Against float64 entry by entry ("What is pinned"): no condition on the crossing gaps, every level of K.ISOS,
# every attribute width.  The bounds are derived (R.forward64, R.entry_bound), not measured; tests/test_marching_tets_cpu.py
# holds the reference, the bounds and the inputs to their own conditions without a GPU.
@pytest.fixture(scope="module")
def tops(cuda):
    """name of a per-entry input -> its TetEdges, one per tet list"""
    built = {}

    def get(name):
        pos, _field, tets, edges, tet_edge, _iso = K.per_entry_case(name)
        if id(tets) not in built:
            built[id(tets)] = (tets, topology(cuda, tets, pos.shape[1], edges, tet_edge))
        return built[id(tets)][1]
    return get


@pytest.mark.parametrize("name", K.FORWARD)
def test_forward_within_the_fp64_bounds(cuda, tops, name):
    """Bit for bit against the restatement, then t within 4u |t64| and verts, vert_attr within 6u (|x_min| + |x_max|) of the
    float64 evaluation of the same float32 inputs, u = 2^-24: thin fields (gaps down to 1.8e-6 of the range) at iso 0.0, 0.1 and
    -0.37, spheres not picked for their gap, a subdivided list, and a field of float32(0.1) and its two neighbours at iso = 0.1.
    Measured on an MI355X, error over bound at the worst: t 0.57, verts 0.48, vert_attr 0.35 (the restatement's own: bit-equal)."""
    from deftet_amd import hip_ops
    pos, field, tets, edges, tet_edge, iso = K.per_entry_case(name)
    attr = K.attrs(field.shape[0], field.shape[1], 3, 40)
    got, wants = run_and_compare(cuda, tops(name), pos, field, tets, edges, tet_edge, iso, attr)
    for b, w in enumerate(wants):
        assert w.t.size > 20
        (t, bt), (v, bv), (a, ba) = R.forward64(pos[b], field[b], edges, iso, attr[b])
        check_bound("mt fwd t %s[%d]" % (name, b), got.t[b], t, bt)
        check_bound("mt fwd verts %s[%d]" % (name, b), got.verts[b], v, bv)
        check_bound("mt fwd vert_attr %s[%d]" % (name, b), got.vert_attr[b], a, ba)
        if name.startswith("level"):
            assert np.isin(w.t, (0, 0.5, 1)).all() and (w.t == 0).any() and (w.t == 1).any()
    if name == "subdivided8":                                                            # the list IS the operator's subdivision
        p0, t0, _e, _te = K.shuffled8()
        p2, _f2, t2 = hip_ops.subdivide(torch.from_numpy(np.array(t0)).to(cuda), torch.from_numpy(np.array(p0[0])).to(cuda),
                                        torch.zeros(p0.shape[1], 1, device=cuda))
        assert same(p2.cpu().numpy()[None], pos) and same(t2.cpu().numpy(), tets)


def run_backward(cuda, top, pos, field, iso, attr, gv, ga):
    """(mesh, gradients of sum(verts gv) + sum(vert_attr ga) for (pos, field[, attr]), the same of a second forward)"""
    from deftet_amd import hip_ops
    dev = lambda x: torch.from_numpy(np.array(x)).to(cuda)
    leaves = [dev(x).requires_grad_(True) for x in ((pos, field) if attr is None else (pos, field, attr))]
    gv, ga = [dev(g) for g in gv], None if attr is None else [dev(g) for g in ga]

    def grads_of(mesh):
        assert [tuple(v.shape) for v in mesh.verts] == [tuple(g.shape) for g in gv]
        loss = sum((v * g).sum() for v, g in zip(mesh.verts, gv))
        if attr is not None:
            loss = loss + sum((a * g).sum() for a, g in zip(mesh.vert_attr, ga))
        return torch.autograd.grad(loss, leaves)
    call = lambda **kw: hip_ops.marching_tets(leaves[0], leaves[1], top, iso=iso, attr=None if attr is None else leaves[2], **kw)
    m = call(return_index=True)
    return m, grads_of(m), grads_of(call())


def per_entry_case(cuda, tops, name, C):
    """Every gradient entry within 2^-24 |want| + 2^-40 S + 2^-149 of the float64 terms (R.entry_bound: a double accumulation
    rounded once), and the assertions of backward_case without its GAP condition: maxnorm 1e-5, exact zeros at untouched
    vertices, the same bits from a second run."""
    pos, field, _tets, edges, _te, iso = K.per_entry_case(name)
    attr, gv, ga = K.per_entry_gradients(name, C)
    m, grads, again = run_backward(cuda, tops(name), pos, field, iso, attr, gv, ga)
    for b in range(field.shape[0]):
        want, S = R.grads64_terms(pos[b], field[b], edges, iso, gv[b], None if attr is None else attr[b], None if ga is None else ga[b])
        untouched = np.ones(field.shape[1], bool)
        untouched[edges[m.edge_id[b].cpu().numpy()].reshape(-1)] = False
        for gname, g, w, s in zip(("grad_pos", "grad_field", "grad_attr"), grads, want, S):
            check_bound("mt bwd %s %s C=%d [%d]" % (gname, name, C, b), g[b], w, R.entry_bound(w, s))
            check_close("mt bwd %s %s C=%d [%d] maxnorm" % (gname, name, C, b), g[b], w, MAXNORM)
            assert not g[b].cpu().numpy()[untouched].any(), (gname, b)
    assert len(grads) == (2 if C == 0 else 3) and all(torch.equal(a, b) for a, b in zip(grads, again))
    return m


@pytest.mark.parametrize("C", K.WIDTHS)
@pytest.mark.parametrize("iso", K.ISOS)
def test_backward_per_entry_on_thin_fields_every_level_and_width(cuda, tops, iso, C):
    """Crossing gaps from 1.8e-6 of the field's range to all of it, B = 3, V = 125 (one partial block), iso 0.0, 0.1 and -0.37
    (the level is float32(iso)), no attributes and every width 1..8: <0>, <4> partial and full, <8> partial and full.  Float32
    accumulation misses this bound by a factor 18 to 7.6e7 on the same fields (tests/test_marching_tets_cpu.py).  Measured on an
    MI355X, error over bound at the worst of all 27 cases: grad_pos 0.9996, grad_field 0.997, grad_attr 0.994 (the float64 terms
    rounded once reach the same 0.9996); max-norm error 5.7e-8 at the most."""
    per_entry_case(cuda, tops, "thin8@%s" % iso, C)


@pytest.mark.parametrize("name", [n for n in K.PER_ENTRY if not n.startswith("thin8")])
def test_backward_per_entry_on_the_other_inputs(cuda, tops, name):
    """thin20@0.1: B = 2, V = 1331 (six blocks, the last partial), C = 5.  spheres20, subdivided8: crossing gaps of 0.48 %, 0.27 %
    and 0.9 % of the range, under the GAP of the max-norm tests; `+0.25` is the same field shifted, with iso = 0.25: the same
    topology.  shuffled8-thin: negative tets and edge ends in either field order, iso = -0.37, C = 3.  kuhn8, kuhn20: the inputs
    of the max-norm tests under the per-entry bound.  Measured on an MI355X, error over bound at the worst: grad_pos 0.998,
    grad_field 0.983, grad_attr 0.994."""
    meshes = [per_entry_case(cuda, tops, name, C) for C in K.PER_ENTRY[name]]
    if name.endswith("+0.25"):
        base = per_entry_case(cuda, tops, name[:-5], 0)
        for b in range(len(base.faces)):
            assert base.faces[b].shape[0] > 200
            for part in ("faces", "edge_id", "tet_id"):
                assert torch.equal(getattr(base, part)[b], getattr(meshes[0], part)[b]), (part, b)


def test_non_finite_field_values_stay_where_they_are(cuda, tops):
    """Containment.  Shape 0: a banded field with six interior vertices, no two joined, at NaN, +inf, -inf, NaN, +inf, -inf;
    shape 1: clean.  NaN and -inf count as outside, +inf as inside: faces, edge_id, tet_id and the row counts equal the
    restatement's.  verts, t, vert_attr: the rows of unaffected edges bit for bit; an affected row (a crossing edge with a
    non-finite end) has NaN where the restatement has NaN and the same bytes elsewhere — +-inf at the higher vertex id gives
    t = +-0 and the vertex p_min, +-inf at the lower id and NaN at either give NaN.  Gradients: at every vertex that is no end
    of an affected edge, within the per-entry bound of the float64 terms summed without those edges, and exactly zero without a
    crossing edge; the clean shape's gradients carry the bits of a run of the clean shape alone.  NOTHING is asserted at the
    affected vertices (at most 90 of 1331, under 10 % of the vertices with a crossing edge: asserted on the CPU): the gradients
    there hold NaN, 0 or a finite number as IEEE gives them.  Measured on an MI355X, error over bound at the worst: grad_pos 0.989,
    grad_field 0.987, grad_attr 0.992."""
    name, C = "hostile20", 3
    from deftet_amd import hip_ops
    pos, field, tets, edges, tet_edge, iso = K.per_entry_case(name)
    _f, bad_edge, bad_vertex = K.hostile(K.banded(field.shape[1], 170), 171)
    attr, gv, ga = K.per_entry_gradients(name, C)
    m, grads, again = run_backward(cuda, tops(name), pos, field, iso, attr, gv, ga)
    for b in range(2):
        w = R.marching_tets(pos[b], field[b], tets, iso, attr=attr[b], edges=edges, tet_edge=tet_edge)
        for part in ("faces", "edge_id", "tet_id"):
            assert same(getattr(m, part)[b].cpu().numpy(), getattr(w, part)), (b, part)
        clean_row = ~bad_edge[w.edge_id] if b == 0 else np.ones(w.edge_id.size, bool)
        assert (~clean_row).sum() == (bad_edge.sum() if b == 0 else 0)
        for part in ("verts", "t", "vert_attr"):
            g = getattr(m, part)[b].detach().cpu().numpy()
            assert same(g[clean_row], getattr(w, part)[clean_row]) and np.isfinite(g[clean_row]).all(), (b, part)
            assert R.same_rows_nan_aware(g, getattr(w, part)), (b, part)
        skip, ok = (bad_edge, ~bad_vertex) if b == 0 else (None, np.ones(field.shape[1], bool))
        want, S = R.grads64_terms(pos[b], field[b], edges, iso, gv[b], attr[b], ga[b], skip=skip)
        untouched = np.ones(field.shape[1], bool)
        untouched[edges[w.edge_id].reshape(-1)] = False
        for gname, g, x, s in zip(("grad_pos", "grad_field", "grad_attr"), grads, want, S):
            mask = ok if x.ndim == 1 else ok[:, None]
            check_bound("mt bwd %s %s C=%d [%d] unaffected" % (gname, name, C, b), g[b], x, R.entry_bound(x, s), mask=mask)
            assert not g[b].cpu().numpy()[untouched].any(), (gname, b)
    assert not np.isfinite(grads[1][0].cpu().numpy()[bad_vertex]).all()                 # (the hostile values did reach the backward)
    assert all(same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(grads, again))        # (bytes: a NaN equals itself)
    _m, alone, _again = run_backward(cuda, tops(name), pos[1:], field[1:], iso, attr[1:], gv[1:], ga[1:])
    assert all(torch.equal(g[1], a[0]) for g, a in zip(grads, alone))


# ------------------------------------------------------------------------------------------------------------ model path
class StubModel:
    """the attributes and methods the marching-tetrahedra export reads of a render model (3_model/deftet.py:503-523)"""

    def __init__(self, points, tets, dev):
        g = torch.Generator().manual_seed(5)
        self.coef = 1.25
        self.tfpoint_px3 = (torch.from_numpy(points.copy()) / self.coef).to(dev)
        self.tfpointmov_px3 = (torch.randn(points.shape, generator=g) * 0.005).to(dev).requires_grad_(True)
        self.tfpointfeat_pxd = torch.randn(points.shape[0], 4, generator=g).to(dev).requires_grad_(True)
        self.tftet_tx4 = torch.from_numpy(tets.copy()).to(dev)

    def get_point(self, with_coef=False):
        p = self.tfpoint_px3 + self.tfpointmov_px3
        return self.coef * p if with_coef else p

    def get_feat(self):
        return self.tfpointfeat_pxd


def processfunc(points, feat):
    """weights [P,1] = a soft sphere of radius 0.3 nudged by the first feature, colours [P,3] = sigmoid of the others"""
    w = torch.sigmoid((0.3 - points.norm(dim=1, keepdim=True)) * 20 + 0.1 * feat[:, :1])
    return w, torch.sigmoid(feat[:, 1:4])


def parse_obj(path, n_numbers):
    v, f = [], []
    for line in open(path):
        tok = line.split()
        if tok[0] == "v":
            assert len(tok) == 1 + n_numbers
            v.append(tok[1:])
        else:
            assert tok[0] == "f"
            f.append([int(x) - 1 for x in tok[1:]])
    return v, np.asarray(f, np.int64).reshape(-1, 3)


def test_model_path_and_obj_export(cuda, tmp_path):
    from deftet_amd import hip_ops
    from deftet_amd.render import export, marching_tets
    pos, tets, _edges, _te = K.grid(8, 1)
    V = pos.shape[1]
    model = StubModel(pos[0], tets, cuda)
    mesh = marching_tets(model, 0.25, processfunc, return_index=True)
    w, col = processfunc(model.get_point(True), model.get_feat())
    direct = hip_ops.marching_tets(model.get_point(True), w.reshape(1, -1), hip_ops.TetEdges(model.tftet_tx4, V), iso=0.25, attr=col,
                                   return_index=True)
    assert mesh.verts.shape[0] > 20 and mesh.faces.shape[0] > 40
    for got, want in zip(mesh, direct):
        assert torch.equal(got, want[0])
    gm, gf = torch.autograd.grad(mesh.verts.square().sum() + mesh.vert_attr.sum(), (model.tfpointmov_px3, model.tfpointfeat_pxd))
    assert gm.shape == (V, 3) and gf.shape == (V, 4) and gm.abs().max() > 0 and gf[:, 0].abs().max() > 0 and gf[:, 1:].abs().max() > 0
    kept = model._deftet_tet_edges[1]
    marching_tets(model, 0.25, processfunc)
    assert model._deftet_tet_edges[1] is kept                                            # the same list object: kept
    model.tftet_tx4 = model.tftet_tx4[: tets.shape[0] // 2].clone()                      # a new list object (deletetet): rebuilt
    half = marching_tets(model, 0.25, processfunc)
    assert model._deftet_tet_edges[1] is not kept and model._deftet_tet_edges[1].n_tet == tets.shape[0] // 2
    assert 0 < half.faces.shape[0] < mesh.faces.shape[0]
    # the export: the marching-tetrahedra files beside the threshold sweep's
    model.tftet_tx4 = torch.from_numpy(tets.copy()).to(cuda)
    nbr = hip_ops.tet_face_neighbours(tets, V, cuda)
    paths = export.save_surface_objs(model.get_point(True), (w, col), tets, nbr, str(tmp_path), "stub", thresholds=(0.25,), iso=0.25)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["tet-geo-stub-thres-0.250.obj", "tet-color-stub-thres-0.250.obj",
                                                      "mt-geo-stub-iso-0.250.obj", "mt-color-stub-iso-0.250.obj"]
    want_v = mesh.verts.detach().cpu().numpy().astype(np.float64)
    want_c = mesh.vert_attr.detach().cpu().numpy()[:, ::-1].astype(np.float64)          # colours are written reversed, as saveobj does
    v, f = parse_obj(paths[2], 3)
    assert v == [("%f %f %f" % tuple(r)).split() for r in want_v] and same(f, mesh.faces.cpu().numpy())
    v, f = parse_obj(paths[3], 6)
    assert v == [("%f %f %f %f %f %f" % (tuple(r) + tuple(c))).split() for r, c in zip(want_v, want_c)] and same(f, mesh.faces.cpu().numpy())
    assert len(export.save_surface_objs(model.get_point(True), (w, col), tets, nbr, str(tmp_path), "plain", thresholds=(0.25,))) == 2


def test_topology_errors_and_the_cached_accessor(cuda):
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import TetTopology
    pos, tets, edges, tet_edge = K.grid(4, 1)
    t = torch.from_numpy(tets.copy()).to(cuda)
    bad = t.clone()
    bad[3, 2] = 27
    with pytest.raises(IndexError):
        hip_ops.TetEdges(bad, 27)
    bad[3, 2] = -1
    with pytest.raises(IndexError):
        hip_ops.TetEdges(bad, 27)
    topo = TetTopology(t[None], 27)
    e = topo.edges()
    assert isinstance(e, hip_ops.TetEdges) and topo.edges() is e and same(e.edges.cpu().numpy().astype(np.int64), edges)
    host = hip_ops.TetEdges(tets, 27, device=cuda)                                       # a host list, put on the device
    assert torch.equal(host.tet_edge, e.tet_edge)
    with pytest.raises(TypeError):
        hip_ops.marching_tets(torch.zeros(1, 27, 3, device=cuda), torch.zeros(1, 27, device=cuda), topo)
    with pytest.raises(RuntimeError):
        hip_ops.marching_tets(torch.zeros(1, 26, 3, device=cuda), torch.zeros(1, 26, device=cuda), e)
    with pytest.raises(hip_ops._lib.DefTetHipError):
        hip_ops.marching_tets(torch.zeros(1, 27, 3, device=cuda), torch.zeros(1, 27, device=cuda), e, iso=float("nan"))
