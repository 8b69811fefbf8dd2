"""The point-in-tet weights and backward (A1b) against fp64 on tets of known conditioning: well shaped, flattened
to 1/10 and 1/100, small next to their coordinates, and 100 units from the origin (tests/bary_cases.py; tests/test_bary_ref_cpu.py
is the CPU half and says where the bounds come from).  The tets of a shape are disjoint and every query is made inside a tet, so
the index is known without an oracle.  Per asserted tet (kappa <= 5e4) or query of one, with u = 2^-24 and K = bary_cases.K:

    weights     max|err| <= K u kappa max(1, max|w|)             grad_tet   max|err| <= (K + n_t) u kappa_t S_t
    grad_pts    max|err| <= K u kappa max|G|                     grad_pos   the sum of the bounds of the incident tets
    grad_pred   |err| <= (2 + log2 n + n / 64) u sum|term|       (n terms added into the entry; every miss goes to tet 0)

forward     every band x algo 0-5: index == the tet the query was made in, weights bit-equal to the CPU oracle and within the bound.
backward    every band x every path, each with want_grad_pts / grad_occ both on and both off; the backward takes the GPU's own index:
            records and spill records; overflowed records (ordered scan of the uncovered list); the per-tet lists (with and without
            hits=); the float-atomic fallback; onto the vertices from the gathered tensor and from the index list, with one and with
            per-shape index lists; out= accumulation.  grad_pts is exactly zero on the misses.
butterfly   1,728 tets, one of them with 2,048 hits: the unordered list scan with the butterfly.
mixed       three bands in one batch: no shape's box or scale reaches another shape's result.
autograd    point_in_tet_bary and DefTet.occupancy_query (gathered and indexed) on the 1/100 band.

Every comparison reports its worst error / bound (tests/tol.check_bound); profiles/bary_backward_tolerances.jsonl is an MI355X run:
weights <= 0.032, grad_tet and grad_pos <= 0.052, grad_pts <= 0.137 (what the fp32 restatement gives on the CPU), grad_pred <= 0.50.
"""
import numpy as np
import pytest
import torch

from tests import bary_cases as C
from tests import bary_ref as R
from tests.tol import check_bound

pytestmark = pytest.mark.gpu

BOTH = [True, False]                                                 # want_grad_pts and grad_occ: both on, both off


def _t(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _n(x):
    return x.detach().cpu().numpy()


class Case:
    """B shapes as one batch, forwarded once: index, weights, hit records; the fp64 reference per shape for the GPU's own index"""

    def __init__(self, name, shapes, cuda, algo=0, check_forward=True):
        from deftet_amd import hip_ops
        self.name, self.shapes, self.B = name, shapes, len(shapes)
        self.T, self.Q = shapes[0]["tet"].shape[0], shapes[0]["pts"].shape[0]
        inc = [C.incoming(s) for s in shapes]
        self.gw_np, self.go_np = [g[0] for g in inc], [g[1] for g in inc]
        self.tet, self.pts = _t(np.stack([s["tet"] for s in shapes]), cuda), _t(np.stack([s["pts"] for s in shapes]), cuda)
        self.gw, self.go = _t(np.stack(self.gw_np), cuda), _t(np.stack(self.go_np), cuda)
        self.pred = torch.rand(self.B, self.T, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3))
        self.cond, self.w, self.occ, self.hits = hip_ops.point_in_tet(self.tet, self.pts, want_bary=True, pred_bxt=self.pred,
                                                                      want_hits=True, algo=algo)
        self.stats = hip_ops.point_in_tet_stats(self.B, self.T, self.Q, algo, cuda)
        self.cond_np = _n(self.cond)[..., 0]
        self.refs = [R.analytic(s["tet"], s["pts"], self.cond_np[b], self.gw_np[b], self.go_np[b]) for b, s in enumerate(shapes)]
        if check_forward:
            for b, s in enumerate(shapes):
                assert_index(s, self.cond_np[b], "%s[%d]" % (name, b))

    def overflowed(self):
        """bool [B,T]: the tets whose hit record says "more than the record and its spill record hold" (.y == -2)"""
        return _n(self.hits[: self.B * self.T * 2].view(self.B, self.T, 2)[..., 1]) == -2

    def on_asserted(self, b):
        """bool [Q]: hits of the shape's asserted tets"""
        r = self.refs[b]
        return r["hit"] & self.shapes[b]["asserted"][r["t"]]

    def hold(self, path, grad_tet=None, grad_pts=None, grad_pred=None, grad_pos=None, idx=None, base=None, w=None):
        """every given output against fp64 within its bound; returns the worst ratios"""
        worst = {}
        for b, s in enumerate(self.shapes):
            r, k, a = self.refs[b], s["kappa"], s["asserted"]
            tag = "bary pin, %s[%d], %s, " % (self.name, b, path)
            if w is not None:
                worst["w"] = check_bound(tag + "w", _n(w[b]), r["w"], R.bound_w(r, k)[:, None], mask=self.on_asserted(b)[:, None])
                assert not _n(w[b])[~r["hit"]].any()
            if grad_tet is not None:
                worst["grad_tet"] = check_bound(tag + "grad_tet", _n(grad_tet[b]), r["grad_tet"], R.bound_tet(r, k)[:, None, None],
                                                mask=a[:, None, None])
            if grad_pts is not None:
                worst["grad_pts"] = check_bound(tag + "grad_pts", _n(grad_pts[b]), r["G"], R.bound_G(r, k)[:, None],
                                                mask=self.on_asserted(b)[:, None])
                assert (~r["hit"]).any() and not _n(grad_pts[b])[~r["hit"]].any()      # exactly zero on the misses
            if grad_pred is not None:
                assert r["pred_n"][0] - (r["t"][r["hit"]] == 0).sum() == (~r["hit"]).sum() > 0    # tet 0 also sums the misses
                worst["grad_pred"] = check_bound(tag + "grad_pred", _n(grad_pred[b]), r["grad_pred"], R.bound_pred(r))
            if grad_pos is not None:
                i = idx[b if idx.shape[0] > 1 else 0]
                V = i.size
                want = R.scatter_to_vertices(r["grad_tet"], i, V)
                bound = R.scatter_to_vertices(np.broadcast_to(R.bound_tet(r, k)[:, None, None], (self.T, 4, 3)), i, V)
                ok = R.scatter_to_vertices(np.broadcast_to((~a)[:, None], (self.T, 4)).astype(np.float64), i, V) == 0
                if base is not None:                                 # out=: one more fp32 addition per entry
                    want = want + _n(base[b]).astype(np.float64)
                    bound = bound + C.U * (np.abs(_n(base[b])) + np.abs(want))
                worst["grad_pos"] = check_bound(tag + "grad_pos", _n(grad_pos[b]), want, bound, mask=ok[:, None])
        return worst


def assert_index(s, cond, what):
    """the query's tet where that tet is asserted, -1 in the empty margins"""
    own = s["own"]
    check = (own < 0) | s["asserted"][np.maximum(own, 0)]
    assert np.array_equal(cond[check].astype(np.int64), own[check]), (what, int((cond[check] != own[check]).sum()))
    assert 0.05 < (cond < 0).mean() < 0.15, what


@pytest.fixture(scope="module")
def cases(cuda):
    made = {}

    def get(kind, band=None):
        key = (kind, band)
        if key not in made:
            name = kind if band is None else "%s-%g %s" % (band + (kind,))
            shapes = {"records": lambda: [C.records_shape(band)], "overflow": lambda: [C.overflow_shape(band)],
                      "lists": lambda: [C.lists_shape(band)], "pair": lambda: C.pair_batch(band),
                      "butterfly": lambda: [C.butterfly_shape()], "mixed": C.mixed_batch}[kind]()
            made[key] = Case(name, shapes, cuda)
        return made[key]

    return get


def _soup(case, cuda, per_shape):
    """the case's tets as (pos [B,4T,3], idx [T,4] or [B,T,4], csr): every tet with four vertices of its own, scattered"""
    from deftet_amd import hip_ops
    idx = np.stack([C.soup_topology(case.T, seed=b) for b in range(case.B if per_shape else 1)])
    pos = np.stack([C.soup_positions(s["tet"], idx[b if per_shape else 0]) for b, s in enumerate(case.shapes)])
    t_idx = _t(idx if per_shape else idx[0], cuda)
    csr = hip_ops.tet_vertex_csr(t_idx, 4 * case.T)
    assert csr[2] == (case.B if per_shape else 1)
    t_pos = _t(pos, cuda)
    assert torch.equal(hip_ops.tet_gather(t_pos, t_idx), case.tet)
    return t_pos, t_idx, idx, csr


# ---- forward ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_forward_index_and_weights(cuda, oracle, cases, band):
    from deftet_amd import hip_ops
    c = cases("overflow", band)
    s = c.shapes[0]
    assert C.asserted_share(s) >= C.MIN_ASSERTED_SHARE and c.on_asserted(0).sum() > 300
    for algo in range(6):
        cond, w = hip_ops.point_in_tet(c.tet, c.pts, want_bary=True, algo=algo)
        assert_index(s, _n(cond)[0, :, 0], "%s algo %d" % (c.name, algo))
        assert torch.equal(cond, c.cond), algo
        assert np.array_equal(_n(w), oracle.bary(s["tet"][None], s["pts"][None], c.cond_np)), algo
        c.hold("forward algo %d" % algo, w=w)


# ---- backward ---------------------------------------------------------------------------------------------------------------

def _bwd(c, on, hits):
    from deftet_amd import hip_ops
    out = hip_ops.point_in_tet_bwd(c.tet, c.pts, c.cond, c.gw, want_grad_pts=on, grad_occ=c.go if on else None, hits=hits)
    assert (out[1] is not None) == on and len(out) == (3 if on else 2)
    return dict(zip(("grad_tet", "grad_pts", "grad_pred"), out))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_backward_from_records_and_spill_records(cuda, cases, band, on):
    from deftet_amd import hip_ops
    c = cases("records", band)
    assert hip_ops.bwd_uses_records(c.T, c.Q) and c.stats[0, 6] == 0                    # no tet accepted more than six queries
    # (the traversal treats flattened tets as irregular: it marks their records and lists their hits, whatever their number, so
    # on those bands the marked tets take the list scan below and only the well shaped bands are records alone)
    assert band[1] < 1.0 or not c.overflowed().any()
    n = c.refs[0]["n"]
    assert ((n >= 1) & (n <= 2)).sum() > 100 and ((n >= 3) & (n <= 6)).sum() > 50 and n.max() == 6
    c.hold("records", **_bwd(c, on, c.hits))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_backward_from_overflowed_records(cuda, cases, band, on):
    from deftet_amd import hip_ops
    c = cases("overflow", band)
    n = c.refs[0]["n"]
    # the 9- and 40-hit tets take the ordered list scan: their records are marked.  The statistics count a tet as overflowed
    # ([6]) or, when it is flattened so far that the traversal treats it as irregular, as that ([0]) - at 1/100 all ten of them
    assert hip_ops.bwd_uses_records(c.T, c.Q) and (n > 6).sum() >= 10 and c.overflowed()[0][n > 6].all()
    assert c.stats[0, 6] + c.stats[0, 0] >= (n > 6).sum() and (c.stats[0, 6] > 0 or band[1] < 0.1)
    assert (n[c.shapes[0]["asserted"]] == 40).sum() == 2 and (n[c.shapes[0]["asserted"]] == 9).sum() >= 8
    c.hold("overflowed records", **_bwd(c, on, c.hits))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
@pytest.mark.parametrize("with_hits", [True, False], ids=["hits=", "no hits"])
@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_backward_from_per_tet_lists(cuda, cases, band, with_hits, on):
    from deftet_amd import hip_ops
    c = cases("lists", band)
    assert not hip_ops.bwd_uses_records(c.T, c.Q) and c.refs[0]["n"].max() == 40
    c.hold("lists, %s" % ("hits=" if with_hits else "no hits"), **_bwd(c, on, c.hits if with_hits else None))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_backward_float_atomic_fallback(cuda, cases, band, on):
    """deftet_point_in_tet_bwd_f32 without a workspace: every hit adds its 12 entries with float atomics"""
    from deftet_amd import _lib
    lib = _lib.load()
    c = cases("overflow", band)
    g_tet = torch.full_like(c.tet, 7.0)                              # overwritten: accumulate == 0
    g_pts = torch.full_like(c.pts, 7.0) if on else None
    g_pred = torch.full((c.B, c.T), 7.0, device=cuda) if on else None
    _lib.check(lib.deftet_point_in_tet_bwd_f32(_lib.ptr(c.tet), _lib.ptr(c.pts), _lib.ptr(c.cond), _lib.ptr(c.gw), _lib.ptr(g_tet),
                                               _lib.ptr(g_pts), _lib.ptr(c.go) if on else None, _lib.ptr(g_pred), None, c.B, c.T, c.Q, 0,
                                               None, 0, _lib.current_stream(cuda)), "bwd atomic")
    torch.cuda.synchronize()
    c.hold("float atomics", grad_tet=g_tet, grad_pts=g_pts, grad_pred=g_pred)


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
@pytest.mark.parametrize("kind", ["overflow", "lists", "pair"])
@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_backward_onto_the_vertices(cuda, cases, band, kind, on):
    """from the gathered tensor and from the index list; `pair`: two shapes, each with an index list of its own"""
    from deftet_amd import hip_ops
    c = cases(kind, band)
    pos, t_idx, idx, csr = _soup(c, cuda, per_shape=kind == "pair")
    assert hip_ops.bwd_uses_records(c.T, c.Q) == (kind != "lists")
    go = c.go if on else None
    names = ("grad_pos", "grad_pts", "grad_pred")
    out = hip_ops.point_in_tet_bwd_to_vertices(c.tet, c.pts, c.cond, c.gw, csr, 4 * c.T, want_grad_pts=on, grad_occ=go, hits=c.hits)
    assert len(out) == (3 if on else 2) and (out[1] is not None) == on
    c.hold("to vertices, gathered", idx=idx, **dict(zip(names, out)))
    fwd = hip_ops.point_in_tet_indexed(pos, t_idx, c.pts, want_bary=True, pred_bxt=c.pred, want_hits=True)
    assert torch.equal(fwd[0], c.cond) and torch.equal(fwd[1], c.w)
    out = hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, t_idx, c.pts, fwd[0], c.gw, csr, want_grad_pts=on, grad_occ=go, hits=fwd[3])
    c.hold("to vertices, indexed", idx=idx, **dict(zip(names, out)))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_backward_onto_the_vertices_accumulates_into_out(cuda, cases, band, on):
    from deftet_amd import hip_ops
    c = cases("overflow", band)
    pos, t_idx, idx, csr = _soup(c, cuda, per_shape=False)
    go = c.go if on else None
    base = torch.randn(c.B, 4 * c.T, 3, device=cuda, generator=torch.Generator(device=cuda).manual_seed(8))
    fresh = hip_ops.point_in_tet_bwd_to_vertices(c.tet, c.pts, c.cond, c.gw, csr, 4 * c.T, want_grad_pts=on, grad_occ=go, hits=c.hits)
    acc = hip_ops.point_in_tet_bwd_to_vertices(c.tet, c.pts, c.cond, c.gw, csr, 4 * c.T, want_grad_pts=on, grad_occ=go, hits=c.hits,
                                               out=base.clone())
    # base + the fresh result (bit-reproducible on the record path), one rounding apart
    both = _n(base).astype(np.float64) + _n(fresh[0]).astype(np.float64)
    check_bound("bary pin, %s, out= against base + fresh" % c.name, _n(acc[0]), both, C.U * np.abs(both))
    c.hold("to vertices, out=", idx=idx, base=base, **dict(zip(("grad_pos", "grad_pts", "grad_pred"), acc)))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
def test_backward_butterfly_for_a_tet_with_thousands_of_hits(cuda, cases, on):
    from deftet_amd import hip_ops
    c = cases("butterfly")
    r, s = c.refs[0], c.shapes[0]
    big = int(r["n"].argmax())
    assert c.T == 1728 and r["n"][big] == C.BUTTERFLY_HITS and s["asserted"][big] and np.sort(r["n"])[-2] <= 1
    assert hip_ops.bwd_uses_records(c.T, c.Q) and c.stats[0, 6] > 0 and c.overflowed()[0, big]
    assert C.BUTTERFLY_HITS * ((C.BUTTERFLY_HITS + 63) // 64) > 16384                   # past the ordered scan's budget
    c.hold("butterfly", **_bwd(c, on, c.hits))


@pytest.mark.parametrize("on", BOTH, ids=["pts+occ", "tet only"])
def test_backward_of_a_batch_that_mixes_bands(cuda, cases, on):
    c = cases("mixed")
    assert c.B == 3 and [(s["band"], s["flat"]) for s in c.shapes] == C.MIXED_BANDS
    c.hold("mixed batch, forward", w=c.w)
    c.hold("mixed batch, records", **_bwd(c, on, c.hits))
    c.hold("mixed batch, lists", **_bwd(c, on, None))


# ---- autograd ---------------------------------------------------------------------------------------------------------------

def test_autograd_operators_on_the_flattened_band(cuda, cases):
    from deftet_amd.layers.DefTet.check_condition_tetrahedron_base.utils import point_in_tet_bary
    from deftet_amd.layers.DefTet.deftet import DefTet
    c = cases("pair", ("unit", 0.01))
    # point_in_tet_bary: tet.grad and pts.grad
    t, p = c.tet.clone().requires_grad_(True), c.pts.clone().requires_grad_(True)
    cond, w = point_in_tet_bary(t, p)
    assert torch.equal(cond, c.cond) and torch.equal(w, c.w)
    (w * c.gw).sum().backward()
    c.hold("autograd point_in_tet_bary", grad_tet=t.grad, grad_pts=p.grad)
    # DefTet.occupancy_query, gathered and indexed: pos.grad, pts.grad and pred.grad
    pos, t_idx, idx, _ = _soup(c, cuda, per_shape=True)
    m = DefTet(device=cuda)
    for indexed in (False, True):
        x, p, pred = pos.clone().requires_grad_(True), c.pts.clone().requires_grad_(True), c.pred.clone().requires_grad_(True)
        cond, w, occ = m.occupancy_query(x, t_idx, p, pred, indexed=indexed)
        assert torch.equal(cond, c.cond) and torch.equal(w, c.w) and torch.equal(occ, c.occ)
        ((w * c.gw).sum() + (occ * c.go).sum()).backward()
        c.hold("autograd occupancy_query%s" % (", indexed" if indexed else ""), grad_pos=x.grad, grad_pts=p.grad, grad_pred=pred.grad, idx=idx)
