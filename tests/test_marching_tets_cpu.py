"""Marching tetrahedra without a GPU: the triangle table of the numpy restatement (tests/marching_tets_ref.py) is geometrically
right on every mixed code; the restatement's mesh of a sphere on a jittered Kuhn grid is closed, consistently oriented and of
genus 0; its float32 vertices and gradients stay inside the bound the GPU test asserts against float64; the per-entry
reference, bounds and inputs of the GPU test hold their own conditions (the closed formulas equal autograd, a double rounded once
is inside the bound and a float32 accumulation far outside it, the gap spread, the level rule, the hostile cap); the library exports
the entry points and rejects bad arguments with DEFTET_EINVAL and a message before any device work; the Python front ends
refuse CPU tensors."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import marching_tets_cases as K
from tests import marching_tets_ref as R
from tests.tol import check_bound, check_close

EINVAL = -1
SYMBOLS = ("deftet_edge_vertex_csr_workspace_bytes", "deftet_edge_vertex_csr_i32", "deftet_marching_tets_workspace_bytes",
           "deftet_marching_tets_count_f32", "deftet_marching_tets_fill_f32", "deftet_marching_tets_bwd_f32")
MAXNORM = 1e-5                                               # the project's bound; the GPU test asserts the same


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ table
POS_TET = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)


def _triangles(code):
    q = R.TRIANGLES[code]
    return [q[:3]] + ([(q[0], q[2], q[3])] if len(q) == 4 else [])


def test_table_geometry_on_a_positive_tet():
    a, b, c, d = POS_TET
    assert np.dot(np.cross(b - a, c - a), d - a) > 0
    assert R.TRIANGLES[0] == () and R.TRIANGLES[15] == ()
    mid = np.array([(POS_TET[i] + POS_TET[j]) / 2 for i, j in R.LOCAL_EDGES])
    for code in range(1, 15):
        ins = np.array([(code >> k) & 1 for k in range(4)], bool)
        crossing = {e for e, (i, j) in enumerate(R.LOCAL_EDGES) if ins[i] != ins[j]}
        q = R.TRIANGLES[code]
        assert set(q) == crossing and len(q) == len(crossing) and q[0] == min(crossing), code
        assert len(q) == (4 if ins.sum() == 2 else 3), code
        out_dir = POS_TET[~ins].mean(0) - POS_TET[ins].mean(0)
        for tri in _triangles(code):
            v0, v1, v2 = mid[list(tri)]
            assert np.dot(np.cross(v1 - v0, v2 - v0), out_dir) > 0, (code, tri)
        # the complementary code: the same edges, the other direction from the same start
        qc = R.TRIANGLES[15 - code]
        assert qc == (q[0],) + tuple(reversed(q[1:])), code
        if len(q) == 4:
            t0, t1 = _triangles(code)
            assert set(t0) & set(t1) == {q[0], q[2]}                                  # two triangles sharing the diagonal q0-q2
            # q0..q3 is a cycle of the quad: consecutive crossing edges share a tet corner, opposite ones do not
            for k in range(4):
                assert set(R.LOCAL_EDGES[q[k]]) & set(R.LOCAL_EDGES[q[(k + 1) % 4]]), code
            assert not set(R.LOCAL_EDGES[q[0]]) & set(R.LOCAL_EDGES[q[2]]), code


def test_restatement_lists_equal_the_definitions():
    _pos, tets, edges, tet_edge = K.grid(4, 1)
    assert (edges[:, 0] < edges[:, 1]).all()
    key = edges[:, 0] * 1000 + edges[:, 1]
    assert (np.diff(key) > 0).all()                                                    # unique, lexicographic
    for k, (i, j) in enumerate(R.LOCAL_EDGES):
        want = np.stack([np.minimum(tets[:, i], tets[:, j]), np.maximum(tets[:, i], tets[:, j])], 1)
        assert (edges[tet_edge[:, k]] == want).all()
    V = int(tets.max()) + 1
    offsets, slots = R.edge_vertex_csr(edges, V)
    assert offsets[0] == 0 and offsets[-1] == 2 * edges.shape[0]
    for v in range(V):
        row = slots[offsets[v]:offsets[v + 1]]
        assert (np.diff(row) > 0).all() and (edges.reshape(-1)[row] == v).all()


# ------------------------------------------------------------------------------------------------------------ mesh
@pytest.fixture(scope="module")
def sphere8():
    pos, tets, edges, tet_edge = K.grid(8, 1)
    field = K.sphere(pos[0], 0.3)
    return pos[0], field, tets, edges, tet_edge


def test_sphere_mesh_is_closed_oriented_and_of_genus_zero(sphere8):
    pos, field, tets, edges, tet_edge = sphere8
    assert (grids_orientation(pos, tets) > 0).all()                                   # the grid convention: positive tets
    m = R.marching_tets(pos, field, tets, 0.0, edges=edges, tet_edge=tet_edge)
    assert m.verts.shape[0] > 20 and m.faces.shape[0] > 40
    assert m.faces.min() == 0 and m.faces.max() == m.verts.shape[0] - 1
    two, once, euler = R.closed_and_oriented(m.faces, m.verts.shape[0])
    assert two and once and euler == 2
    assert R.signed_volume(m.verts, m.faces) > 0
    assert (m.t >= 0).all() and (m.t <= 1).all()
    assert (np.diff(m.edge_id) > 0).all() and (np.diff(m.tet_id) >= 0).all()


def grids_orientation(pos, tets):
    from deftet_amd import grids
    return grids.tet_orientation(pos[tets][None])[0]


def test_float32_restatement_stays_inside_the_gpu_bound(sphere8):
    """What the GPU test asserts of the kernels (check_close, maxnorm 1e-5 against float64) holds for plain float32 arithmetic on
    the same input: vertices, and the three gradients for N(0,1) output gradients."""
    pos, field, tets, edges, tet_edge = sphere8
    assert K.crossing_gap(field, edges) > K.GAP
    attr = K.attrs(1, pos.shape[0], 3, 7)[0]
    m = R.marching_tets(pos, field, tets, 0.0, attr=attr, edges=edges, tet_edge=tet_edge)
    v64, a64 = R.marching_tets_torch(torch.tensor(pos).double(), torch.tensor(field).double(), edges, 0.0,
                                     torch.tensor(attr).double())
    check_close("verts f32 vs f64", m.verts, v64, MAXNORM)
    check_close("vert_attr f32 vs f64", m.vert_attr, a64, MAXNORM)
    rng = np.random.default_rng(11)
    gv, ga = rng.normal(size=m.verts.shape).astype(np.float32), rng.normal(size=m.vert_attr.shape).astype(np.float32)
    got = R.grads32(pos, field, edges, 0.0, gv, attr, ga)
    want = R.grads64(pos, field, edges, 0.0, gv, attr, ga)
    for name, g, w in zip(("grad_pos", "grad_field", "grad_attr"), got, want):
        assert np.abs(w).max() > 0
        check_close(name + " f32 vs f64", g, w, MAXNORM)
    untouched = np.ones(pos.shape[0], bool)
    untouched[edges[m.edge_id].reshape(-1)] = False
    assert untouched.any() and not got[0][untouched].any() and not got[1][untouched].any() and not want[1][untouched].any()


# ------------------------------------------------------------------------------------------------------------ per entry
# What the GPU test asserts entry by entry ("What is pinned"), validated here without a GPU: the reference, the
# bounds and the inputs' conditions.
BACKWARD = [(name, C) for name, widths in K.PER_ENTRY.items() for C in widths]
GRADS = ("grad_pos", "grad_field", "grad_attr")


def _shapes(name, C):
    """per shape of a named input: (pos, field, edges, iso, g_verts, attr | None, g_attr | None)"""
    pos, field, _tets, edges, _te, iso = K.per_entry_case(name)
    attr, gv, ga = K.per_entry_gradients(name, C)
    for b in range(field.shape[0]):
        yield pos[b], field[b], edges, iso, gv[b], None if attr is None else attr[b], None if ga is None else ga[b]


def _worst(got, want, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(np.asarray(got, np.float64) - want) / bound
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("name,C", BACKWARD, ids=lambda x: str(x))
def test_explicit_terms_equal_autograd_and_round_once_inside_the_bound(name, C):
    """grads64_terms (closed formulas) against grads64 (autograd): 1e-12 of the largest entry asserted, 4e-16 at the worst measured;
    and the float64 gradients rounded ONCE to float32 satisfy the per-entry bound the GPU test asserts (worst ratio 0.9996)."""
    for b, args in enumerate(_shapes(name, C)):
        terms, S = R.grads64_terms(*args)
        auto = R.grads64(*args)
        for g, w, a, s in zip(GRADS, terms, auto, S):
            if w is None:
                assert a is None and C == 0
                continue
            assert (s >= np.abs(w) * (1 - 1e-12)).all()                                  # the triangle inequality: S is an absolute sum
            assert np.abs(w - a).max() <= 1e-12 * max(np.abs(a).max(), 1e-300), (g, b)
            check_bound("%s %s C=%d [%d] rounded once" % (name, g, C, b), w.astype(np.float32), w, R.entry_bound(w, s))


@pytest.mark.parametrize("name", K.THIN)
def test_float32_accumulation_breaks_the_per_entry_bound_on_thin_fields(name):
    """The bound tells a double accumulation from a float one: grads32 — the backward's formulas in float32 — misses it by a
    factor above 10 (asserted) for every gradient of every thin shape; measured: grad_pos 2.3e2 to 7.6e7, grad_field 18 to 8.2e3,
    grad_attr 5.7e2 to 2.0e6."""
    for b, args in enumerate(_shapes(name, 3)):
        terms, S = R.grads64_terms(*args)
        got = R.grads32(*args)
        for g, x, w, s in zip(GRADS, got, terms, S):
            worst = _worst(x, w, R.entry_bound(w, s))
            print("%s[%d] %s: float32 error over bound %.3g" % (name, b, g, worst))
            assert worst > 10, (g, b, worst)
        check_close("%s[%d] grad_field f32, max-norm" % (name, b), got[1], terms[1], MAXNORM)   # ... which the max-norm cannot see


@pytest.mark.parametrize("name", K.FORWARD)
def test_float32_restatement_stays_inside_the_forward_bounds(name):
    """t within 4u |t64| and verts, vert_attr within 6u (|x_min| + |x_max|) of the float64 evaluation of the same float32 inputs
    (u = 2^-24; the derivation is R.forward64's).  Measured on these inputs: t 0.57 of its bound at the worst, verts 0.48,
    vert_attr 0.35."""
    pos, field, tets, edges, tet_edge, iso = K.per_entry_case(name)
    attr = K.attrs(field.shape[0], field.shape[1], 3, 40)
    for b in range(field.shape[0]):
        m = R.marching_tets(pos[b], field[b], tets, iso, attr=attr[b], edges=edges, tet_edge=tet_edge)
        assert m.t.size > 20 and (m.t >= 0).all() and (m.t <= 1).all()
        (t, bt), (v, bv), (a, ba) = R.forward64(pos[b], field[b], edges, iso, attr[b])
        check_bound("%s[%d] t f32 vs f64" % (name, b), m.t, t, bt)
        check_bound("%s[%d] verts f32 vs f64" % (name, b), m.verts, v, bv)
        check_bound("%s[%d] vert_attr f32 vs f64" % (name, b), m.vert_attr, a, ba)


def test_level_rule_at_a_level_that_is_no_float32_number():
    """iso = 0.1 means float32(0.1): that value and the float32 below it are outside, the one above is inside, and an edge with
    an end on the level has t exactly 0 (the lower id on it) or 1 (the higher id on it)"""
    pos, field, tets, edges, tet_edge, iso = K.per_entry_case("level8@0.1")
    at = np.float32(0.1)
    assert iso == 0.1 and float(at) != 0.1
    for b in range(field.shape[0]):
        f = field[b]
        assert set(np.unique(f)) == {np.nextafter(at, np.float32(-1)), at, np.nextafter(at, np.float32(1))}
        m = R.marching_tets(pos[b], f, tets, iso, edges=edges, tet_edge=tet_edge)
        lo, hi = edges[m.edge_id, 0], edges[m.edge_id, 1]
        assert ((f[lo] > at) != (f[hi] > at)).all() and ((f[lo] > at) | (f[hi] > at)).all()      # exactly one end ABOVE the level
        uncrossed = np.setdiff1d(np.arange(edges.shape[0]), m.edge_id)
        assert ((f[edges[uncrossed, 0]] > at) == (f[edges[uncrossed, 1]] > at)).all()
        on_lo, on_hi = f[lo] == at, f[hi] == at
        assert on_lo.sum() > 5 and on_hi.sum() > 5 and (m.t[on_lo] == 0).all() and (m.t[on_hi] == 1).all()
        assert np.isin(m.t, (0, 0.5, 1)).all() and (m.t == 0.5).any()                             # gaps of one and two ulps: exact


def test_conditions_of_the_generated_inputs():
    """the gap spread of the thin fields, the gaps of the plain spheres (under GAP: not picked), the shifted fields' topology,
    every attribute width, and the cap on what the hostile field affects"""
    assert set(K.WIDTHS) == set(range(9)) and all(K.PER_ENTRY[n] == K.WIDTHS for n in K.THIN if n.startswith("thin8"))
    for name in K.THIN:
        _pos, field, _tets, edges, _te, iso = K.per_entry_case(name)
        for f in field:
            K.assert_thin(f, edges, iso)                                                 # (per_entry_case asserts it too)
            share = K.crossing_gaps(f, edges, iso) / (f.max() - f.min())
            assert share.size > 250 and np.log10(share.max() / share.min()) > 4.5
    _pos, field, _tets, edges, _te, _iso = K.per_entry_case("spheres20")
    assert [round(100 * K.crossing_gap(f, edges), 2) for f in field] == [0.48, 0.27]
    assert K.crossing_gap(K.per_entry_case("subdivided8")[1][0], K.per_entry_case("subdivided8")[3]) < K.GAP
    for name in ("spheres20", "subdivided8"):
        a, b = K.per_entry_case(name), K.per_entry_case(name + "+0.25")
        assert a[5] == 0.0 and b[5] == 0.25 and ((a[1] > 0) == (b[1] > np.float32(0.25))).all()
    # hostile: six vertices, no two joined, every kind twice; what they affect is under 10 % of the vertices with a crossing edge
    pos, field, _tets, edges, _te, iso = K.per_entry_case("hostile20")
    bad = np.nonzero(~np.isfinite(field[0]))[0]
    assert bad.size == 6 and np.isfinite(field[1]).all()
    assert sorted(map(str, field[0][bad])) == sorted(map(str, np.float32(K.HOSTILE)))
    assert not (np.isin(edges[:, 0], bad) & np.isin(edges[:, 1], bad)).any()
    assert (np.bincount(edges.reshape(-1))[bad] == 14).all()
    _f, bad_edge, bad_vertex = K.hostile(K.banded(field.shape[1], 170), 171)
    assert R.same_rows_nan_aware(_f, field[0])
    inside = field[0] > 0
    cross = inside[edges[:, 0]] != inside[edges[:, 1]]
    touched = np.zeros(field.shape[1], bool)
    touched[edges[cross].reshape(-1)] = True
    assert 6 < bad_vertex.sum() <= 90 and bad_vertex.sum() <= 0.1 * touched.sum() and not (bad_vertex & ~touched).any()
    assert bad_edge.sum() >= 6 and (bad_edge <= cross).all()
    # NaN and -inf are outside, +inf is inside
    assert [bool(x) for x in np.float32(K.HOSTILE) > 0] == [False, True, False, False, True, False]


def test_hostile_rows_of_the_restatement_are_what_the_rule_gives():
    """t = (iso - f_min) / (f_max - f_min) in float32 IEEE is not symmetric in the two ends: +-inf at the HIGHER vertex id gives
    t = +-0 and the vertex p_min; +-inf at the lower id, and NaN at either end, give NaN.  The fp64 terms without the affected edges
    are finite at every unaffected vertex, and every affected edge puts a NaN into grad_field at one of its ends at least."""
    pos, field, tets, edges, tet_edge, iso = K.per_entry_case("hostile20")
    _f, bad_edge, bad_vertex = K.hostile(K.banded(field.shape[1], 170), 171)
    f = field[0]
    m = R.marching_tets(pos[0], f, tets, iso, edges=edges, tet_edge=tet_edge)
    lo, hi = edges[m.edge_id, 0], edges[m.edge_id, 1]
    assert np.isfinite(m.t[~bad_edge[m.edge_id]]).all() and np.isfinite(m.verts[~bad_edge[m.edge_id]]).all()
    inf_hi = np.isinf(f[hi])
    assert inf_hi.any() and (m.t[inf_hi] == 0).all() and (np.abs(m.verts[inf_hi]) == np.abs(pos[0][lo[inf_hi]])).all()
    rest = bad_edge[m.edge_id] & ~inf_hi
    assert rest.any() and np.isnan(m.t[rest]).all() and np.isnan(m.verts[rest]).all()
    assert np.isinf(f[lo[rest]]).any() and np.isnan(f[lo[rest]]).any() and np.isnan(f[hi[rest]]).any()
    attr, gv, ga = K.per_entry_gradients("hostile20", 3)
    with np.errstate(all="ignore"):
        dirty, _S = R.grads64_terms(pos[0], f, edges, iso, gv[0], attr[0], ga[0])
    # grad_field: (iso - f_other) / d^2 is NaN at the FINITE end of an edge with an infinite one (inf / inf) and 0 at the infinite end;
    # a NaN end makes both NaN.  Every affected edge therefore leaves a NaN in grad_field at one of its ends at least.
    bl, bh = lo[bad_edge[m.edge_id]], hi[bad_edge[m.edge_id]]
    assert (np.isnan(dirty[1][bl]) | np.isnan(dirty[1][bh])).all()
    assert np.isnan(dirty[1][bl[np.isinf(f[bh])]]).all() and np.isnan(dirty[1][bh[np.isinf(f[bl])]]).all()
    assert np.isnan(dirty[1][bl[np.isnan(f[bh])]]).all() and np.isnan(dirty[1][bh[np.isnan(f[bl])]]).all()
    terms, S = R.grads64_terms(pos[0], f, edges, iso, gv[0], attr[0], ga[0], skip=bad_edge)
    for w, s, d in zip(terms, S, dirty):
        assert np.isfinite(w).all() and np.isfinite(s).all()
        assert (w[~bad_vertex] == d[~bad_vertex]).all()                                  # leaving the edges out changes nothing there


# ------------------------------------------------------------------------------------------------------------ library
def test_library_exports_the_entry_points(lib):
    raw = ctypes.CDLL(importlib.import_module("deftet_amd._lib").LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    assert lib.deftet_version() >= 320
    assert lib.deftet_marching_tets_workspace_bytes(8, 257250, 310000) > 8 * (257250 + 310000) * 4
    assert lib.deftet_marching_tets_workspace_bytes(1, 1, 6) > 0
    assert lib.deftet_edge_vertex_csr_workspace_bytes(46656, 310000) > 2 * 310000 * 4


def _buf(nbytes, align=256, offset=0):
    raw = ctypes.create_string_buffer(nbytes + align * 2)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + align - 1) // align * align + offset)


def _count(lib, B=2, V=9, T=8, E=30, iso=0.0, null=None, wsb=None, ws_off=0):
    bufs = dict(field=_buf(4 * 2 * 9), edges=_buf(8 * 30), tets=_buf(16 * 8), ev=_buf(4 * 2 * 30), offs=_buf(4 * 6), ws=_buf(1 << 16, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    need = lib.deftet_marching_tets_workspace_bytes(2, 8, 30)
    return lib.deftet_marching_tets_count_f32(a["field"], a["edges"], a["tets"], B, V, T, E, iso, a["ev"], a["offs"], a["ws"],
                                              need if wsb is None else wsb, None)


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-2), dict(T=0), dict(T=-1), dict(E=0), dict(V=0), dict(V=-5), dict(null="field"),
                                 dict(null="edges"), dict(null="tets"), dict(null="ev"), dict(null="offs"), dict(null="ws"), dict(wsb=64),
                                 dict(ws_off=64), dict(iso=float("nan")), dict(iso=float("inf")), dict(iso=-float("inf")),
                                 dict(B=40000, E=60000, wsb=1 << 40), dict(B=40000, T=60000, wsb=1 << 40)], ids=str)
def test_count_rejects_bad_arguments(lib, bad):
    assert _count(lib, **bad) == EINVAL
    assert lib.deftet_last_error()


def _fill(lib, B=2, V=9, T=8, E=30, C=3, iso=0.0, null=None, wsb=None, ws_off=0, nv=4, nf=4, attr=True):
    bufs = dict(pos=_buf(12 * 18), field=_buf(4 * 18), attr=_buf(4 * 18 * 8), edges=_buf(8 * 30), tets=_buf(16 * 8), te=_buf(24 * 8),
                ev=_buf(4 * 60), verts=_buf(48), vattr=_buf(4 * 4 * 8), faces=_buf(96), eid=_buf(32), t=_buf(16), tid=_buf(32),
                ws=_buf(1 << 16, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    need = lib.deftet_marching_tets_workspace_bytes(2, 8, 30)
    return lib.deftet_marching_tets_fill_f32(a["pos"], a["field"], a["attr"] if attr else None, C, a["edges"], a["tets"], a["te"], a["ev"], B, V,
                                             T, E, iso, nv, nf, a["verts"], a["vattr"] if attr else None, a["faces"], a["eid"], a["t"],
                                             a["tid"], a["ws"], need if wsb is None else wsb, None)


@pytest.mark.parametrize("bad", [dict(B=0), dict(T=0), dict(E=-1), dict(V=0), dict(C=9), dict(C=-1), dict(C=0), dict(attr=False, C=3),
                                 dict(null="pos"), dict(null="field"), dict(null="attr"), dict(null="edges"), dict(null="tets"),
                                 dict(null="te"), dict(null="ev"), dict(null="verts"), dict(null="vattr"), dict(null="faces"),
                                 dict(null="ws"), dict(wsb=16), dict(ws_off=128), dict(nv=-1), dict(nf=-1), dict(iso=float("nan")),
                                 dict(iso=float("inf")), dict(B=40000, E=60000, wsb=1 << 40), dict(B=40000, T=60000, wsb=1 << 40)],
                         ids=str)
def test_fill_rejects_bad_arguments(lib, bad):
    assert _fill(lib, **bad) == EINVAL
    assert lib.deftet_last_error()


def test_csr_and_backward_reject_bad_arguments(lib):
    e, off, sl, bad, ws = (_buf(1 << 12) for _ in range(5))
    need = lib.deftet_edge_vertex_csr_workspace_bytes(9, 30)
    csr = lib.deftet_edge_vertex_csr_i32
    assert csr(e[1], off[1], sl[1], bad[1], 0, 30, ws[1], need, None) == EINVAL
    assert csr(e[1], off[1], sl[1], bad[1], 9, 0, ws[1], need, None) == EINVAL
    assert csr(None, off[1], sl[1], bad[1], 9, 30, ws[1], need, None) == EINVAL and b"null" in lib.deftet_last_error()
    assert csr(e[1], None, sl[1], bad[1], 9, 30, ws[1], need, None) == EINVAL
    assert csr(e[1], off[1], sl[1], None, 9, 30, ws[1], need, None) == EINVAL
    gv, ga, pos, f, at, ed, co, cs, ev, of, gp, gf, gat = (_buf(1 << 12) for _ in range(13))
    ok = [gv[1], ga[1], 4, pos[1], f[1], at[1], 3, ed[1], co[1], cs[1], ev[1], of[1], 2, 9, 30, 0.0, gp[1], gf[1], gat[1], None]
    names = ["gv", "ga", "nv", "pos", "f", "attr", "C", "edges", "co", "cs", "ev", "of", "B", "V", "E", "iso", "gp", "gf", "gat", "st"]

    def call(**kw):
        args = list(ok)
        for k, val in kw.items():
            args[names.index(k)] = val
        return lib.deftet_marching_tets_bwd_f32(*args)
    for kw in (dict(B=0), dict(V=0), dict(E=0), dict(C=9), dict(C=0), dict(attr=None), dict(nv=-1), dict(gv=None, ga=None), dict(pos=None),
               dict(f=None), dict(edges=None), dict(co=None), dict(cs=None), dict(ev=None), dict(of=None), dict(gp=None, gf=None, gat=None),
               dict(iso=float("nan")), dict(iso=float("inf")), dict(B=70000), dict(C=0, attr=None, gat=None)):
        assert call(**kw) == EINVAL, kw
        assert lib.deftet_last_error()


def test_front_ends_refuse_cpu_tensors():
    from deftet_amd import hip_ops
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.render import export, marching_tets as model_marching_tets         # noqa: F401  (imports on a CPU-only host)
    pos, tets, _edges, _te = K.grid(2, 1)
    V = pos.shape[1]
    p, f = torch.from_numpy(pos.copy()), torch.zeros(1, V)
    with pytest.raises(DefTetHipError):
        hip_ops.TetEdges(torch.from_numpy(tets.copy()), V)
    with pytest.raises(DefTetHipError):
        hip_ops.marching_tets(p, f, None)
    with pytest.raises(DefTetHipError):
        hip_ops.marching_tets(p[0], f, None, iso=0.5, attr=torch.zeros(1, V, 3), return_index=True)
    for C in (0, 9):
        with pytest.raises(DefTetHipError, match="1 <= C <= 8"):
            hip_ops.marching_tets(p, f, None, attr=torch.zeros(1, V, C))
    with pytest.raises(DefTetHipError):
        export.save_surface_objs(p[0], (f.reshape(-1, 1), p[0]), tets, hip_ops.TetFaceNeighbours(torch.zeros(tets.shape[0], 4).long(),
                                                                                                   torch.zeros(tets.shape[0], 4).int()),
                                 "/nonexistent", "x", iso=0.25)
    assert hasattr(hip_ops.IsoMesh, "_fields") and hip_ops.IsoMesh._fields == ("verts", "faces", "vert_attr", "edge_id", "t", "tet_id")
