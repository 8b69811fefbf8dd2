"""Conforming selective refinement on the GPU (hip_ops.refine_tets, deftet_amd/csrc/tet_refine.hip) against the numpy
restatement tests/refine_ref.py: every integer and every float bit-equal, whatever the sweep schedule.  Nothing is compared
against the library itself except where the contract says so (every tet selected = hip_ops.subdivide)."""
import numpy as np
import pytest
import torch

from tests import builder_cases as B
from tests import marching_tets_ref as M
from tests import refine_cases as C
from tests import refine_ref as R

pytestmark = pytest.mark.gpu
FIELDS = ("points_new", "feat_new", "tet_new", "parent", "kind", "edges_split")
DTYPES = (np.float32, np.float32, np.int64, np.int64, np.uint8, np.int64)


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(cuda, x):
    return torch.from_numpy(np.array(x, order="C")).to(cuda)                     # (a copy: the shared inputs are read-only)


def run(cuda, tets, pts, feat, select, **kw):
    from deftet_amd import hip_ops
    return hip_ops.refine_tets(dev(cuda, np.asarray(tets, np.int64)), dev(cuda, pts), dev(cuda, feat), dev(cuda, np.asarray(select, bool)), **kw)


def check(got, want, what=""):
    for name, dtype in zip(FIELDS, DTYPES):
        g, w = getattr(got, name), np.asarray(getattr(want, name), dtype)
        assert same(g, w), "%s %s: %s %s against %s" % (what, name, tuple(g.shape), g.dtype, w.shape)


def test_empty_list(cuda):
    pts, feat = C.hand_points(4)
    got = run(cuda, np.zeros((0, 4), np.int64), pts, feat, np.zeros(0, bool))
    check(got, R.refine(np.zeros((0, 4), np.int64), pts, feat, np.zeros(0, bool)))
    assert got.tet_new.shape == (0, 4) and got.edges_split.shape == (0, 2) and same(got.points_new, pts) and same(got.feat_new, feat)


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_worked(cuda, name):
    h = C.HAND[name]
    pts, feat = C.hand_points(h["n_point"])
    got = run(cuda, h["tets"], pts, feat, h["select"])
    for key in ("tet_new", "parent", "kind", "edges_split"):
        assert same(getattr(got, key), h[key]), key
    check(got, R.refine(h["tets"], pts, feat, h["select"]), name)


def test_none_is_the_identity_and_all_is_subdivide(cuda):
    from deftet_amd import hip_ops
    tets, pts, _ = C.grid("kuhn8_jitter")
    feat = C.features(pts, 3)
    T = len(tets)
    got = run(cuda, tets, pts, feat, np.zeros(T, bool))
    assert same(got.tet_new, tets) and same(got.points_new, pts) and same(got.feat_new, feat)
    assert same(got.parent, np.arange(T)) and same(got.kind, np.zeros(T, np.uint8)) and got.edges_split.shape == (0, 2)
    got = run(cuda, tets, pts, feat, np.ones(T, bool))
    pn, fn, tn = hip_ops.subdivide(dev(cuda, tets), dev(cuda, pts), dev(cuda, feat), None)
    assert torch.equal(got.points_new, pn) and torch.equal(got.feat_new, fn) and torch.equal(got.tet_new, tn)
    assert got.points_new.dtype == pn.dtype and got.tet_new.dtype == tn.dtype and tn.shape[0] == 8 * T
    check(got, R.refine(tets, pts, feat, np.ones(T, bool)), "all")
    assert same(got.kind, np.full(8 * T, 6, np.uint8)) and same(got.parent, np.repeat(np.arange(T), 8))


@pytest.mark.parametrize("sel", C.SELECTIONS)
def test_res20_any_schedule(cuda, sel):
    """T = 6,000: past one workgroup and one scan block; one and four sweeps per read-back, and a second run, give the same bits"""
    from deftet_amd import hip_ops
    tets, pts, _ = C.grid("kuhn20_jitter")
    feat, select, want = C.features(pts, 2), C.selection("kuhn20_jitter", sel), C.reference("kuhn20_jitter", sel)
    first = run(cuda, tets, pts, feat, select)
    check(first, want, sel)
    for kw in (dict(sweeps_per_sync=1), dict(sweeps_per_sync=4), dict(sweeps_per_sync=64)):
        again = run(cuda, tets, pts, feat, select, **kw)
        for name in FIELDS:
            assert torch.equal(getattr(again, name), getattr(first, name)), (kw, name)
    # the marks themselves, and the count every sweep reports: every mark the closure adds is counted exactly once
    edges, tet_edge = R.tet_edges(tets, pts.shape[0])
    added = int(want.marks.sum() - R.initial_marks(tet_edge, select, len(edges)).sum())
    for S in (1, 4):
        marks, counts = hip_ops.refine_marks(dev(cuda, tet_edge), dev(cuda, select), len(edges), S)
        assert marks.dtype == torch.int32 and same(marks, want.marks.astype(np.int32))
        assert len(counts) % S == 0 and counts[-1] == 0 and sum(counts) == added and all(c >= 0 for c in counts)
        print("%s: sweeps_per_sync=%d counts=%s (the Jacobi restatement: %d rounds)" % (sel, S, counts, want.rounds))
        if S == 1:
            assert all(c > 0 for c in counts[:-1])                    # a sweep that sets nothing is the last
        if sel == "random" and S == 4:
            assert len(counts) > 4                                    # more sweeps than one read-back group


def test_cube40_band(cuda):
    tets, pts, _ = C.grid("cube40")
    assert tets.shape[0] == 47472
    check(run(cuda, tets, pts, C.features(pts, 2), C.selection("cube40", "band")), C.reference("cube40", "band"), "cube40")


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_irregular_lists(cuda, name):
    """many-owner faces, duplicate tets, repeated vertices, sparse ids up to the largest vertex count, sizes around the tiles of
    the sort and the scan; K = 0, 1 and 7 feature columns"""
    tets, n_point = B.case(name)
    T = len(tets)
    rng = np.random.default_rng(len(name) + T)
    pts = rng.random((n_point, 3), np.float32)
    K = (0, 1, 7)[sorted(B.CASES).index(name) % 3]
    for k in ((0, 1, 7) if name == "degenerate" else (K,)):
        feat = rng.random((n_point, k), np.float32)
        for select in (rng.random(T) < 0.3, np.ones(T, bool)):
            check(run(cuda, tets, pts, feat, select), R.refine(tets, pts, feat, select), "%s K=%d" % (name, k))


def test_precomputed_edges(cuda):
    from deftet_amd import hip_ops
    tets, pts, _ = C.grid("kuhn8")
    feat, select = C.features(pts, 2), C.selection("kuhn8", "random")
    edges, tet_edge = hip_ops.tet_edges(dev(cuda, tets), pts.shape[0])
    assert same(edges, R.tet_edges(tets, pts.shape[0])[0]) and same(tet_edge, R.tet_edges(tets, pts.shape[0])[1])
    got = run(cuda, tets, pts, feat, select, edges=edges, tet_edge=tet_edge)
    check(got, C.reference("kuhn8", "random"), "edges given")
    check(run(cuda, tets, pts, feat, select), C.reference("kuhn8", "random"), "edges computed")
    with pytest.raises(RuntimeError, match="come together"):
        run(cuda, tets, pts, feat, select, edges=edges)


def test_bad_input(cuda):
    from deftet_amd import _lib, hip_ops
    lib = _lib.load()
    tets, pts, _ = C.grid("kuhn8")
    feat, select = C.features(pts, 2), C.selection("kuhn8", "band")
    edges, tet_edge = R.tet_edges(tets, pts.shape[0])
    T, E, Pn = len(tets), len(edges), pts.shape[0]
    for value in (E, -1):
        bad = tet_edge.copy()
        bad[T // 2, 3] = value
        with pytest.raises(IndexError, match="tet_edge"):
            run(cuda, tets, pts, feat, select, edges=dev(cuda, edges), tet_edge=dev(cuda, bad))
    far = edges.copy()
    far[tet_edge[np.nonzero(select)[0][0], 0], 1] = Pn                 # an end of a marked edge outside the points
    with pytest.raises(RuntimeError, match="outside"):
        run(cuda, tets, pts, feat, select, edges=dev(cuda, far), tet_edge=dev(cuda, tet_edge))
    with pytest.raises(RuntimeError, match="select"):
        run(cuda, tets, pts, feat, select[:-1])
    with pytest.raises(RuntimeError, match="points"):
        run(cuda, tets, pts, feat[:-1], select)
    # the entry points themselves: a workspace one byte short, and marks that are not closed
    want = C.reference("kuhn8", "band")
    marks, totals = dev(cuda, want.marks.astype(np.int32)), torch.zeros(3, dtype=torch.int32, device=cuda)
    need = lib.deftet_tet_refine_workspace_bytes(T, E)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    args = (dev(cuda, tet_edge), dev(cuda, edges), marks, Pn, T, E, totals)
    with pytest.raises(_lib.DefTetHipError, match="workspace null, misaligned or too small: need %d bytes, got %d" % (need, need - 1)):
        _lib.call("deftet_tet_refine_count_i64", cuda, *args, ws=ws[:need - 1])
    _lib.call("deftet_tet_refine_count_i64", cuda, *args, ws=ws)
    assert totals.tolist() == [int(want.marks.sum()), len(want.tet_new), 0]
    open_marks = np.zeros(E, np.int32)
    open_marks[tet_edge[0, [0, 1]]] = 1                                # two edges of a face without the third
    _lib.call("deftet_tet_refine_count_i64", cuda, args[0], args[1], dev(cuda, open_marks), Pn, T, E, totals, ws=ws)
    assert totals.tolist()[2] == 1
    assert hip_ops.refine_marks(dev(cuda, tet_edge), dev(cuda, select), E)[1][-1] == 0


def test_downstream_operators_take_the_refinement(cuda):
    """what the closure is for, at res 20: the refined list has the hull faces of the input and nothing else without a partner,
    the occupancy surface on it is closed, and marching tets runs on it"""
    from deftet_amd import hip_ops
    name = "kuhn20_jitter"
    tets, pts, nbr = C.grid(name)
    select, want = C.selection(name, "band"), C.reference(name, "band")
    feat = C.features(pts, 2)
    got = run(cuda, tets, pts, feat, select)
    check(got, want, "band")
    Pn = int(got.points_new.shape[0])
    # face neighbours: -1 entries = the one-owner faces of the restatement; the reference's selective split has strictly more
    table = hip_ops.tet_neighbours(got.tet_new, Pn, cuda)
    n_open = int((table == -1).sum())
    assert n_open == len(R.one_owner_faces(want.tet_new)) == len(R.one_owner_faces(tets))         # (the band is interior: the hull is untouched)
    _pn, _fn, loose = hip_ops.subdivide(dev(cuda, tets), dev(cuda, pts), dev(cuda, feat), dev(cuda, select))
    assert int((hip_ops.tet_neighbours(loose, int(_pn.shape[0]), cuda) == -1).sum()) > n_open
    # the occupancy surface of the parents' occupancy: every welded edge has two faces
    inside = R.sphere_inside(pts, tets)
    occ = dev(cuda, inside[want.parent].astype(np.float32))[None]
    fnb = hip_ops.tet_face_neighbours(got.tet_new, Pn, cuda)
    soup = hip_ops.surface_extract(got.points_new[got.tet_new][None], occ, fnb, "binary", tet_idx=got.tet_new, return_faces=True)
    verts, _attr, faces, _old = hip_ops.surface_weld(got.points_new, soup.faces[0])
    closed, _oriented, _euler = M.closed_and_oriented(faces.cpu().numpy(), verts.shape[0])
    assert faces.shape[0] > 0 and closed
    assert faces.shape[0] == 4 * int((inside[:, None] & ~inside[np.where(nbr >= 0, nbr, 0)] & (nbr >= 0)).sum())   # every face of the band was split in four
    # marching tets on the refined list, the field interpolated through edges_split like the positions
    f = (0.3 - np.linalg.norm(pts.astype(np.float64), axis=1)).astype(np.float32)
    fn = np.concatenate([f, (f[want.edges_split[:, 0]] + f[want.edges_split[:, 1]]) / np.float32(2)])
    top = hip_ops.TetEdges(got.tet_new, Pn)
    mesh = hip_ops.marching_tets(got.points_new, dev(cuda, fn), top)
    ref = M.marching_tets(want.points_new, fn, want.tet_new)
    assert same(mesh.verts[0], ref.verts) and same(mesh.faces[0], ref.faces)
    assert M.closed_and_oriented(ref.faces, len(ref.verts)) == (True, True, 2)


def test_occupancy_band_on_the_device(cuda):
    from deftet_amd import hip_ops
    tets, pts, nbr = C.grid("kuhn20")
    inside = R.sphere_inside(pts, tets)
    fnb = hip_ops.tet_face_neighbours(dev(cuda, tets), pts.shape[0], cuda)
    for rings in (0, 1):
        got = hip_ops.occupancy_band(dev(cuda, inside), fnb, rings)
        assert got.is_cuda and same(got, R.occupancy_band(inside, R.neighbour_table(tets), rings))
        assert same(hip_ops.occupancy_band(dev(cuda, np.stack([inside, ~inside])), fnb.table, rings), R.occupancy_band(inside, nbr, rings))


def test_ported_wrapper_round_trips_numpy(cuda):
    from deftet_amd.render import prepare_for_wz
    tets, pts, _ = C.grid("kuhn8_jitter")
    feat, select = C.features(pts, 2), C.selection("kuhn8_jitter", "band")
    want = R.refine(tets, pts, feat, select)
    pn, fn, tn = prepare_for_wz.generate_conforming_subdivision(tets.astype(np.int32), np.array(pts), feat, select)
    assert all(isinstance(x, np.ndarray) for x in (pn, fn, tn))
    assert same(pn, want.points_new) and same(fn, want.feat_new) and same(tn, want.tet_new)
    pn, fn, tn = prepare_for_wz.generate_conforming_subdivision(dev(cuda, tets), dev(cuda, pts), dev(cuda, feat), dev(cuda, select))
    assert pn.is_cuda and same(pn, want.points_new) and same(fn, want.feat_new) and same(tn, want.tet_new)
