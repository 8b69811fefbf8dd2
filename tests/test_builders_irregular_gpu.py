"""GPU tests of the adjacency / face-table builders (deftet_amd/csrc/builders.hip) on the irregular meshes of
tests/builder_cases.py: faces with more than two owners, duplicate tets, repeated vertices (where the two face-key functions
differ and a tet can own both sides of a face), n_point = 2,097,151 (face keys on all 63 sorted bits), sizes on both sides of the
sort-tile and one-workgroup-scan limits, and a face-adjacency output larger than the reference's 4*T*50 buffer.  Integer work:
every comparison is exact, row order included — against the oracle, against what the reference's native builders returned
(tests/golden/ref_native_builders_irregular.npz), against its Python twins on the families without repeated vertices
(tests/golden/builders_irregular.npz) and against rows worked out by hand for the tiny families."""
import functools

import numpy as np
import pytest
import torch

from tests import builder_cases as BC
from tests.test_builders_irregular_cpu import check_against_hand, check_against_twins, native_fixture, twin_fixture
from tests.test_cpu_oracle_golden import lexsorted

pytestmark = pytest.mark.gpu
ALL = list(BC.CASES)
SENTINEL = -77


def np_(x):
    return tuple(np_(y) for y in x) if isinstance(x, tuple) else (x.cpu().numpy() if torch.is_tensor(x) else x)


@functools.lru_cache(maxsize=None)
def mesh(name):
    return native_fixture(name)[:2] if name in BC.REF_NATIVE else BC.case(name)


@pytest.mark.parametrize("name", ALL)
def test_native_builders_on_irregular_meshes(cuda, oracle, name):
    """tet_adj_share, tet_face_adj (both key widths) and tet_point_adj: the oracle's rows in the oracle's order, the reference's
    native rows where they were recorded, and the same bits on a second call"""
    from deftet_amd import hip_ops
    tets, n_point = mesh(name)
    want = native_fixture(name)[2] if name in BC.REF_NATIVE else None
    share = np_(hip_ops.tet_adj_share(tets, n_point, cuda))
    assert share.dtype == np.int32 and share.shape[1:] == (3,)
    assert np.array_equal(share, oracle.tet_adj_share(tets, n_point))
    fa = {w: np_(hip_ops.tet_face_adj(tets, n_point, cuda, wrap32=w)) for w in (True, False)}
    for w in (True, False):
        assert fa[w].dtype == np.int32 and fa[w].shape[1:] == (2,)
        assert np.array_equal(fa[w], oracle.tet_face_adj(tets, n_point, wrap32=w)), w
    pa = np_(hip_ops.tet_point_adj(tets, n_point, cuda))
    assert pa.dtype == np.int32 and pa.shape[1:] == (2,)
    assert np.array_equal(pa, oracle.tet_point_adj(tets, n_point))
    if want is not None:
        assert np.array_equal(share, want["adj_share"]) and np.array_equal(fa[True], want["face_adj"])
        assert np.array_equal(pa, lexsorted(want["point_adj"]))
        if oracle.RefBuilders.available():                   # the live native libraries, where they are built
            ref = oracle.RefBuilders()
            assert np.array_equal(share, ref.tet_adj_share(tets, n_point)) and np.array_equal(fa[True], ref.tet_face_adj(tets, n_point))
            assert np.array_equal(pa, lexsorted(ref.tet_point_adj(tets, n_point)))
    assert np.array_equal(np_(hip_ops.tet_adj_share(tets, n_point, cuda)), share)
    assert np.array_equal(np_(hip_ops.tet_face_adj(tets, n_point, cuda, wrap32=True)), fa[True])
    assert np.array_equal(np_(hip_ops.tet_face_adj(tets, n_point, cuda, wrap32=False)), fa[False])
    assert np.array_equal(np_(hip_ops.tet_point_adj(tets, n_point, cuda)), pa)


@pytest.mark.parametrize("name", ALL)
def test_tet_to_face_on_irregular_meshes(cuda, oracle, name):
    """all four tables and all three counts (interior or listed faces, boundary faces, many-owner face keys) equal the oracle with
    and without the boundary inline; every tet-face is accounted for: 2 * interior + boundary + owners of many-owner keys = 4T"""
    from deftet_amd import hip_ops
    tets, n_point = mesh(name)
    T = tets.shape[0]
    n_keys, n_owned = BC.many_owner_faces(tets, n_point)
    if name in ("three_on_face", "dup", "degenerate", "collapsed8", "collapsed8_dups", "soup40_200", "soup60_513", "n1", "fan_dense12"):
        assert n_keys > 0
    for wb in (False, True):
        got = np_(hip_ops.tet_to_face(tets, n_point, cuda, with_boundary=wb))
        want = oracle.tet_to_face(tets, n_point, with_boundary=wb)
        for a, b in zip(got[:4], want[:4]):
            assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), wb
        assert got[4] == want[4] == n_keys
        n_interior = got[0].shape[0] - (got[3].shape[0] if wb else 0)
        assert 2 * n_interior + got[3].shape[0] + n_owned == 4 * T


@pytest.mark.parametrize("name", ALL)
def test_tet_neighbours_on_irregular_meshes(cuda, oracle, name):
    """ValueError exactly when a face key has more than two owners; otherwise the neighbour table and the face-owner table of the
    oracle (on `self_owned` tet 1 lists itself twice in succession)"""
    from deftet_amd import hip_ops
    tets, n_point = mesh(name)
    n_multi = oracle.tet_to_face(tets, n_point, with_boundary=True)[4]
    if n_multi > 0:
        with pytest.raises(ValueError):
            hip_ops.tet_neighbours(tets, n_point, cuda, want_face_owners=True)
        with pytest.raises(ValueError):
            hip_ops.tet_neighbours(tets, n_point, cuda)
        return
    nbr, owners = np_(hip_ops.tet_neighbours(tets, n_point, cuda, want_face_owners=True))
    wn, wo = oracle.tet_neighbours(tets, n_point)
    assert nbr.dtype == np.int64 and nbr.shape == wn.shape and np.array_equal(nbr, wn)
    assert owners.dtype == np.int64 and owners.shape == wo.shape and np.array_equal(owners, wo)
    assert np.array_equal(np_(hip_ops.tet_neighbours(tets, n_point, cuda)), wn)
    if name == "self_owned":
        assert nbr[1].tolist() == [1, 1, -1, -1]


def _library(cuda, tets, n_point):
    """the callables check_against_twins / check_against_hand take, on the library"""
    from deftet_amd import hip_ops
    td = torch.from_numpy(tets.astype(np.int64)).to(cuda)
    return dict(adj_share=lambda: np_(hip_ops.tet_adj_share(tets, n_point, cuda)),
                to_face=lambda: np_(hip_ops.tet_to_face(tets, n_point, cuda)),
                to_face_wb=lambda: np_(hip_ops.tet_to_face(tets, n_point, cuda, with_boundary=True)),
                neighbours=lambda: np_(hip_ops.tet_neighbours(tets, n_point, cuda, want_face_owners=True)),
                edges_fn=lambda: np_(hip_ops.tet_edges(td, n_point)),
                point_adj_idx_fn=lambda: np_(hip_ops.point_adj_idx(n_point, td)))


@pytest.mark.parametrize("name", BC.NON_DEGENERATE)
def test_builders_match_python_twins_on_irregular_meshes(cuda, name):
    tets, n_point, G = twin_fixture(name)
    check_against_twins(name, G, **_library(cuda, tets, n_point))


@pytest.mark.parametrize("name", BC.HAND)
def test_builders_match_hand_worked_rows(cuda, name):
    from deftet_amd import hip_ops
    tets, n_point = mesh(name)
    check_against_hand(BC.hand(name), face_adj=lambda: np_(hip_ops.tet_face_adj(tets, n_point, cuda)),
                       point_adj=lambda: np_(hip_ops.tet_point_adj(tets, n_point, cuda)), **_library(cuda, tets, n_point))


def test_builders_on_the_empty_mesh(cuda):
    from deftet_amd import hip_ops
    tets, n_point = mesh("empty")
    L = _library(cuda, tets, n_point)
    for got, shape in ((L["adj_share"](), (0, 3)), (np_(hip_ops.tet_face_adj(tets, n_point, cuda)), (0, 2)),
                       (np_(hip_ops.tet_point_adj(tets, n_point, cuda)), (0, 2))):
        assert got.dtype == np.int32 and got.shape == shape
    for fn in (L["to_face"], L["to_face_wb"]):
        f3, t2, tf2, b3, nm = fn()
        assert (f3.shape, t2.shape, tf2.shape, b3.shape, nm) == ((0, 3), (0, 2), (0, 2), (0, 3), 0)
        assert {f3.dtype, t2.dtype, tf2.dtype, b3.dtype} == {np.dtype(np.int64)}
    nbr, owners = L["neighbours"]()
    assert nbr.shape == (0, 4) and owners.shape == (0, 2) and nbr.dtype == owners.dtype == np.int64
    e, te = L["edges_fn"]()
    assert e.shape == (0, 2) and te.shape == (0, 6) and e.dtype == te.dtype == np.int64
    table, adjsum = L["point_adj_idx_fn"]()
    assert table.shape == (n_point, 0) and table.dtype == np.int64
    assert adjsum.shape == (n_point, 1) and adjsum.dtype == np.float32 and (adjsum == 0).all()
    pts = torch.arange(n_point * 3, dtype=torch.float32, device=cuda).reshape(n_point, 3)
    pn, fn, tn = hip_ops.subdivide(torch.from_numpy(tets.astype(np.int64)).to(cuda), pts, pts[:, :2].contiguous())
    assert torch.equal(pn, pts) and torch.equal(fn, pts[:, :2]) and tn.shape == (0, 4) and tn.dtype == torch.int64


@pytest.mark.parametrize("name", ["one", "n1"])
def test_subdivide_matches_hand_worked_children(cuda, name):
    from deftet_amd import hip_ops
    tets, n_point = mesh(name)
    H = BC.hand(name)
    pts = torch.arange(1, n_point * 3 + 1, dtype=torch.float32, device=cuda).reshape(n_point, 3)
    feat = pts[:, :1] * 0.5
    pn, fn, tn = hip_ops.subdivide(torch.from_numpy(tets.astype(np.int64)).to(cuda), pts, feat)
    e = torch.from_numpy(H["edges"]).to(cuda)
    assert tn.dtype == torch.int64 and np.array_equal(np_(tn), H["sub_tet"])
    assert torch.equal(pn, torch.cat([pts, (pts[e[:, 0]] + pts[e[:, 1]]) / 2])) and torch.equal(fn, torch.cat([feat, (feat[e[:, 0]] + feat[e[:, 1]]) / 2]))


@pytest.mark.parametrize("name", ALL)
def test_render_side_rebuilds_on_irregular_meshes(cuda, oracle, name):
    """tet_edges, subdivide (no signature, a random one, all-false, all-true) and point_adj_idx equal oracle.generate_*; a
    repeated vertex gives the self-edge (a,a), its midpoint vertex and a's own id in a's adjacency row"""
    from deftet_amd import hip_ops
    tets, n_point = mesh(name)
    t = tets.astype(np.int64)
    T, K = t.shape[0], 2
    rng = np.random.default_rng(T + n_point)
    pts = rng.standard_normal((n_point, 3), dtype=np.float32)
    feat = rng.standard_normal((n_point, K), dtype=np.float32)
    td, pd, fd = (torch.from_numpy(x).to(cuda) for x in (t, pts, feat))
    e, te = np_(hip_ops.tet_edges(td, n_point))
    eo = oracle.generate_edge(t)
    teo = oracle.generate_tet_edge_idx(t, eo).reshape(T, 6)
    assert e.dtype == te.dtype == np.int64 and e.shape == eo.shape and te.shape == teo.shape
    assert np.array_equal(e, eo) and np.array_equal(te, teo)
    if name in BC.DEGENERATE:
        assert (eo[:, 0] == eo[:, 1]).any()
    for s in (None, rng.random(T) < 0.4, np.zeros(T, bool), np.ones(T, bool)):
        got = np_(hip_ops.subdivide(td, pd, fd, None if s is None else torch.from_numpy(s).to(cuda)))
        want = oracle.generate_subdivision(t, pts, feat, s)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    table, adjsum = hip_ops.point_adj_idx(n_point, td)
    wt, ws = oracle.generate_point_adj_idx(n_point, t)
    assert table.dtype == torch.int64 and tuple(table.shape) == wt.shape and adjsum.dtype == torch.float32
    assert torch.equal(table, torch.from_numpy(wt).to(cuda)) and np.array_equal(np_(adjsum), ws)   # (maxn: 2,097,151 rows, compared on the device)


# ---------------------------------------------------------------------------- the capacity of tet_face_adj
N_DENSE = 24552                                              # rows of fan_dense12; the reference's interface allocates 4 * 66 * 50 = 13,200


def test_face_adj_host_interface_reports_the_overflow_and_writes_nothing_past_the_buffer(cuda, oracle):
    """the reference-shaped class (deftet_tet_face_adj_host underneath) sizes its output as the reference does; on a mesh that
    needs more rows the call fails with the library's limit error naming the row count, where the reference's run.cpp writes
    past the buffer"""
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.utils.lib import _host
    from deftet_amd.utils.lib.tet_face_adj.interface import Tet_face_adj
    tets, n_point = mesh("fan_dense12")
    T = tets.shape[0]
    cap, tail = 4 * T * 50, 4096
    assert oracle.tet_face_adj(tets, n_point).shape[0] == N_DENSE > cap
    iface = Tet_face_adj()
    with pytest.raises(DefTetHipError, match=str(N_DENSE)):
        iface.run(n_point, tets)
    pairs = np.full((cap + tail, 2), SENTINEL, np.int32)      # the caller's buffer is the first `cap` rows; the tail is the guard
    n_pairs = np.full(1, SENTINEL, np.int32)
    with pytest.raises(DefTetHipError, match=str(N_DENSE)):
        _host.call(iface.run_native, "deftet_tet_face_adj_host", _host.ptr(tets), _host.ptr(pairs), _host.ptr(n_pairs), n_point, T)
    assert (pairs[cap:] == SENTINEL).all()
    # and a mesh that fits comes back whole through the same class
    tets2, n2 = mesh("fan20")
    fa = iface.run(n2, tets2).tocoo()
    want = oracle.tet_face_adj(tets2, n2)
    assert np.array_equal(lexsorted(np.stack([fa.row, fa.col], 1)), lexsorted(want)) and (fa.data == 1).all()


def test_face_adj_device_entry_honours_its_capacity(cuda, oracle):
    """deftet_tet_face_adj_i32 with capacity below the row count: n_out reports the full count, the rows below the capacity are
    the oracle's first rows, nothing above it is written.  hip_ops.tet_face_adj (count, then fill) returns all rows."""
    from deftet_amd import _lib, hip_ops
    tets, n_point = mesh("fan_dense12")
    want = oracle.tet_face_adj(tets, n_point)
    assert want.shape[0] == N_DENSE
    assert np.array_equal(np_(hip_ops.tet_face_adj(tets, n_point, cuda)), want)
    lib = _lib.load()
    tet = torch.from_numpy(tets).to(cuda)
    T = tets.shape[0]
    for cap in (0, 1, 10001, N_DENSE - 1, N_DENSE):           # 10,001: inside one lane's run of rows
        out = torch.full((N_DENSE + 64, 2), SENTINEL, dtype=torch.int32, device=cuda)
        n = torch.full((1,), SENTINEL, dtype=torch.int64, device=cuda)
        with _lib.on_device(cuda):
            ws = _lib.workspace(cuda, lib.deftet_builder_workspace_bytes(n_point, T))
            _lib.check(lib.deftet_tet_face_adj_i32(_lib.ptr(tet), _lib.ptr(out), cap, _lib.ptr(n), n_point, T, 1, _lib.ptr(ws),
                                                   ws.numel(), _lib.current_stream(cuda)), "deftet_tet_face_adj_i32")
        assert int(n.item()) == N_DENSE
        got = out.cpu().numpy()
        assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == SENTINEL).all(), cap
