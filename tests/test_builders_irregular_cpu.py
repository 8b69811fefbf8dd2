"""CPU tests (no GPU): the oracle on the irregular meshes of tests/builder_cases.py — many-owner faces, duplicate tets,
repeated vertices, n_point at the face-key limit, sizes around the sort / scan switches — against what the reference's native
builders returned (tests/golden/ref_native_builders_irregular.npz; live from oracle/_ref where it is built), against the
reference's Python twins on the families without repeated vertices (tests/golden/builders_irregular.npz) and against rows worked
out by hand for the tiny families."""
import numpy as np
import pytest

from tests import builder_cases as BC
from tests.test_cpu_oracle_golden import lexsorted, load, split_share

NATIVE = "ref_native_builders_irregular.npz"
TWINS = "builders_irregular.npz"


def native_fixture(name):
    """(tets, n_point, rows) as recorded: the mesh comes from the fixture, so that it and the rows always belong together"""
    g = load(NATIVE)
    return g[name + "_tets"], int(g[name + "_n_point"]), {k: g["%s_%s" % (name, k)].astype(np.int32) for k in ("adj_share", "face_adj", "point_adj")}


def twin_fixture(name):
    g = load(TWINS)
    return g[name + "_tets"], int(g[name + "_n_point"]), {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


def test_fixtures_hold_the_meshes_of_builder_cases():
    for names, fixture in ((BC.REF_NATIVE, native_fixture), (BC.NON_DEGENERATE, twin_fixture)):
        for name in names:
            tets, n_point = BC.case(name)
            got = fixture(name)
            assert got[0].dtype == np.int32 and np.array_equal(got[0], tets) and got[1] == n_point, name


def test_families_are_what_their_tags_say():
    for name in BC.NON_DEGENERATE + ["fan_dense12", "empty"]:
        assert not BC.has_repeated_vertex(BC.case(name)[0]), name
    for name in BC.DEGENERATE:
        assert BC.has_repeated_vertex(BC.case(name)[0]), name
    assert set(BC.HAND) <= set(BC.CASES) and set(BC.REF_NATIVE) | set(BC.LIBRARY_ONLY) == set(BC.CASES)
    sizes = {BC.case(n)[0].shape[0] for n in BC.CASES}
    assert {0, 1, 170, 171, 512, 513, 682, 683, 2048, 2049} <= sizes and max(sizes) == 2049
    tets, n_point = BC.case("maxn")
    assert n_point == 2_097_151 and {0, 1, 2_097_149, 2_097_150} <= set(tets.reshape(-1).tolist())
    for name in ("three_on_face", "dup", "degenerate", "collapsed8", "collapsed8_dups", "soup40_200", "n1"):
        assert BC.many_owner_faces(*BC.case(name))[0] > 0, name


@pytest.mark.parametrize("name", BC.REF_NATIVE)
def test_oracle_matches_reference_native_on_irregular_meshes(oracle, name):
    """row for row, order included (tet_point_adj lex-sorted: the native order is hash order)"""
    tets, n_point, want = native_fixture(name)
    assert want["face_adj"].shape[0] <= 200 * tets.shape[0]                   # the reference's buffer: the fixture stayed inside it
    assert np.array_equal(oracle.tet_adj_share(tets, n_point), want["adj_share"])
    assert np.array_equal(oracle.tet_face_adj(tets, n_point, wrap32=True), want["face_adj"])
    assert np.array_equal(oracle.tet_point_adj(tets, n_point), lexsorted(want["point_adj"]))
    if oracle.RefBuilders.available():
        ref = oracle.RefBuilders()
        assert np.array_equal(ref.tet_adj_share(tets, n_point), want["adj_share"])
        assert np.array_equal(ref.tet_face_adj(tets, n_point), want["face_adj"])
        assert np.array_equal(lexsorted(ref.tet_point_adj(tets, n_point)), lexsorted(want["point_adj"]))


def check_against_twins(name, G, adj_share, to_face, to_face_wb, neighbours, edges_fn, point_adj_idx_fn):
    """shared by the CPU (oracle) and GPU (library) tests: every callable returns numpy arrays for the family's mesh"""
    rows = adj_share()
    if int(G["adj_share_raises"]) == 1:                     # IndexError: no shared face at all, the twin indexes an empty list
        assert rows.shape[0] == 0
    elif int(G["adj_share_raises"]) == 0:                   # (2, ValueError on a many-owner face: the native rows are the pin)
        for i in range(4):
            assert np.array_equal(split_share(rows, i), G["adj_share_%d" % i])
    f3, t2, tf2, b3, nm = to_face()
    assert np.array_equal(f3, G["face_fx3"]) and np.array_equal(t2, G["face_tetidx_fx2"])
    assert np.array_equal(tf2, G["face_tetfaceidx_fx2"]) and np.array_equal(b3, G["boundary_fx3"])
    w3, w2, wf2, _, nm2 = to_face_wb()
    assert np.array_equal(w3, G["facewb_fx3"]) and np.array_equal(w2, G["facewb_tetidx_fx2"])
    assert np.array_equal(wf2, G["facewb_tetfaceidx_fx2"]) and nm2 == nm
    assert (nm > 0) == (int(G["withtet_raises"]) == 2) == (int(G["nbr_raises"]) == 2)   # the twins raise ValueError exactly then
    if nm > 0:
        with pytest.raises(ValueError):
            neighbours()
    else:
        nbr, owners = neighbours()
        assert np.array_equal(owners, G["face_withtet_4tx2"])
        if int(G["nbr_raises"]) == 0:
            assert np.array_equal(nbr, G["adj_share_nbr_tx4"])
        else:                                               # IndexError after the table was filled: no face is shared
            assert (nbr == -1).all()
    e, te = edges_fn()
    assert np.array_equal(e, G["edges"]) and np.array_equal(te, G["tet_edge"])
    if int(G["point_adj_raises"]) == 0:
        table, adjsum = point_adj_idx_fn()
        assert np.array_equal(table, G["adj_table"]) and np.array_equal(adjsum, G["adjsum"]) and adjsum.dtype == G["adjsum"].dtype


@pytest.mark.parametrize("name", BC.NON_DEGENERATE)
def test_oracle_matches_python_twins_on_irregular_meshes(oracle, name):
    tets, n_point, G = twin_fixture(name)
    t64 = tets.astype(np.int64)

    def edges():
        e = oracle.generate_edge(t64)
        return e, oracle.generate_tet_edge_idx(t64, e)

    check_against_twins(name, G, lambda: oracle.tet_adj_share(tets, n_point), lambda: oracle.tet_to_face(tets, n_point),
                        lambda: oracle.tet_to_face(tets, n_point, with_boundary=True), lambda: oracle.tet_neighbours(tets, n_point),
                        edges, lambda: oracle.generate_point_adj_idx(n_point, t64))


def check_against_hand(H, adj_share, face_adj, point_adj, to_face, to_face_wb, neighbours, edges_fn, point_adj_idx_fn):
    """shared by the CPU (oracle) and GPU (library) tests"""
    for got, want in ((adj_share(), H["adj_share"]), (face_adj(), H["face_adj"]), (point_adj(), H["point_adj"])):
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    got = to_face()
    for a, b in zip(got[:4], H["face"][:4]):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)
    assert got[4] == H["face"][4]
    got = to_face_wb()
    for a, b in zip(got[:3], H["facewb"]):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)
    assert got[3].shape == H["face"][3].shape and got[4] == H["face"][4]
    if H["nbr"] is None:
        with pytest.raises(ValueError):
            neighbours()
    else:
        nbr, owners = neighbours()
        assert nbr.dtype == np.int64 and nbr.shape == H["nbr"].shape and np.array_equal(nbr, H["nbr"])
        assert owners.dtype == np.int64 and owners.shape == H["owners"].shape and np.array_equal(owners, H["owners"])
    e, te = edges_fn()
    assert e.dtype == np.int64 and e.shape == H["edges"].shape and np.array_equal(e, H["edges"])
    assert te.dtype == np.int64 and te.shape == H["tet_edge"].shape and np.array_equal(te, H["tet_edge"])
    table, adjsum = point_adj_idx_fn()
    assert table.dtype == np.int64 and table.shape == H["adj_table"].shape and np.array_equal(table, H["adj_table"])
    assert adjsum.dtype == np.float32 and adjsum.shape == H["adjsum"].shape and np.array_equal(adjsum, H["adjsum"])


@pytest.mark.parametrize("name", BC.HAND)
def test_oracle_matches_hand_worked_rows(oracle, name):
    tets, n_point = BC.case(name)
    t64 = tets.astype(np.int64)

    def edges():
        e = oracle.generate_edge(t64)
        return e, oracle.generate_tet_edge_idx(t64, e)

    check_against_hand(BC.hand(name), lambda: oracle.tet_adj_share(tets, n_point), lambda: oracle.tet_face_adj(tets, n_point),
                       lambda: oracle.tet_point_adj(tets, n_point), lambda: oracle.tet_to_face(tets, n_point),
                       lambda: oracle.tet_to_face(tets, n_point, with_boundary=True), lambda: oracle.tet_neighbours(tets, n_point),
                       edges, lambda: oracle.generate_point_adj_idx(n_point, t64))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_oracle_face_tables_account_for_every_tet_face(oracle, name):
    """2 * interior + boundary + (tet-faces of many-owner keys) = 4T, with the many-owner keys counted independently
    (np.unique over builder_cases.face_key_share)"""
    tets, n_point = BC.case(name)
    n_keys, n_owned = BC.many_owner_faces(tets, n_point)
    for wb in (False, True):
        f3, t2, tf2, b3, nm = oracle.tet_to_face(tets, n_point, with_boundary=wb)
        n_interior = f3.shape[0] - (b3.shape[0] if wb else 0)
        assert nm == n_keys and 2 * n_interior + b3.shape[0] + n_owned == 4 * tets.shape[0]


def test_fan_dense12_exceeds_the_reference_buffer(oracle):
    tets, n_point = BC.case("fan_dense12")
    assert tets.shape[0] == 66 and oracle.tet_face_adj(tets, n_point).shape[0] == 24552 > 4 * 66 * 50
