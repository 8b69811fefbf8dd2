"""Irregular tet meshes for the adjacency / face-table builders (deftet_amd/csrc/builders.hip): faces with more than two
owners, duplicate tets, tets with repeated vertices, the largest vertex count the face keys allow, and sizes that straddle the
tile and single-workgroup limits of the sort and the scan underneath (prims.hpp: 2,048-key tiles, one-workgroup scan up to 8,192
entries; the builders sort 4T face keys and 12T edge keys).  Deterministic (seeded numpy) and self-contained: the generators
under tests/golden/ and the CPU and GPU tests all take their inputs from here.

    CASES[name]() -> (tets int32 [T,4], n_point)
"""
import numpy as np

from deftet_amd import grids

FACE_IDX = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]])
MAX_N_POINT = 2_097_151                         # check_common: face keys min*n^2 + max*n + mid fill the 63 sorted bits


def _i32(rows):
    return np.asarray(rows, np.int32).reshape(-1, 4)


def three_on_face():
    return _i32([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]]), 6


def dup():
    """the same row twice, the same tet with its corners reversed, and a third owner on a face of each pair"""
    return _i32([[0, 1, 2, 3], [0, 1, 2, 3], [4, 5, 6, 7], [7, 6, 5, 4], [1, 2, 3, 8], [5, 6, 7, 9], [0, 1, 2, 10]]), 11


def degenerate():
    """Repeated vertices in every pair of slots, a triple and a quadruple, next to regular tets that share faces with them.
    Local face 0 of tets 2, 3 and 4 is (5,5,1), (5,1,5) and (1,5,1): the face key of tet_adj_share / tet_to_face (third corner
    when no corner lies strictly between) joins the first and the third, the absolute face id of tet_face_adj (first corner) the
    first and the second."""
    return _i32([[0, 1, 2, 3], [1, 2, 3, 4],
                 [5, 5, 1, 2], [5, 1, 5, 7], [1, 5, 1, 8],
                 [1, 2, 5, 5], [7, 1, 5, 5], [5, 1, 2, 5], [1, 5, 2, 5],
                 [0, 0, 1, 2],                   # faces 2 and 3 coincide with face 0 of tet 0: three owners
                 [2, 3, 3, 4],                   # face 1 = (3,2,4) is face 3 of tet 1
                 [6, 6, 6, 6], [3, 9, 9, 9], [9, 9, 9, 3]]), 10


def self_owned():
    """tet 1 owns one face key twice (local faces 2 and 3 of [a,a,b,c]); tets 0 and 2 share an ordinary face"""
    return _i32([[0, 1, 2, 3], [5, 5, 1, 2], [1, 2, 3, 4]]), 6


def fan20():
    return _i32([[0, 1, 2 + i, 2 + (i + 1) % 20] for i in range(20)]), 22


def fan_dense12():
    """every pair of 12 vertices around the edge (0,1): T = 66 and 24,552 face-adjacency rows, more than the 4*T*50 = 13,200
    the reference's interface allocates — never handed to the reference's native builders"""
    return _i32([[0, 1, 2 + i, 2 + j] for i in range(12) for j in range(i + 1, 12)]), 14


def _collapsed8(n_dup_rows):
    rng = np.random.default_rng(808)
    verts, tets = grids.kuhn_grid(8)
    nv = verts.shape[0]
    src = rng.choice(nv, 60, replace=False)
    remap = np.arange(nv)
    remap[src] = rng.integers(0, nv, 60)         # merged vertices: repeated corners, duplicate tets, many-owner faces
    tets = remap[tets]
    tets = tets[rng.permutation(tets.shape[0])]
    if n_dup_rows:
        same = tets[rng.choice(tets.shape[0], 40, replace=False)]
        rev = tets[rng.choice(tets.shape[0], 10, replace=False)][:, ::-1]
        tets = np.concatenate([tets, same, rev], 0)
        tets = tets[rng.permutation(tets.shape[0])]
    return _i32(tets), nv


def collapsed8():
    return _collapsed8(False)


def collapsed8_dups():
    return _collapsed8(True)


def _soup(nv, T):
    def make():
        rng = np.random.default_rng(1000 * nv + T)
        return _i32(rng.integers(0, nv, (T, 4))), nv
    make.__name__ = "soup%d_%d" % (nv, T)
    return make


def maxn():
    """res-2 Kuhn grid (6 tets, 8 vertices) on sparse ids at both ends of [0, n_point) with n_point at the limit"""
    rng = np.random.default_rng(21)
    verts, tets = grids.kuhn_grid(2)
    ids = np.sort(np.concatenate([[0, 1, MAX_N_POINT - 2, MAX_N_POINT - 1], rng.choice(np.arange(2, MAX_N_POINT - 2), 4, replace=False)]))
    return _i32(ids[rng.permutation(8)][tets]), MAX_N_POINT


def n1():
    return _i32(np.zeros((3, 4))), 1


def one():
    return _i32([[0, 1, 2, 3]]), 4


def empty():
    return _i32(np.zeros((0, 4))), 4


# T in {170,171}: 12T straddles 2,048; {512,513}: 4T straddles 2,048; {682,683}: 12T straddles 8,192; {2048,2049}: 4T straddles
# 8,192.  The vertex counts keep the face-adjacency row count under the reference's 200*T buffer (asserted by gen_ref_native_irregular.py).
SOUPS = [(40, 200), (60, 513), (100, 683), (40, 170), (40, 171), (60, 512), (100, 682), (256, 2048), (256, 2049)]

CASES = {f.__name__: f for f in [three_on_face, dup, degenerate, self_owned, fan20, collapsed8, collapsed8_dups]
         + [_soup(nv, T) for nv, T in SOUPS] + [maxn, n1, one, empty, fan_dense12]}

LIBRARY_ONLY = ["fan_dense12"]                                                    # never for the reference
REF_NATIVE = [n for n in CASES if n not in LIBRARY_ONLY]                          # ref_native_builders_irregular.npz
NON_DEGENERATE = ["three_on_face", "dup", "fan20", "maxn", "one"]                 # builders_irregular.npz (Python twins)
DEGENERATE = [n for n in CASES if n not in NON_DEGENERATE + ["empty", "fan_dense12"]]


def case(name):
    return CASES[name]()


def has_repeated_vertex(tets):
    s = np.sort(np.asarray(tets), 1)
    return bool((s[:, 1:] == s[:, :-1]).any())


def face_key_share(tets, n_point):
    """uint64 [T,4] key of tet_adj_share / tet_to_face, from its definition: min*n^2 + max*n + c where c is the last corner that
    is neither the minimum nor the maximum, and the third corner when there is none (n_point <= 2,097,151: no overflow)"""
    tri = np.asarray(tets, np.int64)[:, FACE_IDX]                                  # [T,4,3]
    a, b = tri.min(-1), tri.max(-1)
    c = tri[..., 2].copy()
    for k in range(3):
        mid = (tri[..., k] != a) & (tri[..., k] != b)
        c[mid] = tri[..., k][mid]
    n = np.uint64(n_point)
    return a.astype(np.uint64) * n * n + b.astype(np.uint64) * n + c.astype(np.uint64)


def many_owner_faces(tets, n_point):
    """(number of face keys with more than two owners, number of tet-faces they own), by np.unique on the keys"""
    if len(tets) == 0:
        return 0, 0
    _, cnt = np.unique(face_key_share(tets, n_point).reshape(-1), return_counts=True)
    return int((cnt > 2).sum()), int(cnt[cnt > 2].sum())


def face_adj_rows_from_runs(runs, same_face_groups):
    """tet_face_adj rows from hand-listed runs: for every edge, in ascending key order, the global faces (4*tet + local face)
    that contain it, in insertion order, once per containing edge; every ordered pair of a run is a row unless the two entries
    are the same face or faces with the same absolute id"""
    grp = {}
    for i, g in enumerate(same_face_groups):
        for f in g:
            grp[f] = i
    rows = [[x, y] for run in runs for x in run for y in run if x != y and (grp.get(x, -1 - x) != grp.get(y, -1 - y))]
    return np.asarray(rows, np.int32).reshape(-1, 2)


# ---------------------------------------------------------------------------- hand-worked expectations for the tiny families
# Local faces of [a,b,c,d]: 0 = (a,b,c), 1 = (b,a,d), 2 = (c,d,a), 3 = (d,c,b); global face = 4*tet + local face.
def _a(rows, width, dtype=np.int64):
    return np.asarray(rows, dtype).reshape(-1, width)


def _pad(rows, width):
    return _a([r + [-1] * (width - len(r)) for r in rows], width)


def hand(name):
    """What every builder returns on `three_on_face`, `one`, `n1` and `self_owned`, written out from the definitions.
    keys: adj_share [*,3], face_adj [*,2], point_adj [*,2] (sorted), face = (face_fx3, tetidx_fx2, tetfaceidx_fx2, boundary_fx3,
    n_many_owner) without boundary, facewb = the first three with boundary faces inline, nbr [T,4] and owners [4T,2] (None: a face
    has more than two owners, tet_neighbours raises ValueError), edges [E,2], tet_edge [T,6], adj_table [P,m], adjsum [P,1]; `one` and `n1` also sub_tet [8T,4], the
    children of a full subdivision (new vertex n_point + e is the midpoint of edge row e)."""
    if name == "one":                                            # [0,1,2,3], n = 4: every pair of its faces shares one edge
        tri = [[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]]
        return dict(
            adj_share=_a([], 3, np.int32),
            # edges by key a*4+b: (0,1) faces 0,1; (0,2) 0,2; (0,3) 1,2; (1,2) 0,3; (1,3) 1,3; (2,3) 2,3
            face_adj=face_adj_rows_from_runs([[0, 1], [0, 2], [1, 2], [0, 3], [1, 3], [2, 3]], []),
            point_adj=_a([[i, j] for i in range(4) for j in range(4) if i != j], 2, np.int32),
            face=(_a([], 3), _a([], 2), _a([], 2), _a(tri, 3), 0),
            facewb=(_a(tri, 3), _a([[0, -1]] * 4, 2), _a([[0, -1], [1, -1], [2, -1], [3, -1]], 2)),
            nbr=_a([[-1, -1, -1, -1]], 4), owners=_a([[0, 0]] * 4, 2),
            edges=_a([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], 2), tet_edge=_a([[0, 1, 2, 3, 4, 5]], 6),
            adj_table=_a([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], 3), adjsum=_a([3] * 4, 1, np.float32),
            # midpoints ab, ac, ad, bc, bd, cd = 4 + edge row = 4..9
            sub_tet=_a([[0, 4, 5, 6], [1, 7, 4, 8], [2, 5, 7, 9], [3, 6, 9, 8], [4, 5, 6, 8], [4, 5, 8, 7], [9, 5, 8, 6], [9, 5, 7, 8]], 4))
    if name == "n1":                                             # three [0,0,0,0], n = 1: one face key with twelve owners
        return dict(
            adj_share=_a([], 3, np.int32),
            face_adj=_a([], 2, np.int32),                        # one edge run of 36 entries, all with the same absolute face id
            point_adj=_a([[0, 0]], 2, np.int32),
            face=(_a([], 3), _a([], 2), _a([], 2), _a([], 3), 1),
            facewb=(_a([], 3), _a([], 2), _a([], 2)),
            nbr=None, owners=None,
            edges=_a([[0, 0]], 2), tet_edge=np.zeros((3, 6), np.int64),
            adj_table=_a([[0]], 1), adjsum=_a([1], 1, np.float32),
            sub_tet=_a(([[0, 1, 1, 1]] * 4 + [[1, 1, 1, 1]] * 4) * 3, 4))          # the one midpoint is vertex 1
    if name == "three_on_face":                                  # [0,1,2,3], [0,1,2,4], [0,1,2,5], n = 6: faces 0, 4, 8 are (0,1,2)
        bnd = [[1, 0, 3], [2, 3, 0], [3, 2, 1], [1, 0, 4], [2, 4, 0], [4, 2, 1], [1, 0, 5], [2, 5, 0], [5, 2, 1]]
        runs = [[0, 1, 4, 5, 8, 9],                              # edge (0,1), key 1
                [0, 2, 4, 6, 8, 10],                             # (0,2)
                [1, 2], [5, 6], [9, 10],                         # (0,3), (0,4), (0,5)
                [0, 3, 4, 7, 8, 11],                             # (1,2), key 8
                [1, 3], [5, 7], [9, 11],                         # (1,3), (1,4), (1,5)
                [2, 3], [6, 7], [10, 11]]                        # (2,3), (2,4), (2,5)
        return dict(
            adj_share=_a([], 3, np.int32),
            face_adj=face_adj_rows_from_runs(runs, [[0, 4, 8]]),
            point_adj=_a([[i, j] for i in range(6) for j in range(6) if i != j and not (i >= 3 and j >= 3)], 2, np.int32),
            face=(_a([], 3), _a([], 2), _a([], 2), _a(bnd, 3), 1),
            facewb=(_a(bnd, 3), _a([[t, -1] for t in range(3) for _ in range(3)], 2), _a([[1, -1], [2, -1], [3, -1]] * 3, 2)),
            nbr=None, owners=None,
            edges=_a([[0, 1], [0, 2], [0, 3], [0, 4], [0, 5], [1, 2], [1, 3], [1, 4], [1, 5], [2, 3], [2, 4], [2, 5]], 2),
            tet_edge=_a([[0, 1, 2, 5, 6, 9], [0, 1, 3, 5, 7, 10], [0, 1, 4, 5, 8, 11]], 6),
            adj_table=_pad([[1, 2, 3, 4, 5], [0, 2, 3, 4, 5], [0, 1, 3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 1, 2]], 5),
            adjsum=_a([5, 5, 5, 3, 3, 3], 1, np.float32))
    if name == "self_owned":                                     # [0,1,2,3], [5,5,1,2], [1,2,3,4], n = 6
        # faces: 0 (0,1,2) 1 (1,0,3) 2 (2,3,0) 3 (3,2,1) | 4 (5,5,1) 5 (5,5,2) 6 (1,2,5) 7 (2,1,5) | 8 (1,2,3) 9 (2,1,4) 10 (3,4,1)
        # 11 (4,3,2).  Share keys a*36+b*6+c: faces 3 and 8 -> (1,3,2) = 56; faces 6 and 7 -> (1,5,2) = 68; face 4 -> (1,5,1),
        # face 5 -> (2,5,2) (third corner), every other face alone.
        runs = [[0, 1], [0, 2], [1, 2],                          # edges (0,1), (0,2), (0,3)
                [0, 3, 6, 7, 8, 9],                              # (1,2)
                [1, 3, 8, 10], [9, 10],                          # (1,3), (1,4)
                [4, 4, 6, 7],                                    # (1,5): two edges of face 4
                [2, 3, 8, 11], [9, 11],                          # (2,3), (2,4)
                [5, 5, 6, 7],                                    # (2,5): two edges of face 5
                [10, 11], [4, 5]]                                # (3,4), (5,5)
        wb_f = [[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1], [5, 5, 1], [5, 5, 2], [1, 2, 5], [2, 1, 4], [3, 4, 1], [4, 3, 2]]
        wb_t = [[0, -1], [0, -1], [0, -1], [0, 2], [1, -1], [1, -1], [1, 1], [2, -1], [2, -1], [2, -1]]
        wb_l = [[0, -1], [1, -1], [2, -1], [3, 0], [0, -1], [1, -1], [2, 3], [1, -1], [2, -1], [3, -1]]
        return dict(
            adj_share=_a([[0, 2, 3], [2, 0, 0], [1, 1, 2], [1, 1, 3]], 3, np.int32),
            face_adj=face_adj_rows_from_runs(runs, [[3, 8], [6, 7]]),
            point_adj=_a([[0, 1], [0, 2], [0, 3], [1, 0], [1, 2], [1, 3], [1, 4], [1, 5], [2, 0], [2, 1], [2, 3], [2, 4], [2, 5],
                          [3, 0], [3, 1], [3, 2], [3, 4], [4, 1], [4, 2], [4, 3], [5, 1], [5, 2], [5, 5]], 2, np.int32),
            face=(_a([[3, 2, 1], [1, 2, 5]], 3), _a([[0, 2], [1, 1]], 2), _a([[3, 0], [2, 3]], 2),
                  _a([[0, 1, 2], [1, 0, 3], [2, 3, 0], [5, 5, 1], [5, 5, 2], [2, 1, 4], [3, 4, 1], [4, 3, 2]], 3), 0),
            facewb=(_a(wb_f, 3), _a(wb_t, 2), _a(wb_l, 2)),
            nbr=_a([[2, -1, -1, -1], [1, 1, -1, -1], [0, -1, -1, -1]], 4),       # tet 1 is its own neighbour, twice in succession
            owners=_a([[0, 0], [0, 0], [0, 0], [0, 2], [1, 0], [1, 0], [1, 1], [1, 1], [0, 2], [2, 0], [2, 0], [2, 0]], 2),
            edges=_a([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [1, 4], [1, 5], [2, 3], [2, 4], [2, 5], [3, 4], [5, 5]], 2),
            tet_edge=_a([[0, 1, 2, 3, 4, 7], [11, 6, 9, 6, 9, 3], [3, 4, 5, 7, 8, 10]], 6),
            adj_table=_pad([[1, 2, 3], [0, 2, 3, 4, 5], [0, 1, 3, 4, 5], [0, 1, 2, 4], [1, 2, 3], [1, 2, 5]], 5),
            adjsum=_a([3, 5, 5, 4, 3, 3], 1, np.float32))
    raise KeyError(name)


HAND = ["three_on_face", "one", "n1", "self_owned"]
