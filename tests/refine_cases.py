"""Inputs shared by tests/test_refine_ref_cpu.py and tests/test_tet_refine_gpu.py: the hand-worked refinements, written out from
the contract, and the seeded grids and selections.  The reference refinement of a grid case is computed
once (reference()) and handed out read-only."""
import os

import numpy as np

from deftet_amd import grids
from tests import refine_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the eight children of [a,b,c,d] with midpoints ab, ac, ad, bc, bd, cd (k_subdiv_tets)
def _eight(a, b, c, d, ab, ac, ad, bc, bd, cd):
    return [[a, ab, ac, ad], [b, bc, ab, bd], [c, ac, bc, cd], [d, ad, cd, bd], [ab, ac, ad, bd], [ab, ac, bd, bc], [cd, ac, bd, ad], [cd, ac, bc, bd]]


def _case(tets, n_point, select, split, tet_new, parent, kind):
    return dict(tets=np.asarray(tets, np.int64).reshape(-1, 4), n_point=n_point, select=np.asarray(select, bool),
                edges_split=np.asarray(split, np.int64).reshape(-1, 2), tet_new=np.asarray(tet_new, np.int64).reshape(-1, 4),
                parent=np.asarray(parent, np.int64), kind=np.asarray(kind, np.uint8))


HAND = {
    # one tet, selected: edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) become vertices 4..9
    "one_selected": _case([[0, 1, 2, 3]], 4, [1], [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]],
                          [[0, 4, 5, 6], [1, 7, 4, 8], [2, 5, 7, 9], [3, 6, 9, 8], [4, 5, 6, 8], [4, 5, 8, 7], [9, 5, 8, 6], [9, 5, 7, 8]], [0] * 8, [6] * 8),
    "one_unselected": _case([[0, 1, 2, 3]], 4, [0], [], [[0, 1, 2, 3]], [0], [0]),
    # [0,1,2,3] selected and [1,2,3,4] across the face (1,2,3).  Edge list (0,1) (0,2) (0,3) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4);
    # marked: (0,1)->5 (0,2)->6 (0,3)->7 (1,2)->8 (1,3)->9 (2,3)->10.  The neighbour has slots ab, ac, bc marked = its face abc, local
    # corners p, q, r = 0, 1, 2: m(p,q) = 8, m(p,r) = 9, m(q,r) = 10
    "shared_face": _case([[0, 1, 2, 3], [1, 2, 3, 4]], 5, [1, 0], [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]],
                         _eight(0, 1, 2, 3, 5, 6, 7, 8, 9, 10) + [[1, 8, 9, 4], [8, 2, 10, 4], [9, 10, 3, 4], [8, 10, 9, 4]],
                         [0] * 8 + [1] * 4, [6] * 8 + [3] * 4),
    # [0,1,2,3] selected and [0,1,4,5] on the edge (0,1) only.  Edge list (0,1) (0,2) (0,3) (0,4) (0,5) (1,2) (1,3) (1,4) (1,5) (2,3)
    # (4,5); marked: (0,1)->6 (0,2)->7 (0,3)->8 (1,2)->9 (1,3)->10 (2,3)->11.  The neighbour has slot ab marked: v[b] = 6, then v[a] = 6
    "shared_edge": _case([[0, 1, 2, 3], [0, 1, 4, 5]], 6, [1, 0], [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]],
                         _eight(0, 1, 2, 3, 6, 7, 8, 9, 10, 11) + [[0, 6, 4, 5], [6, 1, 4, 5]], [0] * 8 + [1] * 2, [6] * 8 + [1] * 2),
    # X = [0,1,2,3] between A = [0,1,4,5] and B = [2,3,6,7], A and B selected.  Edge list (0,1) (0,2) (0,3) (0,4) (0,5) (1,2) (1,3)
    # (1,4) (1,5) (2,3) (2,6) (2,7) (3,6) (3,7) (4,5) (6,7); marked: (0,1)->8 (0,4)->9 (0,5)->10 (1,4)->11 (1,5)->12 (2,3)->13 (2,6)->14
    # (2,7)->15 (3,6)->16 (3,7)->17 (4,5)->18 (6,7)->19.  X has its opposite slots ab and cd marked, no face with two: m0 = 8 on
    # (p0,q0) = corners (0,1), m1 = 13 on (p1,q1) = corners (2,3)
    "opposite_edges": _case([[0, 1, 2, 3], [0, 1, 4, 5], [2, 3, 6, 7]], 8, [0, 1, 1],
                            [[0, 1], [0, 4], [0, 5], [1, 4], [1, 5], [2, 3], [2, 6], [2, 7], [3, 6], [3, 7], [4, 5], [6, 7]],
                            [[0, 8, 2, 13], [0, 8, 13, 3], [8, 1, 2, 13], [8, 1, 13, 3]]
                            + _eight(0, 1, 4, 5, 8, 9, 10, 11, 12, 18) + _eight(2, 3, 6, 7, 13, 14, 15, 16, 17, 19),
                            [0] * 4 + [1] * 8 + [2] * 8, [2] * 4 + [6] * 16),
}


def hand_points(n_point, n_feat=2):
    """positions and features of a hand case: small integers over 8, so every midpoint is exact in fp32 and in any order"""
    rng = np.random.default_rng(n_point)
    return (rng.integers(-40, 40, (n_point, 3)) / 8.0).astype(np.float32), (rng.integers(-40, 40, (n_point, n_feat)) / 8.0).astype(np.float32)


# ---------------------------------------------------------------------------- grids and selections
GRIDS = ["kuhn8", "kuhn8_jitter", "kuhn20", "kuhn20_jitter", "cube40"]
SELECTIONS = ["band", "random", "single"]
_grids, _refs = {}, {}


def grid(name):
    """(tets int64 [T,4], points f32 [P,3] inside [-0.5, 0.5]^3, neighbour table int64 [T,4])"""
    if name not in _grids:
        if name == "cube40":
            d = np.load(os.path.join(GOLD, "cube40_grid.npz"))
            tets = d["tets"].astype(np.int64)
            pos = d["verts"] - d["verts"].mean(0)
            pts = (pos / np.abs(pos).max() * 0.5).astype(np.float32)
        else:
            res = int(name[4:].split("_")[0])
            verts, tets = grids.kuhn_grid(res)
            tets = tets.astype(np.int64)
            pts = grids.jittered_positions(verts, res, 1, jitter=0.1 if name.endswith("_jitter") else 0.0)[0]     # 0.1 h, h = the cell
        for a in (tets, pts):
            a.setflags(write=False)
        _grids[name] = (tets, pts, R.neighbour_table(tets))
    return _grids[name]


def selection(name, sel):
    """bool [T]: `band` = the tets with a face neighbour on the other side of the r = 0.3 sphere; `random` = 5 % of the tets;
    `single` = one tet in the middle of the list"""
    tets, pts, nbr = grid(name)
    T = tets.shape[0]
    if sel == "band":
        return R.occupancy_band(R.sphere_inside(pts, tets), nbr, 0)
    if sel == "random":
        return np.random.default_rng(2020 + T).random(T) < 0.05
    if sel == "single":
        return np.arange(T) == T // 2
    if sel == "all":
        return np.ones(T, bool)
    if sel == "none":
        return np.zeros(T, bool)
    raise KeyError(sel)


def features(pts, K):
    f = np.random.default_rng(pts.shape[0] + K).random((pts.shape[0], K)).astype(np.float32)
    return f


def reference(name, sel, K=2):
    """the numpy refinement of (grid, selection), computed once; read-only"""
    key = (name, sel, K)
    if key not in _refs:
        tets, pts, _ = grid(name)
        r = R.refine(tets, pts, features(pts, K), selection(name, sel))
        for a in r[:7]:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]
