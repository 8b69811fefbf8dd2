"""numpy restatement of conforming selective tet refinement (red-green closure on edge marks), the
reference of tests/test_refine_ref_cpu.py and tests/test_tet_refine_gpu.py.

The contract, in the order refine() follows it:
  1. every edge of every selected tet is marked;
  2. closure: until nothing changes, a face of a tet with at least two of its three edges marked gets the third marked.  The
     rule is monotone, so the result is its least fixed point whatever the order.  close_jacobi() reads, in every round, only the
     marks of the round before (deliberately not the in-place schedule of the kernels); close_gauss_seidel() updates in place, one
     tet after the other in a given order, and must end at the same marks;
  3. marked edge number r (in tet_edges order) becomes vertex P + r = (x[a] + x[b]) / 2 in fp32;
  4. tets in parent order, the children of one parent contiguous, in the order of CHILDREN below, which is built from the words
     of the contract: "v with v[i] = m" is the parent with local position i replaced by midpoint m.

Local edge slots: 0 ab, 1 ac, 2 ad, 3 bc, 4 bd, 5 cd.  A pattern is the 6-bit mask of a tet's marked slots.
"""
import collections

import numpy as np

from tests.surface_extract_ref import neighbour_table            # noqa: F401  nbr[t][i] = the tet across local face i, -1 for none

ENDS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
SLOT = {e: s for s, e in enumerate(ENDS)}
FACES = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]                       # corners of abc, abd, acd, bcd
FACE_SLOTS = [tuple(SLOT[e] for e in ((p, q), (p, r), (q, r))) for p, q, r in FACES]   # {0,1,3}, {0,2,4}, {1,2,5}, {3,4,5}
FACE_MASK = [sum(1 << s for s in f) for f in FACE_SLOTS]
assert FACE_SLOTS == [(0, 1, 3), (0, 2, 4), (1, 2, 5), (3, 4, 5)]

Refined = collections.namedtuple("Refined", "points_new feat_new tet_new parent kind edges_split marks rounds")


def _mid(p, q):
    return 4 + SLOT[(min(p, q), max(p, q))]                                # codes: 0..3 = the parent's corner, 4 + slot = a midpoint


def _with(repl):
    return [repl.get(i, i) for i in range(4)]


def _children():
    """mask -> list of children, each four codes; only the legal masks are keys"""
    table = {0: [[0, 1, 2, 3]]}
    for e, (p, q) in enumerate(ENDS):                                       # kind 1
        m = 4 + e
        table[1 << e] = [_with({q: m}), _with({p: m})]
    for e0 in range(3):                                                     # kind 2: opposite edges e0 < e1 = 5 - e0
        e1 = 5 - e0
        (p0, q0), (p1, q1), m0, m1 = ENDS[e0], ENDS[e1], 4 + e0, 4 + e1
        table[(1 << e0) | (1 << e1)] = [_with({q0: m0, q1: m1}), _with({q0: m0, p1: m1}), _with({p0: m0, q1: m1}), _with({p0: m0, p1: m1})]
    for (p, q, r), mask in zip(FACES, FACE_MASK):                           # kind 3: one face, corners p < q < r
        table[mask] = [_with({q: _mid(p, q), r: _mid(p, r)}), _with({p: _mid(p, q), r: _mid(q, r)}), _with({p: _mid(p, r), q: _mid(q, r)}),
                       _with({p: _mid(p, q), q: _mid(q, r), r: _mid(p, r)})]
    a, b, c, d = 0, 1, 2, 3                                                 # kind 6: the eight children of a full subdivision
    ab, ac, ad, bc, bd, cd = (4 + s for s in range(6))
    table[63] = [[a, ab, ac, ad], [b, bc, ab, bd], [c, ac, bc, cd], [d, ad, cd, bd], [ab, ac, ad, bd], [ab, ac, bd, bc], [cd, ac, bd, ad],
                 [cd, ac, bc, bd]]
    return table


CHILDREN = _children()
LEGAL = sorted(CHILDREN)
N_CHILD = np.ones(64, np.int64)
for _m, _c in CHILDREN.items():
    N_CHILD[_m] = len(_c)
IS_LEGAL = np.zeros(64, bool)
IS_LEGAL[LEGAL] = True
POPCOUNT = np.array([bin(m).count("1") for m in range(64)], np.uint8)


def _close_mask(m):
    while True:
        n = m
        for f in FACE_MASK:
            if bin(n & f).count("1") >= 2:
                n |= f
        if n == m:
            return m
        m = n


LOCAL_CLOSE = [_close_mask(m) for m in range(64)]                           # the fixed point of the face rule inside one tet


def tet_edges(tets, n_point=None):
    """(edges int64 [E,2] unique (min, max) rows in lexicographic order, tet_edge int64 [T,6]) as hip_ops.tet_edges returns them"""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    if tets.shape[0] == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0, 6), np.int64)
    pair = tets[:, np.asarray(ENDS)]                                        # [T,6,2]
    lo, hi = pair.min(-1), pair.max(-1)
    n = np.int64(int(tets.max()) + 1 if n_point is None else n_point)
    key, inv = np.unique(lo * n + hi, return_inverse=True)
    return np.stack([key // n, key % n], 1), inv.reshape(-1, 6).astype(np.int64)


def initial_marks(tet_edge, select, n_edge):
    marks = np.zeros(n_edge, bool)
    marks[tet_edge[np.asarray(select, bool).reshape(-1)].reshape(-1)] = True
    return marks


def patterns(tet_edge, marks):
    """uint8 [T]: bit s set when slot s of the tet is marked"""
    return (marks[tet_edge].astype(np.uint8) << np.arange(6, dtype=np.uint8)).sum(1).astype(np.uint8) if tet_edge.shape[0] else np.zeros(0, np.uint8)


def close_jacobi(tet_edge, marks):
    """(closed marks, rounds that changed something); every round reads the marks of the round before only"""
    marks = marks.copy()
    rounds = 0
    while True:
        m = marks[tet_edge]                                                 # [T,6], the state before the round
        new = marks.copy()
        for f in FACE_SLOTS:
            cnt = m[:, f].sum(1)
            hit = tet_edge[cnt >= 2][:, f]
            new[hit.reshape(-1)] = True
        if (new == marks).all():
            return marks, rounds
        marks = new
        rounds += 1


def close_gauss_seidel(tet_edge, marks, order):
    """in place, tet after tet in `order`, each tet closed locally; (closed marks, sweeps that changed something)"""
    mk = bytearray(np.asarray(marks, np.uint8).tobytes())
    rows = [tet_edge[t].tolist() for t in order]
    sweeps = 0
    while True:
        changed = False
        for te in rows:
            m = mk[te[0]] | mk[te[1]] << 1 | mk[te[2]] << 2 | mk[te[3]] << 3 | mk[te[4]] << 4 | mk[te[5]] << 5
            add = LOCAL_CLOSE[m] & ~m
            if add:
                for s in range(6):
                    if add >> s & 1 and not mk[te[s]]:
                        mk[te[s]] = 1
                        changed = True
        if not changed:
            return np.frombuffer(bytes(mk), np.uint8).astype(bool), sweeps
        sweeps += 1


def refine(tets, points, feat, select, edges=None, tet_edge=None):
    """Refined(points_new f32 [P+M,3], feat_new f32 [P+M,K], tet_new int64 [T',4], parent int64 [T'], kind uint8 [T'], edges_split int64
    [M,2], marks bool [E], rounds).  IndexError on a tet_edge entry outside [0,E).  (ValueError on an illegal pattern: closed marks
    cannot hold one, see test_refine_ref_cpu.py.)"""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    points, feat = np.asarray(points, np.float32), np.asarray(feat, np.float32)
    P, T = points.shape[0], tets.shape[0]
    if edges is None:
        edges, tet_edge = tet_edges(tets, P)
    edges, tet_edge = np.asarray(edges, np.int64).reshape(-1, 2), np.asarray(tet_edge, np.int64).reshape(-1, 6)
    E = edges.shape[0]
    if tet_edge.size and (tet_edge.min() < 0 or tet_edge.max() >= E):
        raise IndexError("tet_edge entry outside [0, %d)" % E)
    marks, rounds = close_jacobi(tet_edge, initial_marks(tet_edge, select, E))
    pat = patterns(tet_edge, marks)
    if not IS_LEGAL[pat].all():
        raise ValueError("illegal pattern %s" % sorted(set(pat[~IS_LEGAL[pat]].tolist())))
    rank = np.cumsum(marks) - marks                                         # exclusive
    split = edges[marks]
    half = np.float32(2.0)
    points_new = np.concatenate([points, (points[split[:, 0]] + points[split[:, 1]]) / half], 0).astype(np.float32)
    feat_new = np.concatenate([feat, (feat[split[:, 0]] + feat[split[:, 1]]) / half], 0).astype(np.float32)
    n_child = N_CHILD[pat]
    start = np.cumsum(n_child) - n_child
    n_out = int(n_child.sum())
    tet_new = np.zeros((n_out, 4), np.int64)
    src = np.concatenate([tets, P + rank[tet_edge]], 1) if T else np.zeros((0, 10), np.int64)    # codes 0..3 corners, 4..9 midpoints
    for mask in LEGAL:
        rows = np.nonzero(pat == mask)[0]
        if rows.size == 0:
            continue
        code = np.asarray(CHILDREN[mask])                                   # [n,4]
        kids = src[rows][:, code]                                           # [R,n,4]
        at = start[rows][:, None] + np.arange(code.shape[0])[None]
        tet_new[at.reshape(-1)] = kids.reshape(-1, 4)
    parent = np.repeat(np.arange(T, dtype=np.int64), n_child)
    kind = POPCOUNT[pat][parent]
    return Refined(points_new, feat_new, tet_new, parent, kind, split, marks, rounds)


# ---------------------------------------------------------------------------- what the tests measure on a tet list
def face_owner_counts(tets):
    """(faces int64 [F,3] sorted rows, unique; owners int64 [F])"""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    tri = np.sort(tets[:, np.asarray(FACES)].reshape(-1, 3), 1)
    return np.unique(tri, axis=0, return_counts=True)


def one_owner_faces(tets):
    f, c = face_owner_counts(tets)
    return f[c == 1]


def volumes(points, tets):
    p = np.asarray(points, np.float64)[np.asarray(tets, np.int64)]
    return np.linalg.det(p[:, 1:] - p[:, :1]) / 6.0


def points64(points, edges_split):
    """fp64 positions of a refinement's vertices from the input's: exact midpoints, for the volume checks"""
    p = np.asarray(points, np.float64)
    return np.concatenate([p, (p[edges_split[:, 0]] + p[edges_split[:, 1]]) / 2.0], 0)


def hull_faces_subdivide(tets, res):
    """True when every one-owner face of the refinement lies inside a one-owner face of the input: its three vertices, each an
    input vertex or the midpoint of an input edge, have exactly the three corners of such a face as their ends"""
    P = res.points_new.shape[0] - res.edges_split.shape[0]
    ends = np.concatenate([np.repeat(np.arange(P, dtype=np.int64)[:, None], 2, 1), res.edges_split], 0)    # [P+M,2]
    f = one_owner_faces(res.tet_new)
    s = np.sort(ends[f].reshape(-1, 6), 1)
    lo, hi = s[:, 0], s[:, 5]
    inner = (s != lo[:, None]) & (s != hi[:, None])
    if not inner.any(1).all():
        return False
    mid = np.where(inner, s, -1).max(1)
    if not (((s == lo[:, None]) | (s == hi[:, None]) | (s == mid[:, None])).all()):
        return False
    n = np.int64(P + 1)
    key = lambda a, b, c: (a * n + b) * n + c
    have = set(key(*one_owner_faces(tets).T).tolist())
    return all(k in have for k in key(lo, mid, hi).tolist())


def occupancy_band(inside, nbr, rings=0):
    """bool [T]: tets with a face neighbour in the other state in any shape of inside [B,T] or [T], grown by `rings` face rings"""
    ins = np.asarray(inside, bool).reshape(-1, nbr.shape[0])
    has = nbr >= 0
    band = ((ins[:, np.where(has, nbr, 0)] != ins[:, :, None]) & has[None]).any((0, 2))
    for _ in range(rings):
        band = band | (band[np.where(has, nbr, 0)] & has).any(1)
    return band


def sphere_inside(points, tets, r=0.3):
    """the centroid of the tet lies within r of the centre of the points' bounding box"""
    p = np.asarray(points, np.float64)
    c = p[np.asarray(tets, np.int64)].mean(1) - (p.min(0) + p.max(0)) / 2.0
    return np.linalg.norm(c, axis=1) < r
