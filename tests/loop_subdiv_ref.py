"""Loop subdivision restated in numpy / scipy, float64, from a plain face list.  Written from the rules, not
from the kernels' traversal: the edges come from np.unique over the (min,max) pairs, the per-vertex classification from
bincounts, and the operator is ASSEMBLED as a sparse matrix S [(V+E) x V] (and L [V x V] for the limit positions) that the
tests multiply in float64.

Rules (Warren's weights).  An edge with a number of (face, local edge) incidences other than 2 is a crease; a vertex with no
crease edge is smooth (kind 0), with exactly two a crease vertex (kind 1), otherwise a corner (kind 2).
  edge vertex  interior (a,b), opposite corners (c,d): 3/8 (a+b) + 1/8 (c+d);  crease: 1/2 (a+b)
  old vertex   smooth of valence n: (1 - n beta) v + beta sum of neighbours, beta = 3/16 (n = 3) or 3/(8n);  n = 0: v
               crease: 3/4 v + 1/8 (the two crease neighbours);  corner: v
  limit        smooth: (1 - n gamma) v + gamma sum, gamma = 1/(n + 3/(8 beta));  crease: 2/3 v + 1/6 (the two);  corner: v
"""
import collections

import numpy as np
import scipy.sparse as sp

Topology = collections.namedtuple(
    "Topology", "faces n_vertex edges face_edge edge_nface edge_opp vertex_kind crease_nbr ev_offsets ev_slots fv_offsets fv_slots child_faces")

LOCAL = ((0, 1), (1, 2), (2, 0))


def beta(n):
    return 3.0 / 16.0 if n == 3 else 3.0 / (8.0 * n)


def gamma(n):
    return 1.0 / (n + 3.0 / (8.0 * beta(n)))


def topology(faces, n_vertex):
    """every table of hip_ops.LoopTopology, as numpy arrays of the same dtypes"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = faces.shape[0], int(n_vertex)
    assert F > 0 and V > 0 and faces.min() >= 0 and faces.max() < V
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 2] != faces[:, 0]).all()
    ends = np.stack([faces[:, [i, j]] for i, j in LOCAL], 1).reshape(-1, 2)             # row 3 f + k
    pairs = np.sort(ends, 1)
    edges, inverse, counts = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)   # lexicographic
    inverse = np.asarray(inverse).reshape(-1)
    E = edges.shape[0]
    face_edge = inverse.reshape(F, 3)
    opposite = faces[:, [2, 0, 1]].reshape(-1)                                           # of incidence 3 f + k
    edge_opp = np.full((E, 2), -1, np.int64)
    by_edge = np.argsort(inverse, kind="stable")                                         # incidences grouped by edge, ascending id inside
    start = np.concatenate([[0], np.cumsum(counts)])
    two = np.nonzero(counts == 2)[0]
    edge_opp[two, 0] = opposite[by_edge[start[two]]]
    edge_opp[two, 1] = opposite[by_edge[start[two] + 1]]
    crease = counts != 2
    n_crease = np.bincount(edges[crease].reshape(-1), minlength=V)
    kind = np.where(n_crease == 0, 0, np.where(n_crease == 2, 1, 2)).astype(np.uint8)
    crease_nbr = np.full((V, 2), -1, np.int64)
    fill = np.zeros(V, np.int64)
    for e in np.nonzero(crease)[0]:                                                      # ascending edge id
        a, b = edges[e]
        for v, far in ((a, b), (b, a)):
            if kind[v] == 1:
                crease_nbr[v, fill[v]] = far
                fill[v] += 1
    ev_offsets, ev_slots = incidence_csr(edges, V)
    fv_offsets, fv_slots = incidence_csr(faces, V)
    m = V + face_edge
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    mab, mbc, mca = m[:, 0], m[:, 1], m[:, 2]
    child = np.stack([np.stack(t, 1) for t in ((a, mab, mca), (b, mbc, mab), (c, mca, mbc), (mab, mbc, mca))], 1).reshape(-1, 3)
    return Topology(faces, V, edges.astype(np.int32), face_edge.astype(np.int32), counts.astype(np.int32), edge_opp.astype(np.int32), kind,
                    crease_nbr.astype(np.int32), ev_offsets, ev_slots, fv_offsets, fv_slots, child.astype(np.int64))


def incidence_csr(elements, n_vertex):
    """(offsets int32 [V+1], slots int32 [n]): per vertex the flat positions corners * e + corner that name it, ascending"""
    flat = np.asarray(elements).reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_vertex))])
    return offsets.astype(np.int32), order.astype(np.int32)


def _neighbours(top):
    nb = [[] for _ in range(top.n_vertex)]
    for a, b in top.edges:
        nb[a].append(int(b))
        nb[b].append(int(a))
    return nb


def _old_vertex_rows(top, smooth_nb, crease_own, crease_nb):
    """the [V x V] block of the old-vertex rule: smooth_nb(n) the neighbour weight of a smooth vertex of valence n"""
    rows, cols, vals = [], [], []
    nb = _neighbours(top)
    for v in range(top.n_vertex):
        k = int(top.vertex_kind[v])
        if k == 0:
            n = len(nb[v])
            w = smooth_nb(n) if n else 0.0
            rows += [v] * (n + 1)
            cols += [v] + nb[v]
            vals += [1.0 - n * w] + [w] * n
        elif k == 1:
            rows += [v] * 3
            cols += [v, int(top.crease_nbr[v, 0]), int(top.crease_nbr[v, 1])]
            vals += [crease_own, crease_nb, crease_nb]
        else:
            rows.append(v)
            cols.append(v)
            vals.append(1.0)
    return rows, cols, vals


def subdivision_matrix(top):
    """S [(V+E) x V] in CSR, float64; duplicates (an opposite corner named twice) are summed"""
    V, E = top.n_vertex, top.edges.shape[0]
    rows, cols, vals = _old_vertex_rows(top, beta, 0.75, 0.125)
    for e in range(E):
        a, b = (int(x) for x in top.edges[e])
        if top.edge_nface[e] == 2:
            c, d = (int(x) for x in top.edge_opp[e])
            rows += [V + e] * 4
            cols += [a, b, c, d]
            vals += [0.375, 0.375, 0.125, 0.125]
        else:
            rows += [V + e] * 2
            cols += [a, b]
            vals += [0.5, 0.5]
    S = sp.coo_matrix((np.array(vals, np.float64), (rows, cols)), shape=(V + E, V)).tocsr()
    S.sum_duplicates()
    return S


def limit_matrix(top):
    V = top.n_vertex
    rows, cols, vals = _old_vertex_rows(top, gamma, 2.0 / 3.0, 1.0 / 6.0)
    return sp.coo_matrix((np.array(vals, np.float64), (rows, cols)), shape=(V, V)).tocsr()


def forward_bound(M, x):
    """(nnz_row + 3) 2^-24 (|M| |x|) per output component: the forward bound of an fp32 dot product with fp32-rounded weights"""
    nnz = np.diff(M.tocsr().indptr).astype(np.float64)
    return (nnz[:, None] + 3.0) * 2.0 ** -24 * (abs(M) @ np.abs(np.asarray(x, np.float64)))


def backward_bound(M, g):
    """(nnz_col + 3) 2^-24 (|M|^T |g|) per input component: the same bound for the transpose"""
    nnz = np.diff(M.tocsc().indptr).astype(np.float64)
    return (nnz[:, None] + 3.0) * 2.0 ** -24 * (abs(M).T @ np.abs(np.asarray(g, np.float64)))


def subdivide(verts, faces, levels=1):
    """float64 (verts, faces) after `levels` rounds, and the product of the matrices"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    total = None
    for _ in range(levels):
        top = topology(faces, verts.shape[0])
        S = subdivision_matrix(top)
        verts, faces = S @ verts, top.child_faces
        total = S if total is None else S @ total
    return verts, faces, total


def edge_face_counts(faces):
    pairs = np.sort(np.stack([faces[:, [i, j]] for i, j in LOCAL], 1).reshape(-1, 2), 1)
    _e, counts = np.unique(pairs, axis=0, return_counts=True)
    return counts


def euler(faces, n_vertex):
    used = np.unique(faces).shape[0]
    return used - edge_face_counts(faces).shape[0] + faces.shape[0]


def one_ring_matrix(n):
    """the (n+1) x (n+1) subdivision matrix of a smooth vertex of valence n and its ring (row 0 the vertex, rows 1..n the edge
    vertices of its spokes, which are the ring of the next level)"""
    M = np.zeros((n + 1, n + 1))
    b = beta(n)
    M[0, 0], M[0, 1:] = 1.0 - n * b, b
    for i in range(n):
        M[1 + i, 0] += 0.375
        M[1 + i, 1 + i] += 0.375
        M[1 + i, 1 + (i + 1) % n] += 0.125
        M[1 + i, 1 + (i - 1) % n] += 0.125
    return M
