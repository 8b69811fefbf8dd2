"""numpy / scipy reference of the mesh components, their measures and the mesh clean-up (hip_ops.mesh_components / mesh_cleanup,
DESIGN.md §6v), in float64, for the tests.  It does not restate the kernels' traversal: edges come from np.unique over sorted
pairs, components from scipy.sparse.csgraph.connected_components on the face graph (the face-vertex bipartite graph in vertex
mode), counts from bincounts, sums from math.fsum; selection and compaction are plain numpy."""
import collections
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

Components = collections.namedtuple("Components", "labels count n_face area volume boundary_edges nonmanifold_edges misoriented_edges "
                                                  "S_area S_vol closed")
Clean = collections.namedtuple("Clean", "faces vertex_map face_map face_offsets vertex_offsets keep")


def edge_table(faces, n_vertex):
    """(edge id of every incidence [F,3], incidences per edge, per edge whether all its incidences run min -> max or all max -> min)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f, np.roll(f, -1, axis=1)                                       # local edges (f0,f1), (f1,f2), (f2,f0)
    key = np.minimum(a, b) * np.int64(n_vertex) + np.maximum(a, b)
    _uniq, inv, cnt = np.unique(key.reshape(-1), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    forward = np.bincount(inv, weights=(a < b).reshape(-1).astype(np.float64), minlength=cnt.size).astype(np.int64)
    return inv.reshape(-1, 3), cnt, (forward == cnt) | (forward == 0)


def _relabel(raw):
    """component ids -> the smallest face index of the component"""
    smallest = np.full(raw.max() + 1 if raw.size else 0, np.iinfo(np.int64).max)
    np.minimum.at(smallest, raw, np.arange(raw.size))
    return smallest[raw]


def labels(faces, n_vertex, connectivity="edge"):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    if F == 0:
        return np.zeros(0, np.int64)
    rows = np.repeat(np.arange(F), 3)
    if connectivity == "edge":
        face_edge, cnt, _same = edge_table(f, n_vertex)
        M = sp.coo_matrix((np.ones(3 * F), (rows, face_edge.reshape(-1))), shape=(F, cnt.size)).tocsr()
    elif connectivity == "vertex":
        M = sp.coo_matrix((np.ones(3 * F), (rows, f.reshape(-1))), shape=(F, n_vertex)).tocsr()
    else:
        raise ValueError(connectivity)
    n = M.shape[1]
    graph = sp.bmat([[None, M], [M.T, None]], format="csr")               # faces and their edges (vertices): bipartite
    _k, raw = connected_components(graph, directed=False)
    assert graph.shape[0] == F + n
    return _relabel(raw[:F])


def face_terms(verts, faces):
    """per face in float64 from the widened float32 positions: (area, volume, |b-a| |c-a|, |a| |b| |c|)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    s_area = np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1)
    s_vol = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) * np.linalg.norm(c, axis=1)
    return area, vol, s_area, s_vol


def components(faces, n_vertex, verts=None, connectivity="edge", face_offsets=None):
    """every per-component array stands at the label's index and is 0 elsewhere, as the operator stores them"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    foff = [0, F] if face_offsets is None else list(face_offsets)
    lab = labels(f, n_vertex, connectivity)
    n_face = np.bincount(lab, minlength=F).astype(np.int64) if F else np.zeros(0, np.int64)
    bnd, nm, mis = np.zeros(F, np.int64), np.zeros(F, np.int64), np.zeros(F, np.int64)
    if F:
        face_edge, cnt, same = edge_table(f, n_vertex)
        owner = np.zeros(cnt.size, np.int64)
        owner[face_edge.reshape(-1)] = np.repeat(lab, 3)                   # every face of an edge lies in one component
        bnd = np.bincount(owner[cnt == 1], minlength=F)
        nm = np.bincount(owner[cnt > 2], minlength=F)
        mis = np.bincount(owner[(cnt == 2) & same], minlength=F)
    roots = np.nonzero(lab == np.arange(F))[0]
    count = np.array([int(((roots >= foff[s]) & (roots < foff[s + 1])).sum()) for s in range(len(foff) - 1)], np.int64)
    area = volume = s_area = s_vol = None
    if verts is not None:
        terms = face_terms(verts, f)
        area, volume, s_area, s_vol = (np.zeros(F) for _ in range(4))
        order = np.argsort(lab, kind="stable")
        bounds = np.concatenate([[0], np.cumsum(n_face[roots])]).astype(np.int64)
        for k, r in enumerate(roots):
            mine = order[bounds[k]:bounds[k + 1]]
            area[r], volume[r], s_area[r], s_vol[r] = (math.fsum(t[mine]) for t in terms)
    closed = (n_face > 0) & (bnd == 0) & (nm == 0) & (mis == 0)
    return Components(lab, count, n_face, area, volume, bnd, nm, mis, s_area, s_vol, closed)


def cleanup(faces, n_vertex, comps, keep_largest=False, min_faces=0, min_area=0.0, drop_voids=False, largest_by="faces", face_offsets=None,
            vertex_offsets=None):
    """the selection in the operator's order and the compaction; faces' are numbered inside their shapes, the maps hold old indices"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    foff = [0, F] if face_offsets is None else list(face_offsets)
    voff = [0, n_vertex] if vertex_offsets is None else list(vertex_offsets)
    lab = comps.labels
    alive = lab == np.arange(F)
    if drop_voids:
        alive &= ~(comps.closed & (comps.volume < 0))
    if min_faces > 0:
        alive &= comps.n_face >= min_faces
    if min_area > 0:
        alive &= ~(comps.area < min_area)
    if keep_largest:
        size = comps.n_face if largest_by == "faces" else comps.area
        best = np.zeros(F, bool)
        for s in range(len(foff) - 1):
            mine = np.nonzero(alive[foff[s]:foff[s + 1]])[0] + foff[s]
            if mine.size:
                best[mine[np.argmax(size[mine])]] = True                   # argmax: the first = the smaller label among equals
        alive = best
    keep = alive[lab] if F else np.zeros(0, bool)
    face_map = np.nonzero(keep)[0]
    used = np.zeros(n_vertex, bool)
    used[f[face_map].reshape(-1)] = True
    vertex_map = np.nonzero(used)[0]
    new = np.cumsum(used) - 1
    shape = np.searchsorted(np.asarray(foff[1:]), face_map, side="right")
    before = np.concatenate([[0], np.cumsum(used)])[np.asarray(voff)]      # kept vertices before every shape
    faces_out = new[f[face_map]] - before[shape][:, None]
    fo = np.concatenate([[0], np.cumsum(keep)])[np.asarray(foff)]
    return Clean(faces_out.astype(np.int64), vertex_map.astype(np.int64), face_map.astype(np.int64), fo.astype(np.int64), before.astype(np.int64),
                 keep)
