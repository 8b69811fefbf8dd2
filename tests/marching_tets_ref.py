"""numpy restatement of marching tetrahedra (deftet_amd/csrc/marching_tets.hip), for the tests.

One shape at a time, in float32 and in the kernel's operation order, with this file's own copy of the triangle table:

    tet_edges(tets)                         unique (min,max) edges in lexicographic order, tet -> edge ids in local order
    edge_vertex_csr(edges, V)               offsets [V+1], slots [2E] = 2*e+side, ascending per vertex
    marching_tets(pos, field, tets, ...)    Mesh(verts, faces, vert_attr, edge_id, t, tet_id) of one shape
    grads32(...)                            the backward's formulas in float32
    marching_tets_torch(...)                the same vertices in torch (float64 when its inputs are), for autograd
    grads64(...)                            the gradients by float64 autograd
    grads64_terms(...), entry_bound(...)    the same by the closed formulas, with the absolute sum of every entry's terms, and
                                            the per-entry bound of a double accumulation rounded once
    forward64(...)                          t, vertices and attributes in float64 with their float32 bounds
    same_rows_nan_aware(a, b)               bit equality that takes any NaN for any NaN
    closed_and_oriented(faces, n_vert)      the watertightness check of the tests
"""
import collections

import numpy as np

LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# case code (bit k = corner k inside) -> crossing local edges in cyclic order from the lowest id; three ids are one triangle,
# four are the quad q0..q3 = triangles (q0,q1,q2), (q0,q2,q3).  Normals point from the inside corners to the outside ones on a
# positively oriented tet.
TRIANGLES = ((), (0, 1, 2), (0, 4, 3), (1, 2, 4, 3), (1, 3, 5), (0, 3, 5, 2), (0, 4, 5, 1), (2, 4, 5),
             (2, 5, 4), (0, 1, 5, 4), (0, 2, 5, 3), (1, 5, 3), (1, 3, 4, 2), (0, 3, 4), (0, 2, 1), ())

Mesh = collections.namedtuple("Mesh", "verts faces vert_attr edge_id t tet_id")


def tet_edges(tets):
    """(edges int64 [E,2], tet_edge int64 [T,6]) as hip_ops.tet_edges returns them"""
    tets = np.asarray(tets, np.int64)
    pairs = np.stack([tets[:, [a, b]] for a, b in LOCAL_EDGES], 1)               # [T,6,2]
    pairs = np.stack([pairs.min(2), pairs.max(2)], 2).reshape(-1, 2)
    edges, inv = np.unique(pairs, axis=0, return_inverse=True)                    # (lexicographic)
    return edges, inv.reshape(-1, 6)


def edge_vertex_csr(edges, n_vertex):
    ends = np.asarray(edges, np.int64).reshape(-1)                                # slot 2*e+side holds vertex ends[slot]
    order = np.argsort(ends, kind="stable")
    offsets = np.zeros(n_vertex + 1, np.int64)
    np.cumsum(np.bincount(ends, minlength=n_vertex), out=offsets[1:])
    return offsets.astype(np.int32), order.astype(np.int32)


def _crossings(field, edges, iso):
    inside = field > np.float32(iso)                                              # strict, fp32; NaN is outside
    cross = inside[edges[:, 0]] != inside[edges[:, 1]]
    return inside, cross


def marching_tets(pos, field, tets, iso=0.0, attr=None, edges=None, tet_edge=None):
    pos, field = np.asarray(pos, np.float32), np.asarray(field, np.float32)
    tets = np.asarray(tets, np.int64)
    if edges is None:
        edges, tet_edge = tet_edges(tets)
    iso32 = np.float32(iso)
    inside, cross = _crossings(field, edges, iso)
    edge_id = np.nonzero(cross)[0]
    lo, hi = edges[edge_id, 0], edges[edge_id, 1]
    with np.errstate(all="ignore"):
        t = ((iso32 - field[lo]) / (field[hi] - field[lo])).astype(np.float32)
        verts = (pos[lo] + t[:, None] * (pos[hi] - pos[lo])).astype(np.float32)
        vattr = None
        if attr is not None:
            attr = np.asarray(attr, np.float32)
            vattr = (attr[lo] + t[:, None] * (attr[hi] - attr[lo])).astype(np.float32)
    edge_vertex = -np.ones(edges.shape[0], np.int64)
    edge_vertex[edge_id] = np.arange(edge_id.size)
    code = (inside[tets] << np.arange(4)).sum(1)
    faces, tet_id = [], []
    for tt in np.nonzero((code != 0) & (code != 15))[0]:
        q = TRIANGLES[code[tt]]
        for tri in ((q[0], q[1], q[2]),) + (((q[0], q[2], q[3]),) if len(q) == 4 else ()):
            faces.append([edge_vertex[tet_edge[tt, k]] for k in tri])
            tet_id.append(tt)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return Mesh(verts, faces, vattr, edge_id.astype(np.int64), t, np.asarray(tet_id, np.int64))


def grads32(pos, field, edges, iso, g_verts, attr=None, g_attr=None):
    """(grad_pos, grad_field, grad_attr) of sum(verts * g_verts) + sum(vert_attr * g_attr) in float32 arithmetic"""
    pos, field, g_verts = np.asarray(pos, np.float32), np.asarray(field, np.float32), np.asarray(g_verts, np.float32)
    iso32 = np.float32(iso)
    _inside, cross = _crossings(field, edges, iso)
    e = np.nonzero(cross)[0]
    lo, hi = edges[e, 0], edges[e, 1]
    d = field[hi] - field[lo]
    t = (iso32 - field[lo]) / d
    one = np.float32(1)
    gp, gf = np.zeros_like(pos), np.zeros_like(field)
    np.add.at(gp, lo, (one - t)[:, None] * g_verts)
    np.add.at(gp, hi, t[:, None] * g_verts)
    s = (g_verts * (pos[hi] - pos[lo])).sum(1, dtype=np.float32)
    ga = None
    if attr is not None:
        attr, g_attr = np.asarray(attr, np.float32), np.asarray(g_attr, np.float32)
        ga = np.zeros_like(attr)
        np.add.at(ga, lo, (one - t)[:, None] * g_attr)
        np.add.at(ga, hi, t[:, None] * g_attr)
        s = s + (g_attr * (attr[hi] - attr[lo])).sum(1, dtype=np.float32)
    np.add.at(gf, lo, (iso32 - field[hi]) / (d * d) * s)
    np.add.at(gf, hi, -(iso32 - field[lo]) / (d * d) * s)
    return gp, gf, ga


def marching_tets_torch(pos, field, edges, iso=0.0, attr=None):
    """(verts, vert_attr) of one shape from torch tensors of any float dtype, differentiable in pos, field and attr"""
    import torch
    edges = torch.as_tensor(np.array(edges, np.int64), device=pos.device)
    inside = field.detach() > iso
    e = torch.nonzero(inside[edges[:, 0]] != inside[edges[:, 1]])[:, 0]
    lo, hi = edges[e, 0], edges[e, 1]
    t = (iso - field[lo]) / (field[hi] - field[lo])
    verts = pos[lo] + t[:, None] * (pos[hi] - pos[lo])
    vattr = None if attr is None else attr[lo] + t[:, None] * (attr[hi] - attr[lo])
    return verts, vattr


def grads64(pos, field, edges, iso, g_verts, attr=None, g_attr=None):
    """the same gradients by float64 autograd through marching_tets_torch: (grad_pos, grad_field, grad_attr) as float64 numpy.
    The inside test runs on the float32 field against the float32 iso, like the operator's."""
    import torch
    f32 = torch.from_numpy(np.array(field, np.float32))
    p = torch.from_numpy(np.asarray(pos, np.float64)).requires_grad_(True)
    f = f32.double().requires_grad_(True)
    a = None if attr is None else torch.from_numpy(np.asarray(attr, np.float64)).requires_grad_(True)
    v, va = marching_tets_torch(p, f, edges, float(np.float32(iso)), a)
    loss = (v * torch.from_numpy(np.asarray(g_verts, np.float64))).sum()
    if a is not None:
        loss = loss + (va * torch.from_numpy(np.asarray(g_attr, np.float64))).sum()
    if not loss.requires_grad or v.shape[0] == 0:
        return np.zeros(p.shape), np.zeros(f.shape), None if a is None else np.zeros(a.shape)
    grads = torch.autograd.grad(loss, (p, f) if a is None else (p, f, a), allow_unused=True)
    out = [np.zeros(x.shape) if g is None else g.numpy() for g, x in zip(grads, (p, f, a))]
    return out[0], out[1], (out[2] if a is not None else None)


def grads64_terms(pos, field, edges, iso, g_verts, attr=None, g_attr=None, skip=None):
    """The same gradients by the closed formulas of DESIGN.md §6l, term by term in float64 from the float32 inputs widened and
    float(float32(iso)); the inside test runs in float32 like the operator's.  ((grad_pos, grad_field, grad_attr), (S_pos, S_field,
    S_attr)): S holds, entry by entry, the sum of the absolute values of the terms that were added into it — (1-t) g and t g for
    grad_pos and grad_attr, |dt/df| sum_k |g_k (x_max - x_min)_k| over position and attribute components for grad_field.  The rows
    of g_verts / g_attr are the crossing edges in ascending id, ALL of them; `skip` (bool [E]) leaves edges out of the sums."""
    field = np.asarray(field, np.float32)
    _inside, cross = _crossings(field, edges, iso)
    e = np.nonzero(cross)[0]
    keep = np.ones(e.size, bool) if skip is None else ~np.asarray(skip, bool)[e]
    e = e[keep]
    lo, hi = edges[e, 0], edges[e, 1]
    pos, f, iso64 = np.asarray(pos, np.float32).astype(np.float64), field.astype(np.float64), float(np.float32(iso))
    d = f[hi] - f[lo]
    t = (iso64 - f[lo]) / d
    dt_lo, dt_hi = (iso64 - f[hi]) / (d * d), -(iso64 - f[lo]) / (d * d)
    absdot = np.zeros(e.size)

    def spread(x, g):
        """the two weighted sums of g into a zero array like x, their absolute sums, and this part of sum_k g_k (x_max - x_min)_k"""
        g = np.asarray(g, np.float32).astype(np.float64)[keep]
        out, S = np.zeros(x.shape), np.zeros(x.shape)
        for ends, w in ((lo, 1.0 - t), (hi, t)):
            np.add.at(out, ends, w[:, None] * g)
            np.add.at(S, ends, np.abs(w[:, None] * g))
        prod = g * (x[hi] - x[lo])
        absdot[:] += np.abs(prod).sum(1)
        return out, S, prod.sum(1)
    gp, Sp, dot = spread(pos, g_verts)
    ga = Sa = None
    if attr is not None:
        ga, Sa, dot_a = spread(np.asarray(attr, np.float32).astype(np.float64), g_attr)
        dot = dot + dot_a
    gf, Sf = np.zeros(f.shape), np.zeros(f.shape)
    for ends, dt in ((lo, dt_lo), (hi, dt_hi)):
        np.add.at(gf, ends, dt * dot)
        np.add.at(Sf, ends, np.abs(dt) * absdot)
    return (gp, gf, ga), (Sp, Sf, Sa)


def entry_bound(want, S):
    """|kernel - want| entry by entry for a kernel that works and sums in double and rounds once: 2^-24 |want| for
    the one rounding to float32, 2^-40 S for a double sum in another order than numpy's (about 28 terms at 2^-53 each is 2^-48 S:
    a factor 2^8 to spare, and 2^16 under what one float32 intermediate leaves), 2^-149 for a float32-subnormal result"""
    return 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * S + 2.0 ** -149


U32 = 2.0 ** -24


def forward64(pos, field, edges, iso, attr=None):
    """(t, verts, vert_attr) of the crossing edges in float64 from the float32 inputs, each with its float32 bound:
    4u |t| — the roundings of iso - f_min, f_max - f_min and the quotient, one u for the second order; 6u (|x_min| + |x_max|) per
    component — 3u from t, u each for the difference, the product (5u on t (x_max - x_min), at most |x_min| + |x_max| for t in
    [0,1]) and the sum.  u = 2^-24.  -> ((t, bound), (verts, bound), (vert_attr, bound) | None)"""
    field = np.asarray(field, np.float32)
    _inside, cross = _crossings(field, edges, iso)
    e = np.nonzero(cross)[0]
    lo, hi = edges[e, 0], edges[e, 1]
    f = field.astype(np.float64)
    t = (float(np.float32(iso)) - f[lo]) / (f[hi] - f[lo])

    def lerp(x):
        x = np.asarray(x, np.float32).astype(np.float64)
        return x[lo] + t[:, None] * (x[hi] - x[lo]), 6 * U32 * (np.abs(x[lo]) + np.abs(x[hi]))
    return (t, 4 * U32 * np.abs(t)), lerp(pos), (None if attr is None else lerp(attr))


def same_rows_nan_aware(a, b):
    """equal shapes and dtypes, NaN exactly where the other side has NaN (any payload, either sign), equal BYTES everywhere else"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype != np.float32:
        return False
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~na]).all())


def closed_and_oriented(faces, n_vert):
    """(every undirected edge in exactly two faces, each directed edge once, V - E + F) of a face list"""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _u, n_und = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    _v, n_dir = np.unique(d, axis=0, return_counts=True)
    return bool((n_und == 2).all()), bool((n_dir == 1).all()), int(n_vert) - int(n_und.size) + int(f.shape[0])


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("fi,fi->", np.cross(v[:, 0], v[:, 1]), v[:, 2]) / 6.0)
