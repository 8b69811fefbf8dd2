"""Numpy restatement of the ground-truth preparation stages, written from the rules in include/deftet_hip.h, not
from the kernels: conservative voxelization (fp32 in the stated operation order, and fp64 with every decision's margin), depth
maps, their projection, the cuberille surface and the unique edges of a triangle list.  PARITY UNPINNED against Kaolin."""
import numpy as np


def default_frame(vertices, dtype=np.float32):
    """origin [B,3] = the per-shape minimum, scale [B] = the largest per-shape extent"""
    v = np.asarray(vertices, dtype)
    mn, mx = v.min(axis=1), v.max(axis=1)
    return mn, (mx - mn).max(axis=1)


def _box_axes(a, h):
    """the three box axes of _axis_margins"""
    out = []
    for c in range(3):
        mn, mx = np.minimum(np.minimum(a[0, c], a[1, c]), a[2, c]), np.maximum(np.maximum(a[0, c], a[1, c]), a[2, c])
        out.append((np.maximum(mn - h, -h - mx), a.dtype.type(1)))
    return out


def _axis_margins(a, e, h, xp_abs=np.abs):
    """a [3 corners, 3, n] relative to the voxel centres, e [3 edges, 3] -> list of (separation, axis length) per axis; the voxel
    and the triangle are separated on an axis iff its separation is > 0.  Every product and sum is one rounded operation."""
    out = _box_axes(a, h)
    nx, ny, nz = e[0, 1] * e[1, 2] - e[0, 2] * e[1, 1], e[0, 2] * e[1, 0] - e[0, 0] * e[1, 2], e[0, 0] * e[1, 1] - e[0, 1] * e[1, 0]
    d = (nx * a[0, 0] + ny * a[0, 1]) + nz * a[0, 2]
    out.append((np.abs(d) - h * ((abs(nx) + abs(ny)) + abs(nz)), np.sqrt(nx * nx + ny * ny + nz * nz)))
    for i in range(3):
        for j in range(3):
            u, v = (j + 1) % 3, (j + 2) % 3
            p = [e[i, v] * a[m, u] - e[i, u] * a[m, v] for m in range(3)]
            r = h * (abs(e[i, v]) + abs(e[i, u]))
            mn, mx = np.minimum(np.minimum(p[0], p[1]), p[2]), np.maximum(np.maximum(p[0], p[1]), p[2])
            out.append((np.maximum(mn - r, -r - mx), np.sqrt(e[i, v] * e[i, v] + e[i, u] * e[i, u])))
    return out


def _voxelize(vertices, faces, R, origin, scale, dtype, want_margin):
    v = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    B = v.shape[0]
    if origin is None or scale is None:
        o0, s0 = default_frame(v, np.float32)
        origin = o0 if origin is None else origin
        scale = s0 if scale is None else scale
    origin, scale = np.asarray(origin, np.float32).astype(dtype), np.asarray(scale, np.float32).astype(dtype)
    vox = np.zeros((B, R, R, R), np.uint8)
    near = np.zeros((B, R, R, R), bool) if want_margin else None
    h, Rt = dtype(0.5), dtype(R)
    with np.errstate(all="ignore"):
        for b in range(B):
            q_all = ((v[b].astype(dtype) - origin[b][None, :]) / scale[b]) * Rt
            for f in faces:
                if (f < 0).any() or (f >= v.shape[1]).any():
                    continue
                q = q_all[f]                                             # [3 corners, 3]
                if not np.isfinite(q).all():
                    continue
                lo = np.maximum(np.ceil(np.clip(q.min(axis=0), -1, R + 1)).astype(np.int64) - 1, 0)
                hi = np.minimum(np.floor(np.clip(q.max(axis=0), -1, R + 1)).astype(np.int64), R - 1)
                if want_margin:                                         # one more ring: decisions just outside the candidate rule
                    lo, hi = np.maximum(lo - 1, 0), np.minimum(hi + 1, R - 1)
                if (lo > hi).any():
                    continue
                ii, jj, kk = np.meshgrid(*[np.arange(lo[c], hi[c] + 1) for c in range(3)], indexing="ij")
                idx = np.stack([ii.ravel(), jj.ravel(), kk.ravel()])    # [3, n]
                centre = idx.astype(dtype) + h
                a = q[:, :, None] - centre[None, :, :]
                e = np.stack([q[1] - q[0], q[2] - q[1], q[0] - q[2]])
                axes = _axis_margins(a, e, h)
                sep = np.zeros(idx.shape[1], bool)
                for s, _ in axes:
                    sep |= s > 0
                hit = ~sep
                vox[b, idx[0][hit], idx[1][hit], idx[2][hit]] = 1
                if want_margin:
                    # the decision flips when the largest separation (in voxel units: divided by the axis length) crosses zero
                    worst = np.full(idx.shape[1], -np.inf)
                    for s, length in axes:
                        if length > 0:
                            worst = np.maximum(worst, s / length)
                    close = np.abs(worst) < want_margin
                    near[b, idx[0][close], idx[1][close], idx[2][close]] = True
    return (vox, near) if want_margin else vox


def _frame(v, origin, scale, dtype):
    if origin is None or scale is None:
        o0, s0 = default_frame(v, np.float32)
        origin = o0 if origin is None else origin
        scale = s0 if scale is None else scale
    return np.asarray(origin, np.float32).astype(dtype), np.asarray(scale, np.float32).astype(dtype)


def _candidate_boxes(q, faces, n_vertex, R, ring):
    """q [V,3] in voxel units, faces int64 [F,3] -> (corners [F,3 corners,3], lo, hi int64 [F,3] inclusive, ok bool [F]): the
    candidate rule of include/deftet_hip.h for every triangle at once (`ring`: one more voxel on every side, as the fp64 margin
    pass looks); ok is False for a face index outside [0,V), a non-finite corner and an empty box"""
    valid = ((faces >= 0) & (faces < n_vertex)).all(axis=1)
    qf = q[np.where(valid[:, None], faces, 0)]
    ok = valid & np.isfinite(qf).all(axis=(1, 2))
    qf = np.where(ok[:, None, None], qf, q.dtype.type(0))
    lo = np.maximum(np.ceil(np.clip(qf.min(axis=1), -1, R + 1)).astype(np.int64) - 1, 0)
    hi = np.minimum(np.floor(np.clip(qf.max(axis=1), -1, R + 1)).astype(np.int64), R - 1)
    if ring:
        lo, hi = np.maximum(lo - 1, 0), np.minimum(hi + 1, R - 1)
    return qf, lo, hi, ok & (lo <= hi).all(axis=1)


def _voxelize_flat(vertices, faces, R, origin, scale, dtype, want_margin, chunk=1 << 19):
    """_voxelize without the loop over the triangles: the same rule, the same operations in the same order, over flat
    (triangle, voxel) pairs, `chunk` of them at a time.  Pinned bit for bit to the loop in test_dataprep_cases_cpu.py."""
    v = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    B = v.shape[0]
    origin, scale = _frame(v, origin, scale, dtype)
    vox = np.zeros((B, R, R, R), np.uint8)
    near = np.zeros((B, R, R, R), bool) if want_margin else None
    h, Rt = dtype(0.5), dtype(R)
    with np.errstate(all="ignore"):
        for b in range(B):
            q_all = ((v[b].astype(dtype) - origin[b][None, :]) / scale[b]) * Rt
            qf, lo, hi, ok = _candidate_boxes(q_all, faces, v.shape[1], R, bool(want_margin))
            ext = np.where(ok[:, None], hi - lo + 1, 0)
            sel = np.flatnonzero(ext.prod(axis=1))
            ends = np.cumsum(ext[sel].prod(axis=1))
            first = 0
            while first < sel.shape[0]:
                done = ends[first - 1] if first else 0
                last = max(int(np.searchsorted(ends, done + chunk, side="right")), first + 1)
                fs = sel[first:last]
                first = last
                n_f = ext[fs].prod(axis=1)
                own = np.repeat(np.arange(fs.shape[0]), n_f)            # the pair's triangle, and its place in that triangle's box
                local = np.arange(int(n_f.sum())) - np.repeat(np.cumsum(n_f) - n_f, n_f)
                ny, nz = ext[fs, 1][own], ext[fs, 2][own]
                idx = np.stack([lo[fs, 0][own] + local // (ny * nz), lo[fs, 1][own] + (local // nz) % ny, lo[fs, 2][own] + local % nz])
                qt = qf[fs]                                             # [m, 3 corners, 3]
                centre = idx.astype(dtype) + h
                a = np.moveaxis(qt, 0, -1)[:, :, own] - centre[None, :, :]
                # a pair that a box axis separates by the margin or more (fp32: at all) is neither set nor near, whatever the
                # ten other axes say: most of the candidate box, and nearly all of its ring
                cut = np.zeros(idx.shape[1], bool)
                for s, _ in _box_axes(a, h):
                    cut |= (s >= want_margin) if want_margin else (s > 0)
                keep = np.flatnonzero(~cut)
                idx, a, own = idx[:, keep], a[:, :, keep], own[keep]
                e = np.moveaxis(np.stack([qt[:, 1] - qt[:, 0], qt[:, 2] - qt[:, 1], qt[:, 0] - qt[:, 2]]), 1, -1)[:, :, own]
                axes = _axis_margins(a, e, h)
                sep = np.zeros(idx.shape[1], bool)
                for s, _ in axes:
                    sep |= s > 0
                hit = ~sep
                vox[b, idx[0][hit], idx[1][hit], idx[2][hit]] = 1
                if want_margin:
                    worst = np.full(idx.shape[1], -np.inf)
                    for s, length in axes:
                        worst = np.where(length > 0, np.maximum(worst, s / length), worst)
                    close = np.abs(worst) < want_margin
                    near[b, idx[0][close], idx[1][close], idx[2][close]] = True
    return (vox, near) if want_margin else vox


def mesh_voxelize_f32(vertices, faces, R, origin=None, scale=None, flat=False):
    """uint8 [B,R,R,R]: the rule evaluated in fp32 in the stated operation order (`flat`: by the vectorised evaluator)"""
    return (_voxelize_flat if flat else _voxelize)(vertices, faces, R, origin, scale, np.float32, None)


def mesh_voxelize_f64(vertices, faces, R, origin=None, scale=None, margin=1e-4, flat=False):
    """(uint8 [B,R,R,R], bool [B,R,R,R]) in fp64; the second grid marks the voxels with a (triangle, voxel) decision whose smallest
    separating margin, in voxel units, is below `margin` — where an fp32 evaluation may decide the other way"""
    return (_voxelize_flat if flat else _voxelize)(vertices, faces, R, origin, scale, np.float64, margin)


def voxelize_tasks(vertices, faces, R, origin=None, scale=None, budget=256):
    """int64 [B,F]: the wave tasks of every triangle (include/deftet_hip.h): its candidate box in fp32 has (i extent) (j extent)
    (words of k it touches) word columns, a task is `budget` (DEFTET_VOXELIZE_UNIT_BUDGET) of them; a triangle with a bad index,
    a non-finite corner or an empty box has none.  stats = (tasks.sum(), (tasks > 1).sum(), 0, 0) when no index is bad."""
    v = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    origin, scale = _frame(v, origin, scale, np.float32)
    out = np.zeros((v.shape[0], faces.shape[0]), np.int64)
    with np.errstate(all="ignore"):
        for b in range(v.shape[0]):
            q_all = ((v[b] - origin[b][None, :]) / scale[b]) * np.float32(R)
            _, lo, hi, ok = _candidate_boxes(q_all, faces, v.shape[1], R, False)
            units = (hi[:, 0] - lo[:, 0] + 1) * (hi[:, 1] - lo[:, 1] + 1) * ((hi[:, 2] >> 5) - (lo[:, 2] >> 5) + 1)
            out[b] = np.where(ok, (units + budget - 1) // budget, 0)
    return out


# ---------------------------------------------------------------------------- depth maps
def extract_odms(vox):
    """int32 [B,6,R,R]: direction d scans axis d // 2 (ascending for even d), maps indexed by the two other axes ascending"""
    v = np.asarray(vox) != 0
    B, R = v.shape[0], v.shape[1]
    out = np.empty((B, 6, R, R), np.int32)
    for a in range(3):
        m = np.moveaxis(v, a + 1, -1)                                   # [B, p, q, scan]
        for rev in range(2):
            s = m[..., ::-1] if rev else m
            out[:, 2 * a + rev] = np.where(s.any(axis=-1), s.argmax(axis=-1), R)
    return out


def project_odms(odms, voxelgrids=None, votes=1):
    odms = np.asarray(odms)
    B, R = odms.shape[0], odms.shape[2]
    carved = np.zeros((B, R, R, R), np.int32)
    x = np.arange(R)
    for a in range(3):
        for rev in range(2):
            depth = odms[:, 2 * a + rev]                                # [B, p, q]
            pos = (R - 1 - x) if rev else x
            c = pos[None, None, None, :] < depth[..., None]             # [B, p, q, scan]
            carved += np.moveaxis(c, -1, a + 1)
    start = np.ones((B, R, R, R), bool) if voxelgrids is None else (np.asarray(voxelgrids) != 0)
    return (start & (carved < votes)).astype(np.uint8)


# ---------------------------------------------------------------------------- cuberille
def voxel_surface_mesh(vox, iso_value=0.5):
    """(list of verts f32 [V_b,3], list of faces int64 [F_b,3]): include/deftet_hip.h, deftet_voxel_surface_count_b32"""
    vox = np.asarray(vox)
    occ_all = vox > iso_value
    B, R = vox.shape[0], vox.shape[1]
    verts_out, faces_out = [], []
    for b in range(B):
        occ = np.zeros((R + 2,) * 3, bool)
        occ[1:-1, 1:-1, 1:-1] = occ_all[b]
        rows = []                                                       # (voxel linear index, direction, triangle, 3 corner keys)
        for d in range(6):
            a, plus = d // 2, d % 2
            u, v = (a + 1) % 3, (a + 2) % 3
            shift = np.roll(occ, -1 if plus else 1, axis=a)             # the neighbour towards the direction
            idx = np.argwhere(occ[1:-1, 1:-1, 1:-1] & ~shift[1:-1, 1:-1, 1:-1])
            if idx.shape[0] == 0:
                continue
            p00 = idx.copy()
            p00[:, a] += plus
            eu, ev = np.eye(3, dtype=np.int64)[u], np.eye(3, dtype=np.int64)[v]
            p10, p01, p11 = p00 + eu, p00 + ev, p00 + eu + ev
            key = lambda p: (p[:, 0] * (R + 1) + p[:, 1]) * (R + 1) + p[:, 2]
            lin = (idx[:, 0] * R + idx[:, 1]) * R + idx[:, 2]
            tris = ((p00, p10, p11), (p00, p11, p01)) if plus else ((p00, p01, p11), (p00, p11, p10))
            for t, tri in enumerate(tris):
                rows.append(np.stack([lin, np.full_like(lin, d), np.full_like(lin, t), key(tri[0]), key(tri[1]), key(tri[2])], axis=1))
        if not rows:
            verts_out.append(np.zeros((0, 3), np.float32))
            faces_out.append(np.zeros((0, 3), np.int64))
            continue
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        keys, inv = np.unique(rows[:, 3:], return_inverse=True)
        faces_out.append(inv.reshape(-1, 3).astype(np.int64))
        R1 = R + 1
        verts_out.append(np.stack([keys // (R1 * R1), (keys // R1) % R1, keys % R1], axis=1).astype(np.float32))
    return verts_out, faces_out


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def directed_edge_imbalance(faces):
    """number of directed edges (a, b) whose count differs from that of (b, a): 0 for a closed, consistently wound mesh"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return 0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    fwd, cf = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    bwd, cb = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    if fwd.shape != bwd.shape or not np.array_equal(fwd, bwd):
        return int(np.setxor1d(fwd, bwd).size) or 1
    return int((cf != cb).sum())


# ---------------------------------------------------------------------------- edges and smoothing
def face_edges(faces, n_vertex):
    """sorted unique directed pairs (a, b), a != b: int64 [n,2]"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 0]], f[:, [1, 2]], f[:, [2, 1]], f[:, [2, 0]], f[:, [0, 2]]])
    e = e[e[:, 0] != e[:, 1]]
    k = np.unique(e[:, 0] * n_vertex + e[:, 1])
    return np.stack([k // n_vertex, k % n_vertex], axis=1)


def edge_csr(faces, n_vertex):
    """(offsets int64 [V+1], cols int64 [n]) of face_edges"""
    p = face_edges(faces, n_vertex)
    return np.concatenate([[0], np.cumsum(np.bincount(p[:, 0], minlength=n_vertex))]), p[:, 1]


def smooth(verts, faces, iterations):
    """float64 neighbour mean, `iterations` times"""
    x = np.asarray(verts, np.float64)
    p = face_edges(faces, x.shape[0])
    deg = np.bincount(p[:, 0], minlength=x.shape[0]).astype(np.float64)
    for _ in range(iterations):
        s = np.zeros_like(x)
        np.add.at(s, p[:, 0], x[p[:, 1]])
        x = s / deg[:, None]
    return x


# ---------------------------------------------------------------------------- inputs
def icosphere(subdivisions=2, seed=0, radius=0.4, jitter=0.05):
    """an icosphere-like closed mesh: the subdivided icosahedron pushed to a sphere, its vertices jittered along the radius (by
    up to `jitter` of it; 0: a true sphere) and
    the whole turned by a random rotation (general floats, no face in a lattice plane): (verts f32 [V,3], faces int64 [F,3])"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    v = np.asarray(v) * (1.0 + jitter * rng.uniform(-1, 1, (len(v), 1)))
    return (radius * v @ q.T).astype(np.float32), np.asarray(f, np.int64)
