"""numpy restatements of the evaluation metrics (deftet_amd/csrc/metrics.hip), for the tests.

tri_dist(points, faces, dtype): Ericson's closest point on a triangle, every (point, face) pair, in the kernel's exact operation
order — bit-identical to the kernel at float32, the geometric reference at float64.  point_to_mesh(...): the first strict minimum
over faces.  sample(...): the integer-CDF face choice and the square-root warp.  metric_block(...): eval's formulas in float64."""
import numpy as np


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _seg(a, b, p):
    """segment [a, b] against p: (squared distance, end: 0 / 1 clamped, -1 inside); arrays broadcast over [P,F]"""
    abx, aby, abz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    apx, apy, apz = p[..., 0] - a[..., 0], p[..., 1] - a[..., 1], p[..., 2] - a[..., 2]
    l2 = _dot(abx, aby, abz, abx, aby, abz)
    t = np.where(l2 > 0, _dot(apx, apy, apz, abx, aby, abz) / np.where(l2 > 0, l2, 1), 0).astype(l2.dtype)
    end = np.full(t.shape, -1)
    lo = ~(t > 0)
    hi = ~lo & (t >= 1)
    end[lo], end[hi] = 0, 1
    t = np.where(lo, 0, np.where(hi, 1, t)).astype(l2.dtype)
    dx = p[..., 0] - (a[..., 0] + t * abx)
    dy = p[..., 1] - (a[..., 1] + t * aby)
    dz = p[..., 2] - (a[..., 2] + t * abz)
    return (dx * dx + dy * dy) + dz * dz, end


def tri_dist(points, faces, dtype=np.float32):
    """points [P,3], faces [F,3,3] -> (d [P,F], type [P,F]) in `dtype`; types 0 inside, 1-3 vertex, 4 ab, 5 bc, 6 ca."""
    p = np.asarray(points, dtype)[:, None, :]
    f = np.asarray(faces, dtype)[None]
    a, b, c = f[..., 0, :], f[..., 1, :], f[..., 2, :]
    P, F = p.shape[0], f.shape[1]
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], ap[..., 0], ap[..., 1], ap[..., 2])
        d2 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], ap[..., 0], ap[..., 1], ap[..., 2])
        bp = p - b
        d3 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], bp[..., 0], bp[..., 1], bp[..., 2])
        d4 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], bp[..., 0], bp[..., 1], bp[..., 2])
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], cp[..., 0], cp[..., 1], cp[..., 2])
        d6 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], cp[..., 0], cp[..., 1], cp[..., 2])
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        shape = (P, F)
        q = np.zeros(shape + (3,), dtype)
        typ = np.full(shape, -1)
        done = np.zeros(shape, bool)

        def put(mask, val, t):
            m = mask & ~done
            q[m] = np.broadcast_to(val, shape + (3,))[m]
            typ[m] = t
            done[m] = True

        put((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, shape + (3,)), 1)
        put((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, shape + (3,)), 2)
        v = (d1 / (d1 - d3))[..., None]
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + v * ab, 4)
        put((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, shape + (3,)), 3)
        w = (d2 / (d2 - d6))[..., None]
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + w * ac, 6)
        w = (e43 / (e43 + e56))[..., None]
        put((va <= 0) & (e43 >= 0) & (e56 >= 0), b + w * (c - b), 5)
        s = (va + vb) + vc
        den = (dtype(1.0) / s)
        v, w = (vb * den)[..., None], (vc * den)[..., None]
        zero = (~(s > 0) | ~np.isfinite(v[..., 0]) | ~np.isfinite(w[..., 0])) & ~done
        put(~zero, (a + ab * v) + ac * w, 0)
        dq = p - q
        d = (dq[..., 0] * dq[..., 0] + dq[..., 1] * dq[..., 1]) + dq[..., 2] * dq[..., 2]
        zero = zero | ~np.isfinite(d)
        if zero.any():
            pb = np.broadcast_to(p, shape + (3,))
            s0, e0 = _seg(np.broadcast_to(a, shape + (3,)), np.broadcast_to(b, shape + (3,)), pb)
            s1, e1 = _seg(np.broadcast_to(b, shape + (3,)), np.broadcast_to(c, shape + (3,)), pb)
            s2, e2 = _seg(np.broadcast_to(c, shape + (3,)), np.broadcast_to(a, shape + (3,)), pb)
            m, t = s0.copy(), np.where(e0 < 0, 4, np.where(e0 == 0, 1, 2))
            u = s1 < m
            m, t = np.where(u, s1, m), np.where(u, np.where(e1 < 0, 5, np.where(e1 == 0, 2, 3)), t)
            u = s2 < m
            m, t = np.where(u, s2, m), np.where(u, np.where(e2 < 0, 6, np.where(e2 == 0, 3, 1)), t)
            d = np.where(zero, m, d).astype(dtype)
            typ = np.where(zero, t, typ)
    return d.astype(dtype), typ


def point_to_mesh(points, faces, dtype=np.float32):
    """-> (dist [P], face [P], type [P]): the first face with the strictly smallest distance; faces with a non-finite corner never
    win; no face: (+inf, -1, -1); a non-finite point: (NaN, -1, -1)."""
    points = np.asarray(points, dtype)
    faces = np.asarray(faces, dtype).reshape(-1, 3, 3)
    P = points.shape[0]
    best = np.full(P, np.inf, dtype)
    bf = np.full(P, -1, np.int64)
    bt = np.full(P, -1, np.int32)
    if faces.shape[0]:
        d, t = tri_dist(points, faces, dtype)
        d = np.where(np.isfinite(faces).all(axis=(1, 2))[None, :], d, np.nan)
        for f in range(faces.shape[0]):          # ascending, strict: the kernel's scan
            u = d[:, f] < best
            best[u], bf[u], bt[u] = d[u, f], f, t[u, f]
    bad = ~np.isfinite(points).all(axis=1)
    best[bad], bf[bad], bt[bad] = np.nan, -1, -1
    return best, bf, bt


def face_areas(faces):
    f = np.asarray(faces, np.float32).reshape(-1, 3, 3)
    e1, e2 = f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.float32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)


def tickets(areas):
    """the integer quantisation: the largest area gets 2^24 tickets, every other positive area max(1, trunc(a * (2^24 / amax)))"""
    a = np.asarray(areas, np.float32)
    a = np.where(np.isfinite(a) & (a > 0), a, np.float32(0))
    if not (a > 0).any():
        return np.zeros(a.shape, np.int64)
    s = np.float32(16777216.0) / a.max()
    t = np.where(a > 0, np.maximum(1, (a * s).astype(np.int64)), 0)
    return t.astype(np.int64)


def sample(faces, uniforms, areas=None):
    """faces [F,3,3], uniforms [N,3] -> (points f32 [N,3], choice int64 [N]); None when there is nothing to sample"""
    f = np.asarray(faces, np.float32).reshape(-1, 3, 3)
    u = np.asarray(uniforms, np.float32)
    cum = np.cumsum(tickets(face_areas(f) if areas is None else areas))
    T = int(cum[-1]) if cum.size else 0
    if T == 0:
        return None
    u0 = u[:, 0].astype(np.float64)
    t = np.floor(u0 * float(T))
    t = np.where(~(u[:, 0] > 0), 0, np.where(u[:, 0] >= 1, T - 1, np.minimum(t, T - 1))).astype(np.int64)
    choice = np.searchsorted(cum, t, side="right").astype(np.int64)      # first f with cum[f] > t
    s = np.sqrt(u[:, 1])
    wa, wb, wc = np.float32(1) - s, s * (np.float32(1) - u[:, 2]), s * u[:, 2]
    tri = f[choice]
    pts = (wa[:, None] * tri[:, 0] + wb[:, None] * tri[:, 1]) + wc[:, None] * tri[:, 2]
    return pts.astype(np.float32), choice


def metric_block(s1, s2, dist_a=None, dist_b=None, radius=0.01, esp=1e-15):
    """eval.py's formulas in float64 on one shape's clouds s1 (ground truth) [N1,3] and s2 (prediction) [N2,3]"""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    d12 = ((s1[:, None, :] - s2[None]) ** 2).sum(-1)
    d21 = d12.T
    i12, i21 = d12.argmin(1), d21.argmin(1)
    pd, gd = np.sqrt(d12.min(1) + esp), np.sqrt(d21.min(1) + esp)
    precision = (gd <= radius).sum() / gd.size
    recall = (pd <= radius).sum() / pd.size
    out = {"chamfer": (pd.mean() + gd.mean()) / 2,
           "chamfer_l1": np.abs(s1 - s2[i12]).sum(-1).mean() + np.abs(s2 - s1[i21]).sum(-1).mean(),
           "f_score": 2 * (precision * recall) / (precision + recall + 1e-8)}
    if dist_a is not None:
        sa, sb = np.sqrt(np.asarray(dist_a, np.float64) + esp), np.sqrt(np.asarray(dist_b, np.float64) + esp)
        out["mean_hausdorff"] = ((sa + sb) / 2).mean()
        out["max_hausdorff"] = (sa.max() + sb.max()) / 2
    return out
