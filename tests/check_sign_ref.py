"""A plain fp64 reference for check_sign that has no ray in it: the generalised winding number of a closed
mesh (Van Oosterom-Strackee), the meshes and points the size tests use, and the rule that says at which
points ray parity itself is ill-posed.  Shared by test_check_sign_ref_cpu.py (which checks THIS file and
that the inputs are fair) and test_check_sign_sizes_gpu.py.  Everything is vectorised: a Python loop per
face is too slow at a million faces.  Mesh makers return float32 verts [V,3] and int64 faces [F,3],
outward oriented."""
import numpy as np

EDGE_TOL = 1e-4        # barycentric units: a crossing this close to an edge of its face is forgiven
T_TOL = 1e-4           # ... or this close to the ray's origin
T_BACK = -1e-3         # faces further behind the point than this are not looked at
DEAD_A = 2e-7          # the contract's dead zone |a| < 1e-7, with a factor 2 for the fp32 rounding of a
NEAR_OFFSET = 2e-3     # near-surface points: this far from the face, along its normal


# ------------------------------------------------------------------------------------------ meshes
def sphere_faces_of(n_lat):
    return 4 * n_lat * (n_lat - 1)


def uv_sphere(n_lat, radius=0.4, center=(0.0, 0.0, 0.0), flip=False):
    """n_lat - 1 rings of 2 n_lat vertices and ONE vertex per pole (two fans of valence 2 n_lat):
    4 n_lat (n_lat - 1) faces."""
    n_lon = 2 * n_lat
    th = np.pi * np.arange(1, n_lat, dtype=np.float64) / n_lat
    ph = 2.0 * np.pi * np.arange(n_lon, dtype=np.float64) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.repeat(np.cos(th)[:, None], n_lon, 1)], -1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]]) * radius + np.asarray(center, np.float64)
    s = np.arange(n_lon, dtype=np.int64)
    s1 = (s + 1) % n_lon
    last = v.shape[0] - 1
    top = np.stack([np.zeros(n_lon, np.int64), 1 + s, 1 + s1], 1)
    r0 = (1 + np.arange(n_lat - 2, dtype=np.int64) * n_lon)[:, None]
    a, b, c, d = r0 + s[None], r0 + n_lon + s[None], r0 + n_lon + s1[None], r0 + s1[None]
    mid = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
    rl = 1 + (n_lat - 2) * n_lon
    bot = np.stack([np.full(n_lon, last, np.int64), rl + s1, rl + s], 1)
    f = np.concatenate([top, mid, bot])
    if flip:
        f = f[:, ::-1]
    return v.astype(np.float32), np.ascontiguousarray(f)


def torus(n_u, n_v, R=0.3, r=0.1):
    """genus 1, 2 n_u n_v faces; a line meets it up to 4 times"""
    u = 2.0 * np.pi * np.arange(n_u, dtype=np.float64) / n_u
    w = 2.0 * np.pi * np.arange(n_v, dtype=np.float64) / n_v
    rho = R + r * np.cos(w)[None]
    v = np.stack([rho * np.cos(u)[:, None], rho * np.sin(u)[:, None], np.repeat(r * np.sin(w)[None], n_u, 0)], -1).reshape(-1, 3)
    i = np.arange(n_u, dtype=np.int64)[:, None]
    j = np.arange(n_v, dtype=np.int64)[None]
    i1, j1 = (i + 1) % n_u, (j + 1) % n_v
    a, b, c, d = i * n_v + j, i1 * n_v + j, i1 * n_v + j1, i * n_v + j1
    f = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
    return v.astype(np.float32), np.ascontiguousarray(f)


def join(*meshes):
    vs, fs, at = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + at)
        at += v.shape[0]
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int64)


SHELL_R = (0.4, 0.2)


def shell(n_lat):
    """an outer sphere and an inner one with reversed faces: inside means between them"""
    return join(uv_sphere(n_lat, SHELL_R[0]), uv_sphere(n_lat, SHELL_R[1], flip=True))


CUBE_H, MIXED_R = 0.45, 0.25


def cube(h=CUBE_H):
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)       # index 4 x + 2 y + z
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]         # -x +x -y +y -z +z, outward
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int64)
    return v, f


def mixed(n_lat):
    """a fine sphere inside a 12-face cube as ONE mesh: the fine faces set the grid size, so a cube face spans far
    more cells than a binned face may and lands in the list that every point tests"""
    return join(uv_sphere(n_lat, MIXED_R), cube())


def rotation(seed):
    """a seeded random orthogonal matrix with determinant +1, so that outward stays outward"""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rotate(verts, seed):
    """a seeded random orthogonal matrix applied in fp64, then rounded to fp32.  (Unrotated UV rings lie in planes
    z = const: a special case for a +x ray.)"""
    return (np.asarray(verts, np.float64) @ rotation(seed).T).astype(np.float32)


def signed_volume(verts, faces):
    t = np.asarray(verts, np.float64)[faces]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


# ------------------------------------------------------------------------------------------ points
def uniform_points(verts, n, seed, grow=0.25):
    """uniform in the box of the mesh enlarged by 25 %"""
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * (1.0 + grow)
    return (c + h * (2.0 * np.random.default_rng(seed).random((n, 3)) - 1.0)).astype(np.float32)


def near_surface_points(verts, faces, n, seed, offset=NEAR_OFFSET):
    """an area-random surface point moved +-offset along the normal of its face"""
    rng = np.random.default_rng(seed)
    t = np.asarray(verts, np.float64)[faces]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    k = rng.choice(faces.shape[0], size=n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    fold = a + b > 1.0
    a, b = np.where(fold, 1.0 - a, a), np.where(fold, 1.0 - b, b)
    p = t[k, 0] + a[:, None] * (t[k, 1] - t[k, 0]) + b[:, None] * (t[k, 2] - t[k, 0])
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return (p + (sgn * offset)[:, None] * nrm[k] / area[k, None]).astype(np.float32)


def points_for(verts, faces, n_uniform, n_near, seed):
    return np.concatenate([uniform_points(verts, n_uniform, seed), near_surface_points(verts, faces, n_near, seed + 1)])


# ------------------------------------------------------------------------------------------ fp64 reference
def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _f64(x, like):
    """x as float64 of the kind (numpy / torch on its device) of `like`"""
    if _is_torch(like):
        import torch
        return torch.as_tensor(x).to(device=like.device, dtype=torch.float64)
    return np.asarray(x, np.float64)


def _planes(verts, faces, pts):
    """the nine [1,F] coordinate planes of the three corners and the three [P,1] of the points, in float64"""
    v = _f64(verts, pts)
    p = _f64(pts, pts)
    if _is_torch(pts):
        import torch
        faces = torch.as_tensor(faces).to(pts.device)
    c = [v[faces[:, k]] for k in range(3)]
    return [[c[k][:, d][None, :] for d in range(3)] for k in range(3)], [p[:, d][:, None] for d in range(3)]


def _chunks(n_pts, n_faces, budget=1 << 23):
    step = max(1, budget // max(n_faces, 1))
    return [(s, min(s + step, n_pts)) for s in range(0, n_pts, step)]


def winding_number(verts, faces, pts, budget=1 << 23):
    """Generalised winding number of the mesh about every point, float64 [P]: the sum over the faces of the signed
    solid angle 2 atan2(det(a,b,c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) over 4 pi (Van Oosterom-Strackee),
    a, b, c the corners seen from the point.  Runs on numpy arrays and, unchanged, on torch tensors: then in
    torch.float64 on the device of `pts`.  Points are taken in chunks of budget / F, so that a temporary holds at most
    `budget` elements."""
    tor = _is_torch(pts)
    if tor:
        import torch
        sqrt, atan2, cat = torch.sqrt, torch.atan2, torch.cat
    else:
        sqrt, atan2, cat = np.sqrt, np.arctan2, np.concatenate
    out = []
    for s, e in _chunks(pts.shape[0], faces.shape[0], budget):
        (A, B, C), P = _planes(verts, faces, pts[s:e])
        ax, ay, az = A[0] - P[0], A[1] - P[1], A[2] - P[2]
        bx, by, bz = B[0] - P[0], B[1] - P[1], B[2] - P[2]
        cx, cy, cz = C[0] - P[0], C[1] - P[1], C[2] - P[2]
        la, lb, lc = sqrt(ax * ax + ay * ay + az * az), sqrt(bx * bx + by * by + bz * bz), sqrt(cx * cx + cy * cy + cz * cz)
        det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
        den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb
        out.append((2.0 * atan2(det, den)).sum(1) / (4.0 * np.pi))
    if not out:
        return _f64(np.zeros(0), pts)
    return cat(out)


def winding_inside(w):
    """inside <=> round(|w|) is odd (bool, same kind as w)"""
    if _is_torch(w):
        import torch
        return (torch.round(torch.abs(w)).to(torch.int64) % 2) == 1
    return (np.round(np.abs(w)).astype(np.int64) % 2) == 1


def set_aside(verts, faces, pts, orientation_test=True, budget=1 << 23):
    """bool [P], computed in float64: the only points where ray parity is ill-posed, so that a mismatch with the
    winding number is forgiven.  A point is set aside when its +x ray, looked at from t > -1e-3 on,
      * crosses a face within 1e-4 (barycentric units) of one of its edges, or with |t| < 1e-4; or
      * crosses a face whose doubled projected area satisfies |a| < 2e-7 (the contract never counts |a| < 1e-7).
    `Crosses` carries the same 1e-4 slack outwards.  The barycentric conditions are kept free of the division by a
    (u = U / a, v = W / a are compared as U, W against multiples of |a|), so an edge-on face needs no special case;
    how far such a face lies along the ray is judged by its x range, as its t is not defined.
    orientation_test=False switches the second rule off (used to show that the tests need it)."""
    tor = _is_torch(pts)
    if tor:
        import torch
        absf, where, cat = torch.abs, torch.where, torch.cat
        maxf, minf = torch.maximum, torch.minimum
    else:
        absf, where, cat = np.abs, np.where, np.concatenate
        maxf, minf = np.maximum, np.minimum
    out = []
    for s, e in _chunks(pts.shape[0], faces.shape[0], budget):
        (A, B, C), P = _planes(verts, faces, pts[s:e])
        e1x, e1y, e1z = B[0] - A[0], B[1] - A[1], B[2] - A[2]
        e2x, e2y, e2z = C[0] - A[0], C[1] - A[1], C[2] - A[2]
        a = e1z * e2y - e1y * e2z                                  # [1,F]
        sg = (a >= 0) * 2.0 - 1.0
        aa = absf(a)
        sx, sy, sz = P[0] - A[0], P[1] - A[1], P[2] - A[2]
        U = (sz * e2y - sy * e2z) * sg                             # u |a|
        qx = sy * e1z - sz * e1y
        W = qx * sg                                                # v |a|
        R = aa - U - W                                             # (1 - u - v) |a|
        slack = EDGE_TOL * aa + 1e-12
        touch = (U >= -slack) & (W >= -slack) & (R >= -slack)
        qy, qz = sz * e1x - sx * e1z, sx * e1y - sy * e1x
        tn = (e2x * qx + e2y * qy + e2z * qz) * sg                 # t |a|
        dead = aa < DEAD_A
        xhi = maxf(maxf(A[0], B[0]), C[0])
        ahead = where(dead, xhi - P[0] > T_BACK, tn > T_BACK * aa)
        near = (minf(minf(U, W), R) < slack) | (absf(tn) < T_TOL * aa)
        bad = touch & ahead & ((near & ~dead) | (dead if orientation_test else dead & False))
        out.append(bad.any(1))
    if not out:
        return _f64(np.zeros(0), pts) > 0
    return cat(out)
