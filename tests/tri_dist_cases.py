"""Inputs of the point-to-triangle backward tests (tests/test_tri_dist_ref_cpu.py, tests/test_tri_dist_backward_gpu.py).

pin_*        the fp64 pin: a rotated sphere surface without its nearly vertical faces (for those the operator's xy-only inside
             test is degenerate, see test_a9_semantic_pin_true_point_triangle_distance), points a little off its faces and
             beyond its corners, and an incoming gradient that is zero wherever the operator is not the true gradient
edge_case    wave and block edges: closest_f is constructed, the backward accepts any saved index
"""
import numpy as np
import torch

from tests import tri_dist_ref as R

PIN_SEED = 9
N_FACE_PTS, N_VERTEX_PTS = 1500, 600
CLEAR_WEIGHT = 1e-3
# what the pin must offer before it is worth asserting on
MIN_CLEAR_SHARE, MIN_CLEAR_FACE, MIN_CLEAR_VERTEX, MAX_PER_FACE = 0.8, 1000, 150, 22


def pin_surface_and_points(oracle):
    """tri f32 [F,3,3], pts f32 [2100,3], and the generator to go on with"""
    from tests.test_surface_ops_gpu import _sphere_surfaces
    v, faces = _sphere_surfaces(torch.device("cpu"), oracle, [0.33])
    tri = v[0][faces[0]].numpy().astype(np.float64)
    rng = np.random.default_rng(PIN_SEED)
    qm, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    tri = tri @ qm.T
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    tri = tri[np.abs(n[:, 2]) > 0.2 * np.linalg.norm(n, axis=1)]
    F = tri.shape[0]
    # a little off the faces, on both sides
    t = tri[rng.integers(0, F, N_FACE_PTS)]
    w = rng.dirichlet([2, 2, 2], N_FACE_PTS)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    on_face = (w[:, :, None] * t).sum(1) + 0.01 * rng.choice([-1.0, 1.0], (N_FACE_PTS, 1)) * nrm
    # beyond the corners: the surface is a sphere about the origin
    corner = tri[rng.integers(0, F, N_VERTEX_PTS), rng.integers(0, 3, N_VERTEX_PTS)]
    beyond = corner * rng.uniform(1.02, 1.08, (N_VERTEX_PTS, 1))
    pts = np.concatenate([on_face, beyond], 0)
    return tri.astype(np.float32), pts.astype(np.float32), rng


def pin_gradient(tri, pts, closest_f, rng):
    """The incoming gradient of the pin for the saved faces closest_f [P]: seeded normal values on the clear points (class
    face with every weight above CLEAR_WEIGHT, or class vertex, both judged in fp64 on the saved face), zero elsewhere, so
    that the other points contribute nothing and nothing has to be masked afterwards.  -> (dl_dd f32 [P], cls [P], clear [P])"""
    f = np.asarray(closest_f).reshape(-1).astype(np.int64)
    assert (f >= 0).all() and (f < tri.shape[0]).all()
    t = tri[f].astype(np.float64)
    w, cls = R.closest_on_triangle(pts.astype(np.float64), t[:, 0], t[:, 1], t[:, 2])
    clear = ((cls == R.FACE) & (w.min(1) > CLEAR_WEIGHT)) | (cls == R.VERTEX)
    g = np.where(clear, rng.standard_normal(f.shape[0]), 0.0).astype(np.float32)
    return g, cls, clear


def check_pin_conditions(tri, closest_f, cls, clear):
    f = np.asarray(closest_f).reshape(-1).astype(np.int64)
    per_face = np.bincount(f[clear], minlength=tri.shape[0])
    stats = {"faces": int(tri.shape[0]), "clear_share": float(clear.mean()), "clear_face": int((clear & (cls == R.FACE)).sum()),
             "clear_vertex": int((clear & (cls == R.VERTEX)).sum()), "edge": int((cls == R.EDGE).sum()), "max_per_face": int(per_face.max())}
    assert stats["clear_share"] >= MIN_CLEAR_SHARE, stats
    assert stats["clear_face"] >= MIN_CLEAR_FACE and stats["clear_vertex"] >= MIN_CLEAR_VERTEX, stats
    assert stats["max_per_face"] <= MAX_PER_FACE, stats
    return stats


def non_finite_gradient(tri, pts, cf, cls, clear, g):
    """The pin's incoming gradient with +inf, -inf and NaN on one point of each class each (on faces of their own), and +inf
    and -inf on two face-class points that share a face and a side of it, so that their terms cancel to NaN.
    -> (g, the indices of those points, the shared face, the faces of the three edge-class points)"""
    g = g.copy()
    bad, used = {}, set()

    def take(mask, values):                                          # the first points of the mask on faces not used yet
        for v in values:
            i = next(int(i) for i in np.nonzero(mask)[0] if int(cf[i]) not in used)
            used.add(int(cf[i]))
            bad[i] = v

    take(clear & (cls == R.FACE), [np.inf, -np.inf, np.nan])
    take(clear & (cls == R.VERTEX), [np.inf, -np.inf, np.nan])
    take(cls == R.EDGE, [np.inf, -np.inf, np.nan])
    edge_faces = [int(cf[i]) for i in bad if cls[i] == R.EDGE]
    t = tri[cf].astype(np.float64)
    above = (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) * (pts - t[:, 0])).sum(1) > 0
    cand = clear & (cls == R.FACE) & above & ~np.isin(cf, list(used))
    shared = next(int(f) for f in np.unique(cf[cand]) if (cf[cand] == f).sum() >= 2)
    i, j = np.nonzero(cand & (cf == shared))[0][:2]
    bad[int(i)], bad[int(j)] = np.inf, -np.inf
    idx = np.array(sorted(bad))
    g[idx] = [bad[k] for k in idx]
    return g, idx, shared, edge_faces


def maxnorm(got, want):
    """the max-norm reading of tests/tol.check_close"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- wave and block edges -------------------------------------------------------------------------------------------------

EDGE_P = [1, 63, 64, 65, 255, 256, 257, 64 * 256 + 77]
EDGE_PATTERNS = ["one_face", "distinct", "mixed"]


def _around(tri, rng):
    """One point per triangle of tri [N,3,3] (fp64), cycling through: over the face, beyond each edge, beyond each corner;
    alternately above and below the plane."""
    N = tri.shape[0]
    kind = np.arange(N) % 7
    inside = rng.dirichlet([2, 2, 2], N)
    w = inside.copy()
    for e in range(3):                                               # beyond the edge opposite corner e
        m = kind == 1 + e
        w[m, e] = -rng.uniform(0.2, 0.8, m.sum())
        rest = inside[m][:, [(e + 1) % 3, (e + 2) % 3]]
        rest = 0.2 + 0.6 * rest / rest.sum(1, keepdims=True)         # the foot stays well inside the edge
        rest /= rest.sum(1, keepdims=True)
        w[m, (e + 1) % 3] = rest[:, 0] * (1 - w[m, e])
        w[m, (e + 2) % 3] = rest[:, 1] * (1 - w[m, e])
    for c in range(3):                                               # beyond corner c, in the wedge opposite the face
        m = kind == 4 + c
        out = rng.uniform(0.1, 0.5, (m.sum(), 2))
        w[m, (c + 1) % 3], w[m, (c + 2) % 3] = -out[:, 0], -out[:, 1]
        w[m, c] = 1 + out.sum(1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    h = np.sqrt(np.linalg.norm(nrm, axis=1, keepdims=True))          # ~ the edge length
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    side = np.where((np.arange(N) // 7) % 2 == 0, 1.0, -1.0)[:, None]
    return (w[:, :, None] * tri).sum(1) + side * rng.uniform(0.05, 0.3, (N, 1)) * h * nrm


def edge_case(pattern, P, seed=0):
    """-> pts f32 [1,P,3], face f32 [1,F,3,3], closest_f f32 [1,P,1], dl_dd f32 [1,P,1]"""
    rng = np.random.default_rng([seed, P, EDGE_PATTERNS.index(pattern)])
    if pattern == "one_face":
        face = np.array([[[0.11, 0.07, 0.02], [0.52, 0.13, 0.21], [0.23, 0.61, 0.38]]])
        cf = np.zeros(P, np.int64)
        pts = _around(face[cf], rng)
    elif pattern == "distinct":
        n = int(np.ceil(P ** (1 / 3) - 1e-9))
        cell = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)[:P]
        centre = (cell + 0.5 + (rng.random((P, 3)) - 0.5) * 0.2) / n      # one triangle per lattice cell, well apart
        face = centre[:, None, :] + (rng.random((P, 3, 3)) - 0.5) * (0.3 / n)
        cf = rng.permutation(P)
        pts = _around(face[cf], rng)
    else:
        F = max(1, P // 7)
        face = rng.random((F, 1, 3)) * 0.9 + 0.05 + (rng.random((F, 3, 3)) - 0.5) * 0.1
        cf = rng.integers(0, F, P)
        pts = _around(face[cf], rng)
        skip = rng.random(P)
        cf = np.where(skip < 0.1, -1, np.where(skip < 0.2, F, cf))   # both skips: no face saved, index past the end
    g = rng.standard_normal(P)
    return (pts[None].astype(np.float32), face[None].astype(np.float32), cf.astype(np.float32).reshape(1, P, 1),
            g.astype(np.float32).reshape(1, P, 1))


def per_point_terms(oracle, pts, face, closest_f, dl_dd):
    """[P,3,3] f32: point i's own contribution to its face, from the oracle itself: every point gets a private copy of its
    face, saved as face i, and row i of the oracle's output is then that point's term (zero rows for skipped points)."""
    P, F = pts.shape[1], face.shape[1]
    cf = closest_f.reshape(-1).astype(np.int64)
    ok = (cf >= 0) & (cf < F)
    own = face[0][np.where(ok, cf, 0)][None]                         # [1,P,3,3]
    idx = np.where(ok, np.arange(P), -1).astype(np.float32).reshape(1, P, 1)
    return oracle.tri_dist_bwd(pts, own, idx, dl_dd)[0]


def order_bound(terms, closest_f, F):
    """(want fp64 [F,3,3], bound [F,3,3]): the fp64 sum of the per-point terms per face and n_f * 2^-24 * sum |term|, the
    first-order worst case of any order of fp32 additions of the n_f contributions to a face."""
    cf = closest_f.reshape(-1).astype(np.int64)
    ok = (cf >= 0) & (cf < F)
    want, mag = np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
    np.add.at(want, cf[ok], terms[ok].astype(np.float64))
    np.add.at(mag, cf[ok], np.abs(terms[ok].astype(np.float64)))
    n_f = np.bincount(cf[ok], minlength=F).astype(np.float64)
    return want, n_f[:, None, None] * 2.0 ** -24 * mag
