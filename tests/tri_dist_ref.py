"""fp64 reference of the point-to-triangle backward (operator A9), numpy only.

closest_on_triangle   Ericson's region tests: barycentric weights of the closest point and its feature class
envelope_gradient     the gradient of sum_i g_i * dist^2(p_i, triangle f_i) onto the triangle corners

The closest point cl = sum_c w_c * corner_c minimises |p - cl|^2 over the triangle, so its parameters are stationary (or
pinned at a bound) and the envelope theorem gives d dist^2 / d corner_c = 2 * w_c * (cl - p): nothing of the operator's
own arithmetic (plane projection, xy barycentrics, line parameters) enters.  The operator equals this for the face and the
vertex class; for the edge class it follows the reference, which writes onto the first endpoint only.
"""
import numpy as np

FACE, EDGE, VERTEX = 0, 1, 2


def _dot(x, y):
    return (x * y).sum(-1)


def closest_on_triangle(p, a, b, c):
    """p, a, b, c [N,3] fp64 -> (w [N,3] barycentric weights of the closest point on triangle abc, cls [N] in {0,1,2})."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac = b - a, c - a
    d1, d2 = _dot(ab, p - a), _dot(ac, p - a)
    d3, d4 = _dot(ab, p - b), _dot(ac, p - b)
    d5, d6 = _dot(ab, p - c), _dot(ac, p - c)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    zero = np.zeros_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = va + vb + vc
        w = np.stack([va / s, vb / s, vc / s], -1)                  # the plane projection lies inside
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    cls = np.full(d1.shape, FACE, np.int64)

    def region(mask, weights, kind):
        nonlocal w, cls
        w = np.where(mask[..., None], np.stack(weights, -1), w)
        cls = np.where(mask, kind, cls)

    region((vb <= 0) & (d2 >= 0) & (d6 <= 0), [1 - t_ac, zero, t_ac], EDGE)
    region((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), [zero, 1 - t_bc, t_bc], EDGE)
    region((vc <= 0) & (d1 >= 0) & (d3 <= 0), [1 - t_ab, t_ab, zero], EDGE)
    region((d6 >= 0) & (d5 <= d6), [zero, zero, zero + 1], VERTEX)
    region((d3 >= 0) & (d4 <= d3), [zero, zero + 1, zero], VERTEX)
    region((d1 <= 0) & (d2 <= 0), [zero + 1, zero, zero], VERTEX)
    return w, cls


def envelope_gradient(p, tri, f, g):
    """p [P,3], tri [F,3,3], f [P] saved face per point (outside [0,F): no contribution), g [P] incoming gradient
    -> [F,3,3] fp64: sum over the points of 2 * g_i * w_i[c] * (cl_i - p_i) onto corner c of face f_i."""
    p, tri, g = np.asarray(p, np.float64), np.asarray(tri, np.float64), np.asarray(g, np.float64).reshape(-1)
    f = np.asarray(f).reshape(-1).astype(np.int64)
    out = np.zeros(tri.shape, np.float64)
    ok = (f >= 0) & (f < tri.shape[0])
    p, f, g = p[ok], f[ok], g[ok]
    t = tri[f]
    w, _ = closest_on_triangle(p, t[:, 0], t[:, 1], t[:, 2])
    cl = (w[:, :, None] * t).sum(1)
    np.add.at(out, f, 2.0 * g[:, None, None] * w[:, :, None] * (cl - p)[:, None, :])
    return out
