"""Reference of the point-in-tet weights and backward for one shape, in numpy.

analytic      fp64: w per hit, G = sum_i g_i grad_p w_i (= dL/dp; G_terms: the same sum of absolute values, largest component),
              the per-hit contribution c = -w (x) G to the hit tet's 12 gradient entries, their per-tet sums, hit counts n_t and
              S_t = sum over the tet's hits of max|c|; grad_pred (the per-tet sum of grad_occ, every miss added to tet 0) summed
              with math.fsum, with the number of terms and sum |term|.
restatement   fp32: the arithmetic of the backward kernels (tet_grad_setup / tet_grad_add in csrc/point_in_tet.hip), operation by
              operation, with running fp32 sums in ascending query order.  The build contracts nothing (-ffp-contract=off), and
              numpy rounds every fp32 operation once, so this is what a lane computes.
bounds        the bounds the kernels are held to (tests/bary_cases.py: U, K, kappa).
"""
import math

import numpy as np

from tests.bary_cases import K, U


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _hits(cond):
    c = np.asarray(cond).reshape(-1)
    hit = c >= 0
    return hit, np.where(hit, c, 0).astype(np.int64)


def analytic(tet, pts, cond, grad_w, grad_occ=None):
    tet, pts, gw = np.asarray(tet, np.float64), np.asarray(pts, np.float64), np.asarray(grad_w, np.float64)
    T, Q = tet.shape[0], pts.shape[0]
    hit, t = _hits(cond)
    a, b, c, d = (tet[t][:, k] for k in range(4))
    n = np.stack([_cross(d - b, c - b), _cross(c - a, d - a), _cross(d - a, b - a), _cross(b - a, c - a)], 1)      # [Q,4,3] = det * grad_p w_i
    det = _dot(b - a, n[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.stack([_dot(pts - b, n[:, 0]), _dot(pts - a, n[:, 1]), _dot(pts - a, n[:, 2]), _dot(pts - a, n[:, 3])], 1) / det[:, None]
        G = (gw[:, :, None] * n).sum(1) / det[:, None]
        G_terms = (np.abs(gw)[:, :, None] * np.abs(n)).sum(1).max(1) / np.abs(det)
    w, G = np.where(hit[:, None], w, 0.0), np.where(hit[:, None], G, 0.0)
    contrib = -w[:, :, None] * G[:, None, :]
    out = {"hit": hit, "t": t, "w": w, "G": G, "c": contrib, "G_terms": np.where(hit, G_terms, 0.0)}
    out["grad_tet"], out["S"] = np.zeros((T, 4, 3)), np.zeros(T)
    np.add.at(out["grad_tet"], t[hit], contrib[hit])
    np.add.at(out["S"], t[hit], np.abs(contrib[hit]).max((1, 2)))
    out["n"] = np.bincount(t[hit], minlength=T)
    if grad_occ is not None:
        go = np.asarray(grad_occ, np.float64).reshape(-1)
        terms = [[] for _ in range(T)]
        for q in range(Q):
            terms[t[q]].append(go[q])                                # a miss has t == 0: paste_occ clamps it to tet 0
        out["grad_pred"] = np.array([math.fsum(x) for x in terms])
        out["pred_n"] = np.array([len(x) for x in terms])
        out["pred_abs"] = np.array([math.fsum(abs(v) for v in x) for x in terms])
    return out


def scatter_to_vertices(per_tet, idx, n_vertex):
    """[V,...] fp64: per_tet [T,4,...] (a gradient, or a bound) summed over the incidences of every vertex of idx [T,4]"""
    out = np.zeros((n_vertex,) + per_tet.shape[2:])
    np.add.at(out, np.asarray(idx).reshape(-1), per_tet.reshape((-1,) + per_tet.shape[2:]))
    return out


def restatement(tet, pts, cond, grad_w):
    """-> (w f32 [Q,4], G f32 [Q,3], grad_tet f32 [T,4,3]); zero rows for the misses and for tets without a hit"""
    f = np.float32
    tet, pts, gw = np.asarray(tet, f), np.asarray(pts, f), np.asarray(grad_w, f)
    T = tet.shape[0]
    hit, t = _hits(cond)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # tet_grad_setup
        A, B, C, D = (tet[:, k] for k in range(4))
        vab, vac, vad, vbc, vbd = B - A, C - A, D - A, C - B, D - B
        na, nb, nc, nd = _cross(vbd, vbc), _cross(vac, vad), _cross(vad, vab), _cross(vab, vac)
        v6 = f(1.0) / _dot(vab, nb)
        # tet_grad_add
        vap, vbp = pts - A[t], pts - B[t]
        w = np.stack([_dot(vbp, na[t]), _dot(vap, nb[t]), _dot(vap, nc[t]), _dot(vap, nd[t])], 1) * v6[t][:, None]
        G = (((gw[:, 0:1] * na[t] + gw[:, 1:2] * nb[t]) + gw[:, 2:3] * nc[t]) + gw[:, 3:4] * nd[t]) * v6[t][:, None]
        term = -w[:, :, None] * G[:, None, :]
        assert w.dtype == f and G.dtype == f and term.dtype == f
        # acc += term, in ascending query order within every tet
        acc = np.zeros((T, 4, 3), f)
        q = np.nonzero(hit)[0]
        q = q[np.argsort(t[q], kind="stable")]                       # by tet, ascending query inside a tet
        tq = t[q]
        rank = np.arange(q.shape[0]) - np.searchsorted(tq, tq, side="left")
        for r in range(int(rank.max()) + 1 if q.size else 0):
            sel = q[rank == r]
            acc[t[sel]] = acc[t[sel]] + term[sel]
    return np.where(hit[:, None], w, f(0)), np.where(hit[:, None], G, f(0)), acc


# ---- the bounds ------------------------------------------------------------------------------------------------------------

def bound_w(ref, kappa, k=K):
    """[Q]: k u kappa max(1, max|w64|) for the weights of a query"""
    return k * U * kappa[ref["t"]] * np.maximum(1.0, np.abs(ref["w"]).max(1))


def bound_G(ref, kappa, k=K, terms=False):
    """[Q]: k u kappa max|G64|; terms=True: k u kappa max_k sum_i |g_i| |grad_p w_i|_k instead, the scale of what is added up (on
    a well shaped tet kappa is of order 10, and where the four terms cancel the error no longer follows the size of their sum)"""
    return k * U * kappa[ref["t"]] * (ref["G_terms"] if terms else np.abs(ref["G"]).max(1))


def bound_tet(ref, kappa, k=K):
    """[T]: (k + n_t) u kappa_t S_t, n_t u S_t being the plain bound of a recursive sum of n_t terms"""
    return (k + ref["n"]) * U * kappa * ref["S"]


def bound_pred(ref):
    """[T]: (2 + log2 n + n / 64) u sum |term| for an entry that n terms are added into, 0 where n == 0"""
    n = ref["pred_n"].astype(np.float64)
    return np.where(n > 0, 2.0 + np.log2(np.maximum(n, 1.0)) + n / 64.0, 0.0) * U * ref["pred_abs"]
