"""Restatements of per-vertex field sampling at query points (tet_field_sample.hip), and the inputs its tests share.

(a) numpy fp32, in exactly the library's orders, from the library's OWN cond and bary (so the GPU's location decides the tet and
    no query is excluded for lying near a face):
      values(field, tets, cond, bary, fill)   ((w0 f0 + w1 f1) + w2 f2) + w3 f3 per channel, every product and sum rounded
      grad_w(field, tets, cond, gout)         the sum over c ascending of gout[q,c] * f(v_k,c), one accumulator from 0
      grad_field(gout, cond, bary, tets, V)   per vertex one accumulator from 0 over its incidences (4 t + corner ascending), per
                                              incidence over the queries with cond == t in ascending q, of bary[q,corner] * gout[q,c]
(b) torch fp64 from pos, pts and field: the barycentric weights of utils/tet_utils.py:28-45 in the tet cond names,
    times the gathered field rows, with autograd for all three gradients.
"""
import functools

import numpy as np
import torch

from deftet_amd import grids

F32 = np.float32


def tets_of(tets, B):
    """int64 [B,T,4] view of a shared [T,4] or per-shape [B,T,4] list"""
    t = np.asarray(tets, np.int64)
    return np.broadcast_to(t[None], (B,) + t.shape) if t.ndim == 2 else t


def located(cond):
    """int64 [B,Q]: the tet of every query, -1 for a miss"""
    c = np.asarray(cond, F32).reshape(cond.shape[0], -1)
    return np.where(c >= 0, c, -1).astype(np.int64)


# ---------------------------------------------------------------------------- (a) fp32, the library's orders
def values(field, tets, cond, bary, fill=0.0):
    field, bary = np.asarray(field, F32), np.asarray(bary, F32)
    B, V, C = field.shape
    tt, t = tets_of(tets, B), located(cond)
    out = np.full((B, t.shape[1], C), fill, F32)
    for b in range(B):
        hit = np.nonzero(t[b] >= 0)[0]
        vi = tt[b][t[b, hit]]                                          # [H,4]
        ok = ((vi >= 0) & (vi < V)).all(1)
        f = field[b][np.clip(vi, 0, V - 1)]                            # [H,4,C]
        w = bary[b, hit][:, :, None]                                   # [H,4,1]
        r = ((w[:, 0] * f[:, 0] + w[:, 1] * f[:, 1]) + w[:, 2] * f[:, 2]) + w[:, 3] * f[:, 3]
        assert r.dtype == F32
        r[~ok] = np.nan
        out[b, hit] = r
    return out


def grad_w(field, tets, cond, gout):
    field, gout = np.asarray(field, F32), np.asarray(gout, F32)
    B, V, C = field.shape
    tt, t = tets_of(tets, B), located(cond)
    gw = np.zeros((B, t.shape[1], 4), F32)
    for b in range(B):
        hit = np.nonzero(t[b] >= 0)[0]
        vi = tt[b][t[b, hit]]
        ok = ((vi >= 0) & (vi < V)).all(1)
        f = field[b][np.clip(vi, 0, V - 1)]                            # [H,4,C]
        acc = np.zeros((len(hit), 4), F32)
        for c in range(C):
            acc = acc + gout[b, hit, c][:, None] * f[:, :, c]
        assert acc.dtype == F32
        acc[~ok] = 0
        gw[b, hit] = acc
    return gw


def grad_field(gout, cond, bary, tets, V, base=None):
    gout, bary = np.asarray(gout, F32), np.asarray(bary, F32)
    B, Q, C = gout.shape
    tt, t = tets_of(tets, B), located(cond)
    T = tt.shape[1]
    out = np.zeros((B, V, C), F32)
    for b in range(B):
        lists = [[] for _ in range(T)]
        for q in range(Q):                                             # ascending q
            if 0 <= t[b, q] < T:
                lists[t[b, q]].append(q)
        inc = [[] for _ in range(V)]
        for s, v in enumerate(tt[b].reshape(-1)):                      # ascending 4 t + corner
            if 0 <= v < V:
                inc[v].append(s)
        for v in range(V):
            acc = np.zeros(C, F32)
            for s in inc[v]:
                for q in lists[s >> 2]:
                    acc = acc + bary[b, q, s & 3] * gout[b, q]
            out[b, v] = acc
    assert out.dtype == F32
    return out if base is None else np.asarray(base, F32) + out


def grad_field_dense(gout, cond, bary, tets, V):
    """the same sum in no particular order, in fp64: one term per (query, corner), added to the vertex it names"""
    gout, bary = np.asarray(gout, np.float64), np.asarray(bary, np.float64)
    B, Q, C = gout.shape
    tt, t = tets_of(tets, B), located(cond)
    out = np.zeros((B, V, C))
    for b in range(B):
        for q in range(Q):
            if t[b, q] >= 0:
                for k in range(4):
                    out[b, tt[b, t[b, q], k]] += bary[b, q, k] * gout[b, q]
    return out


# ---------------------------------------------------------------------------- (b) fp64, the whole chain
def bary64(a, b, c, d, p):
    """utils/tet_utils.py:28-45 on torch tensors: the four signed sub-volumes over the tet's"""
    def triple(x, y, z):
        return torch.sum(x * torch.linalg.cross(y, z, dim=-1), dim=-1)
    vap, vbp = p - a, p - b
    vab, vac, vad = b - a, c - a, d - a
    vbc, vbd = c - b, d - b
    v6 = 1 / triple(vab, vac, vad)
    return torch.stack([triple(vbp, vbd, vbc) * v6, triple(vap, vac, vad) * v6, triple(vap, vad, vab) * v6, triple(vap, vab, vac) * v6], -1)


def chain64(field, pos, pts, tets, cond, fill=0.0):
    """fp64 [B,Q,C] from torch tensors field [B,V,C], pos [B,V,3], pts [B,Q,3] (requires_grad kept): weights of pts in the tet
    cond names, times the field rows of its vertices; `fill` on a miss"""
    B = pos.shape[0]
    tt = torch.from_numpy(np.array(tets_of(tets, B)))
    t = torch.from_numpy(located(cond.detach().cpu().numpy() if hasattr(cond, "detach") else cond))
    hit = t >= 0
    vi = torch.gather(tt, 1, t.clamp(min=0)[:, :, None].expand(-1, -1, 4))                  # [B,Q,4]
    bi = torch.arange(B)[:, None, None]
    corners, rows = pos[bi, vi], field[bi, vi]                                              # [B,Q,4,3], [B,Q,4,C]
    w = bary64(corners[:, :, 0], corners[:, :, 1], corners[:, :, 2], corners[:, :, 3], pts)
    val = (w[..., None] * rows).sum(2)
    return torch.where(hit[..., None], val, torch.full_like(val, fill))


# ---------------------------------------------------------------------------- the inputs of the CPU and GPU tests
@functools.lru_cache(maxsize=None)
def mesh(R, B, per_shape=False):
    """(pos f32 [B,V,3], tets int64 [T,4] or [B,T,4]) of the jittered Kuhn grid; per_shape: every shape its own renumbering of the
    corners inside each tet (the same tets, so the same hits; other vertex slots)"""
    verts, tets = grids.kuhn_grid(R)
    pos = grids.jittered_positions(verts, R, B, 0.1)
    tets = tets.astype(np.int64)
    if per_shape:
        g = np.random.default_rng(77)
        even = np.array([[0, 1, 2, 3], [1, 2, 0, 3], [2, 0, 1, 3], [0, 2, 3, 1], [1, 0, 3, 2], [3, 0, 2, 1]])    # orientation kept
        tets = np.stack([np.take_along_axis(tets, even[g.integers(0, len(even), len(tets))], 1) for _ in range(B)])
    return pos, tets


def field_of(B, V, C, seed=3):
    return np.random.default_rng(seed + 10 * C).standard_normal((B, V, C)).astype(F32)


def gout_of(B, Q, C, seed=4):
    return np.random.default_rng(seed + 10 * C + Q).standard_normal((B, Q, C)).astype(F32)


def cpu_location(pos, tets, pts):
    """(cond f32 [B,Q,1], bary f32 [B,Q,4]) by brute force: the lowest tet all four fp64 weights of which are >= 0, and the weights
    in that tet by the same formula in fp32.  It stands in for the library's location where there is no GPU; a query near a face
    may land in the neighbour the library did not choose."""
    B, Q = pts.shape[0], pts.shape[1]
    tt = tets_of(tets, B)
    cond, bary = np.full((B, Q, 1), -1, F32), np.zeros((B, Q, 4), F32)
    for b in range(B):
        c = torch.from_numpy(pos[b].astype(np.float64))[torch.from_numpy(np.array(tt[b]))]                  # [T,4,3]
        p = torch.from_numpy(pts[b].astype(np.float64))[:, None]                                                        # [Q,1,3]
        w = bary64(c[None, :, 0], c[None, :, 1], c[None, :, 2], c[None, :, 3], p).numpy()                               # [Q,T,4]
        inside = (w >= 0).all(-1)
        first = inside.argmax(1)
        hit = inside.any(1)
        cond[b, hit, 0] = first[hit]
        c32, p32 = c.float()[first[hit]], p.float()[np.nonzero(hit)[0], 0]
        bary[b, hit] = bary64(c32[:, 0], c32[:, 1], c32[:, 2], c32[:, 3], p32).numpy()
    return cond, bary
