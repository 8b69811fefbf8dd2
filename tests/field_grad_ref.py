"""Restatements of the field gradients on the tets (tet_field_grad.hip), written from the contract in
include/deftet_hip.h, and the inputs their tests share.

(a) numpy, fp32 or fp64 by `dtype`: gradient (g [B,T,C,3], vol [B,T]) in the adjugate form, energies [B,C,2], and in fp32 only,
    in exactly the library's order, tet_to_vertex (out, weight sums) and its backward.
(b) torch fp64 with autograd over the same formulas: chain64 (g, vol) and energies64.
A tet is live iff det > 0 IN FP32 (live_mask): every restatement, the fp64 ones included, takes that one mask, so a tet on the
edge of flat is the same tet to all of them.
"""
import functools

import numpy as np
import torch

from deftet_amd import grids

F32, F64 = np.float32, np.float64


def tets_of(tets, B):
    """int64 [B,T,4] view of a shared [T,4] or per-shape [B,T,4] list"""
    t = np.asarray(tets, np.int64)
    return np.broadcast_to(t[None], (B,) + t.shape) if t.ndim == 2 else t


def _adjugate(pos, tt, dtype):
    """(n [B,T,3,3], det [B,T]): n0 = e1 x e2, n1 = e2 x e0, n2 = e0 x e1, det = e0 . n0 with e_k = x_{k+1} - x_0"""
    pos = np.asarray(pos, dtype)
    B = pos.shape[0]
    x = pos[np.arange(B)[:, None, None], tt]                              # [B,T,4,3]
    e = x[:, :, 1:] - x[:, :, :1]
    n = np.stack([np.cross(e[:, :, 1], e[:, :, 2]), np.cross(e[:, :, 2], e[:, :, 0]), np.cross(e[:, :, 0], e[:, :, 1])], 2)
    det = (e[:, :, 0] * n[:, :, 0]).sum(-1, dtype=dtype)
    assert n.dtype == dtype and det.dtype == dtype
    return n, det


def live_mask(pos, tets):
    """bool [B,T]: det > 0 in fp32 (NaN, flat and inverted tets are dead)"""
    pos = np.asarray(pos, F32)
    with np.errstate(invalid="ignore"):
        return _adjugate(pos, tets_of(tets, pos.shape[0]), F32)[1] > 0


def gradient(field, pos, tets, dtype=F32):
    """(g [B,T,C,3], vol [B,T]) in `dtype`; 0 and volume 0 on a dead tet"""
    field = np.asarray(field, dtype)
    B = field.shape[0]
    tt, live = tets_of(tets, B), live_mask(pos, tets)
    with np.errstate(invalid="ignore", divide="ignore"):
        n, det = _adjugate(pos, tt, dtype)
        f = field[np.arange(B)[:, None, None], tt]                        # [B,T,4,C]
        df = f[:, :, 1:] - f[:, :, :1]                                    # [B,T,3,C]
        g = ((n[:, :, 0, None, :] * df[:, :, 0, :, None] + n[:, :, 1, None, :] * df[:, :, 1, :, None])
             + n[:, :, 2, None, :] * df[:, :, 2, :, None]) / det[:, :, None, None]
        vol = det / dtype(6)
    g = np.where(live[:, :, None, None], g, dtype(0))
    vol = np.where(live, vol, dtype(0))
    assert g.dtype == dtype and vol.dtype == dtype
    return g, vol


def energies(field, pos, tets, target=1.0, dtype=F32):
    """[B,C,2] in `dtype`: (sum w |g|^2 / W, sum w (|g| - target)^2 / W) over the live tets, the sums in fp64; 0 when W = 0"""
    g, vol = gradient(field, pos, tets, dtype)
    s2 = (g * g).sum(-1, dtype=dtype)                                     # [B,T,C]
    d = np.sqrt(s2) - dtype(target)
    w = vol.astype(F64)[:, :, None]
    W = w.sum(1)                                                          # [B,1]
    S = np.stack([(w * s2.astype(F64)).sum(1), (w * (d * d).astype(F64)).sum(1)], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(W[:, :, None] > 0, S / W[:, :, None], 0.0)
    return out.astype(dtype)


def tet_to_vertex(values, tets, V, weights=None, fill=0.0):
    """(out f32 [B,V,C], weight sums f32 [B,V]) in the library's order: per vertex one fp32 accumulator each for
    sum fl(w_t values[t]) and sum w_t over its incidences in ascending 4 t + corner, then one division; `fill` where the weight sum
    is not > 0"""
    values = np.asarray(values, F32)
    B, T, C = values.shape
    tt = tets_of(tets, B)
    w = np.ones((B, T), F32) if weights is None else np.asarray(weights, F32)
    num, den = np.zeros((B, V, C), F32), np.zeros((B, V), F32)
    for b in range(B):
        for s, v in enumerate(tt[b].reshape(-1)):                         # ascending 4 t + corner
            t = s >> 2
            num[b, v] = num[b, v] + w[b, t] * values[b, t]
            den[b, v] = den[b, v] + w[b, t]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(den[:, :, None] > 0, num / den[:, :, None], F32(fill))
    assert out.dtype == F32 and den.dtype == F32
    return out, den


def tet_to_vertex_bwd(gout, wsum, tets, weights=None):
    """f32 [B,T,C] = w_t * (sum over the corners 0..3 of gout[v_k] / wsum[v_k], one accumulator from 0, a corner whose weight sum
    is not > 0 left out)"""
    gout, wsum = np.asarray(gout, F32), np.asarray(wsum, F32)
    B, V, C = gout.shape
    tt = tets_of(tets, B)
    T = tt.shape[1]
    w = np.ones((B, T), F32) if weights is None else np.asarray(weights, F32)
    bi = np.arange(B)[:, None]
    acc = np.zeros((B, T, C), F32)
    for k in range(4):
        W = wsum[bi, tt[:, :, k]][:, :, None]                             # [B,T,1]
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = np.where(W > 0, acc + gout[bi, tt[:, :, k]] / W, acc)
    out = w[:, :, None] * acc
    assert out.dtype == F32
    return out


# ---------------------------------------------------------------------------- (b) torch fp64, autograd
def chain64(field, pos, tets, live):
    """(g fp64 [B,T,C,3], vol fp64 [B,T]) from torch fp64 field [B,V,C] and pos [B,V,3] (requires_grad kept) with the live mask
    handed in: E^-1 df by the adjugate, 0 and volume 0 on a dead tet"""
    B = pos.shape[0]
    tt = torch.from_numpy(np.array(tets_of(tets, B)))
    lv = torch.from_numpy(np.asarray(live))
    bi = torch.arange(B)[:, None, None]
    x, f = pos[bi, tt], field[bi, tt]                                     # [B,T,4,3], [B,T,4,C]
    e = x[:, :, 1:] - x[:, :, :1]
    cr = lambda a, b: torch.linalg.cross(a, b, dim=-1)
    n = torch.stack([cr(e[:, :, 1], e[:, :, 2]), cr(e[:, :, 2], e[:, :, 0]), cr(e[:, :, 0], e[:, :, 1])], 2)   # [B,T,3,3]
    det = (e[:, :, 0] * n[:, :, 0]).sum(-1)
    det = torch.where(lv, det, torch.ones_like(det))
    df = f[:, :, 1:] - f[:, :, :1]                                        # [B,T,3,C]
    g = torch.einsum("btka,btkc->btca", n, df) / det[:, :, None, None]
    zero = torch.zeros((), dtype=g.dtype)
    return torch.where(lv[:, :, None, None], g, zero), torch.where(lv, det / 6, zero)


def energies64(field, pos, tets, live, target=1.0):
    """fp64 [B,C,2] with autograd; where |g| = 0 the Eikonal term's derivative is 0 (the norm is taken of the rows that are not
    zero only)"""
    g, vol = chain64(field, pos, tets, live)
    s2 = (g * g).sum(-1)
    nz = s2 > 0
    s = torch.where(nz, torch.sqrt(torch.where(nz, s2, torch.ones_like(s2))), torch.zeros_like(s2))
    w = vol[:, :, None]
    W = w.sum(1)
    S = torch.stack([(w * s2).sum(1), (w * (s - target) ** 2).sum(1)], -1)
    safe = torch.where(W > 0, W, torch.ones_like(W))[:, :, None]
    return torch.where(W[:, :, None] > 0, S / safe, torch.zeros_like(S))


# ---------------------------------------------------------------------------- the inputs of the CPU and GPU tests
@functools.lru_cache(maxsize=None)
def mesh(R, B, per_shape=False):
    """(pos f32 [B,V,3], tets int64 [T,4] or [B,T,4]) of the jittered Kuhn grid, as tests/tet_field_ref.mesh builds it"""
    verts, tets = grids.kuhn_grid(R)
    pos = grids.jittered_positions(verts, R, B, 0.1)
    tets = tets.astype(np.int64)
    if per_shape:
        g = np.random.default_rng(77)
        even = np.array([[0, 1, 2, 3], [1, 2, 0, 3], [2, 0, 1, 3], [0, 2, 3, 1], [1, 0, 3, 2], [3, 0, 2, 1]])    # orientation kept
        tets = np.stack([np.take_along_axis(tets, even[g.integers(0, len(even), len(tets))], 1) for _ in range(B)])
    return pos, tets


def normal_field(shape):
    return np.random.default_rng(7).standard_normal(shape).astype(F32)


@functools.lru_cache(maxsize=None)
def wedge_ring(n=130):
    """(pos f32 [1,n+2,3], tets int64 [n,4]): n wedge tets (hub, apex, p_i, p_{i+1}) about the z axis, positively oriented; hub
    (vertex 0) and apex (vertex 1) have n incidences each"""
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(3 * a)], 1)
    pos = np.concatenate([[[0.0, 0.0, -0.3], [0.0, 0.0, 0.9]], ring]).astype(F32)[None]
    i = np.arange(n)
    tets = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), 2 + i, 2 + (i + 1) % n], 1)
    assert live_mask(pos, tets).all()
    return pos, tets


@functools.lru_cache(maxsize=None)
def dead_tet_mesh():
    """(pos f32 [1,V+5,3], tets int64 [T+2,4], ids of the two dead tets, the vertex only they touch): the R = 4 grid with a flat
    tet (four coplanar points, three of them new vertices) and an inverted one (a live tet with two vertices swapped) placed
    among the live ones"""
    pos, tets = mesh(4, 1)
    V = pos.shape[1]
    extra = np.array([[0.7, 0.7, 0.7], [0.9, 0.7, 0.7], [0.7, 0.9, 0.7], [0.9, 0.9, 0.7], [2.0, 2.0, 2.0]], F32)     # z = 0.7: a plane
    pos = np.concatenate([pos, extra[None]], 1)
    flat = np.array([V, V + 1, V + 2, V + 3])
    inverted = tets[5][[1, 0, 2, 3]]
    tets = np.concatenate([tets[:10], flat[None], tets[10:20], inverted[None], tets[20:]])
    live = live_mask(pos, tets)[0]
    assert not live[10] and not live[21] and live.sum() == len(tets) - 2
    return pos, tets, (10, 21), V + 3
