"""Restatements of tet-centroid feature sampling (include/deftet_hip.h), written from its contract:
(a) the whole operator in fp64 with torch autograd, on the sampler of tests/pointvoxel_ref.py;
(b) the two steps the operator adds to that sampler, in fp32 numpy in exactly the stated order: the centroid, and the reduction
    of the centroid gradient onto the vertices (incidences in CSR order, slots ascending, one accumulator, then * 0.25).
Also the inputs the tests share: random tet lists, the lattice vertices on which the position gradient is continuous, and the
literal decode_occ composition of the reference (pc_model.py:276-306)."""
import collections

import numpy as np
import torch

from tests import pointvoxel_ref as pv_ref

f32 = np.float32


def _np(a, dtype=None):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a) if dtype is None else np.asarray(a, dtype)


def _chosen(T, select=None, first=0, count=None):
    if select is not None:
        return _np(select, np.int64)
    return np.arange(first, T if count is None else first + count, dtype=np.int64)


# ---------------------------------------------------------------------------- (a) fp64, autograd
def occ_feature(vols, pos, idx, select=None, first=0, count=None, append_pos=True, dtype=torch.float64):
    """vols [B,C_k,R,R,R], pos [B,V,3], idx int [T,4] or [B,T,4] -> [B, sum C_k (+3), K]; differentiable in pos and vols"""
    idx = torch.as_tensor(_np(idx, np.int64), device=pos.device)
    sel = torch.as_tensor(_chosen(idx.shape[-2], select, first, count), device=pos.device)
    pos = pos.to(dtype)
    tets = pos[:, idx] if idx.dim() == 2 else torch.stack([pos[b, idx[b]] for b in range(pos.shape[0])])      # [B,T,4,3]
    return pv_ref.voxel_sample(vols, tets.mean(2)[:, sel], append_pos=append_pos, dtype=dtype)


def centroids64(pos, idx, select=None, first=0, count=None):
    pos, idx = _np(pos, np.float64), _np(idx, np.int64)
    sel = _chosen(idx.shape[-2], select, first, count)
    tets = pos[:, idx] if idx.ndim == 2 else np.stack([pos[b, idx[b]] for b in range(pos.shape[0])])
    return tets.mean(2)[:, sel]


# ---------------------------------------------------------------------------- (b) fp32, stated order
def centroids(pos, idx, select=None, first=0, count=None):
    """f32 [B,K,3]: (((a + b) + c) + d) * 0.25, every step rounded to fp32, corners in list order"""
    pos, idx = _np(pos, f32), _np(idx, np.int64)
    sel = _chosen(idx.shape[-2], select, first, count)
    t = idx[sel] if idx.ndim == 2 else idx[:, sel]                   # [K,4] / [B,K,4]
    corner = [pos[:, t[..., k]] if idx.ndim == 2 else np.stack([pos[b, t[b, :, k]] for b in range(pos.shape[0])]) for k in range(4)]
    s = (corner[0] + corner[1]).astype(f32)
    s = (s + corner[2]).astype(f32)
    s = (s + corner[3]).astype(f32)
    return (s * f32(0.25)).astype(f32)


def vertex_reduction(gcent, idx, n_vertex, select=None, first=0, base=None):
    """f32 [B,V,3] = 0.25 * S(v), S = one fp32 accumulator from 0 over the (tet, corner) incidences of v in ascending 4 t + corner
    and, per incidence, over the slots that chose tet t in ascending slot (a slot outside [0,T) counts nowhere).  select None: slot
    j is tet first + j.  base: the tensor the result is added to (`accumulate`)."""
    gcent, idx = _np(gcent, f32), _np(idx, np.int64)
    idx = idx[None] if idx.ndim == 2 else idx
    B, K = gcent.shape[:2]
    Bi, T = idx.shape[:2]
    if select is None:
        def slots_of(t):
            return [t - first] if 0 <= t - first < K else []
    else:
        table = collections.defaultdict(list)
        for j, t in enumerate(_np(select, np.int64)):
            if 0 <= t < T:
                table[int(t)].append(j)

        def slots_of(t):
            return table.get(t, [])
    out = np.zeros((B, n_vertex, 3), f32)
    for bi in range(Bi):
        shapes = list(range(B)) if Bi == 1 else [bi]
        incid = [[] for _ in range(n_vertex)]
        for s, v in enumerate(idx[bi].reshape(-1)):                  # ascending 4 t + corner
            if 0 <= v < n_vertex:
                incid[v].append(s)
        for v in range(n_vertex):
            acc = np.zeros((len(shapes), 3), f32)
            for s in incid[v]:
                for j in slots_of(s >> 2):
                    acc = (acc + gcent[shapes, j]).astype(f32)
            out[shapes, v] = (f32(0.25) * acc).astype(f32)
    return out if base is None else (_np(base, f32) + out).astype(f32)


# ---------------------------------------------------------------------------- the reference's own composition
def decode_occ_composition(pos, tet_bxfx4, c_list, center_idx=None):
    """pc_model.py:276-306 restated (pos_encoder None): torch.gather, mean, gather of center_idx, sample_f, cat"""
    n_batch = pos.shape[0]
    gather_input = pos.unsqueeze(2).expand(n_batch, pos.shape[1], 4, 3)
    gather_index = tet_bxfx4.unsqueeze(-1).expand(n_batch, tet_bxfx4.shape[1], 4, 3).long()
    tet_bxfx4x3 = torch.gather(input=gather_input, dim=1, index=gather_index)
    center_pos = torch.mean(tet_bxfx4x3, dim=2)
    if center_idx is not None:
        gather_index = center_idx.long().unsqueeze(0).unsqueeze(-1).expand(n_batch, center_idx.shape[0], 3)
        center_pos = torch.gather(input=center_pos, dim=1, index=gather_index)
    occ_feature = pv_ref.sample_f_composition(center_pos, c_list)
    return torch.cat([occ_feature, center_pos.permute(0, 2, 1)], dim=1)


# ---------------------------------------------------------------------------- shared inputs
def random_tets(T, V, seed, B=None):
    """int64 [T,4] (or [B,T,4]) of four distinct vertices each"""
    g = np.random.default_rng(seed)
    n = T if B is None else B * T
    tets = np.stack([g.choice(V, 4, replace=False) for _ in range(n)]).astype(np.int64)
    return tets if B is None else tets.reshape(B, T, 4)


def fan_tets(T, V, seed):
    """vertex 0 in every tet, the other three distinct among 1 .. V-1"""
    g = np.random.default_rng(seed)
    rest = np.stack([g.choice(V - 1, 3, replace=False) + 1 for _ in range(T)])
    return np.concatenate([np.zeros((T, 1), np.int64), rest], 1).astype(np.int64)


def uniform_vertices(B, V, seed):
    """1.05 (U - 0.5): border and outside positions among them"""
    return 1.05 * (torch.rand(B, V, 3, generator=torch.Generator().manual_seed(seed)) - 0.5)


def lattice_vertices(B, V, seed):
    """(k + f) / 32 - 0.5, integer k in [0,27], f in U[0.05, 0.20]: a centroid's voxel coordinate at R = 32, 16, 8 is a multiple of
    1/4, 1/8, 1/16 plus a fraction in [0.0125, 0.2] — never on an integer, strictly inside (0, R - 1)"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 28, (B, V, 3), generator=g).double()
    f = 0.05 + 0.15 * torch.rand(B, V, 3, generator=g, dtype=torch.float64)
    return ((k + f) / 32 - 0.5).float()


def lattice_margin(cent64, R):
    """the distance in fp64 of the voxel coordinates (cent + 0.5) R from the nearest integer, and whether all lie inside (0, R-1)"""
    u = (np.asarray(cent64, np.float64) + 0.5) * R
    return float(np.abs(u - np.round(u)).min()), bool((u > 0).all() and (u < R - 1).all())
