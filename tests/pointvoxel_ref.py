"""Restatements of the point-voxel operators (include/deftet_hip.h), written from their contracts:
average voxelization in fp32 in the stated order, the trilinear sampler in fp64 / fp32 with torch autograd, and the legacy
devoxelization kernel's indices, weights and values in fp32.  What the GPU tests compare the HIP path with."""
import numpy as np
import torch

f32 = np.float32


# ---------------------------------------------------------------------------- average voxelization (fp32, stated order)
def avg_voxelize(feat, coords, R):
    """feat f32 [B,C,N], coords i32 [B,3,N] -> out f32 [B,C,R^3], ind i32 [B,N], cnt i32 [B,R^3]"""
    feat, coords = np.asarray(feat, f32), np.asarray(coords, np.int64)
    B, C, N = feat.shape
    ok = ((coords >= 0) & (coords < R)).all(axis=1)
    ind = np.where(ok, coords[:, 0] * R * R + coords[:, 1] * R + coords[:, 2], -1).astype(np.int32)
    cnt = np.zeros((B, R ** 3), np.int32)
    for b in range(B):
        np.add.at(cnt[b], ind[b][ok[b]], 1)
    out = np.zeros((B, C, R ** 3), f32)
    for b in range(B):
        for i in range(N):                                          # ascending i: every product rounded, then added
            s = ind[b, i]
            if s >= 0:
                out[b, :, s] = out[b, :, s] + feat[b, :, i] * (f32(1.0) / f32(cnt[b, s]))
    return out, ind, cnt


def avg_voxelize_bwd(gy, ind, cnt):
    gy = np.asarray(gy, f32)
    B, C, _ = gy.shape
    gx = np.zeros((B, C, ind.shape[1]), f32)
    for b in range(B):
        ok = ind[b] >= 0
        s = ind[b][ok]
        gx[b][:, ok] = gy[b][:, s] * (f32(1.0) / cnt[b][s].astype(f32))[None, :]
    return gx


# ---------------------------------------------------------------------------- the sampler (torch, any dtype, autograd)
def _corners(u, r):
    lo = torch.floor(u.detach())
    d = u - lo
    lo = lo.long()
    hi = torch.clamp(lo + 1, max=r - 1)
    idx, w = [], []
    for k in range(8):
        sel = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
        c = [hi[..., j] if sel[j] else lo[..., j] for j in range(3)]
        f = [d[..., j] if sel[j] else 1 - d[..., j] for j in range(3)]
        idx.append((c[0] * r + c[1]) * r + c[2])
        w.append(f[0] * f[1] * f[2])
    return idx, w


def voxel_sample(volumes, pos, append_pos=False, dtype=torch.float64, voxel_units=False):
    """volumes [B,C_k,R,R,R], pos [B,N,3] (or coords [B,3,N] with voxel_units) -> [B, sum C_k (+3), N], differentiable.
    The border rule is stated, not inherited from clamp: a coordinate with raw u <= 0 or >= r - 1 is held constant."""
    pos = pos.to(dtype)
    p = pos.permute(0, 2, 1) if voxel_units else pos
    outs = []
    for v in volumes:
        v = v.to(dtype)
        B, C, r = v.shape[0], v.shape[1], v.shape[-1]
        raw = p if voxel_units else (p + 0.5) * r
        inside = (raw > 0) & (raw < r - 1)
        u = torch.where(inside, raw, torch.nan_to_num(raw.detach(), nan=0.0).clamp(0, r - 1))
        idx, w = _corners(u, r)
        flat = v.reshape(B, C, r ** 3)
        acc = 0
        for k in range(8):
            acc = acc + w[k][:, None, :] * torch.gather(flat, 2, idx[k][:, None, :].expand(B, C, -1))
        outs.append(acc)
    if append_pos:
        outs.append(pos if voxel_units else pos.permute(0, 2, 1))
    return torch.cat(outs, 1)


def grid_sample_composition(c, coords, r):
    """functional/devoxelization.py:44-50 restated: the live trilinear_devoxelize (coords [B,3,N] in voxel units)"""
    g = (coords * 2 + 1.0) / r - 1.0
    g = g.permute(0, 2, 1).reshape(c.shape[0], 1, 1, -1, 3)
    g = torch.flip(g, dims=[-1])
    f = torch.nn.functional.grid_sample(input=c, grid=g, padding_mode='border', align_corners=False)
    return f.squeeze(dim=2).squeeze(dim=2)


def sample_f_composition(point_pos, c_list):
    """pc_model.py:182-194 restated"""
    p = (point_pos + 0.5).permute(0, 2, 1)
    return torch.cat([grid_sample_composition(c, torch.clamp(p * c.shape[-1], 0, c.shape[-1] - 1), c.shape[-1]) for c in c_list], dim=1)


# ---------------------------------------------------------------------------- the legacy devoxelization kernel (fp32)
def legacy_devoxelize(coords, feat, r):
    """coords f32 [B,3,N] in [0, r-1], feat f32 [B,C,r^3] -> outs f32 [B,C,N], inds i32 [B,8,N], wgts f32 [B,8,N]"""
    coords, feat = np.asarray(coords, f32), np.asarray(feat, f32)
    B, C = feat.shape[:2]
    lo_f = np.floor(coords)
    d1 = (coords - lo_f).astype(f32)
    d0 = (f32(1.0) - d1).astype(f32)
    lo = lo_f.astype(np.int32)
    hi = lo + (d1 > 0).astype(np.int32)
    inds, wgts = [], []
    for k in range(8):
        sel = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
        c = [hi[:, j] if sel[j] else lo[:, j] for j in range(3)]
        f = [d1[:, j] if sel[j] else d0[:, j] for j in range(3)]
        inds.append(c[0] * r * r + c[1] * r + c[2])
        wgts.append(((f[0] * f[1]).astype(f32) * f[2]).astype(f32))
    inds, wgts = np.stack(inds, 1).astype(np.int32), np.stack(wgts, 1).astype(f32)
    outs = None
    for k in range(8):
        term = (wgts[:, k][:, None, :] * np.take_along_axis(feat, np.broadcast_to(inds[:, k][:, None, :], (B, C, inds.shape[2])).astype(np.int64),
                                                            axis=2)).astype(f32)
        outs = term if outs is None else (outs + term).astype(f32)
    return outs, inds, wgts


def legacy_devoxelize_bwd(gy, inds, wgts, r):
    """fp64 scatter of w * g to the recorded indices -> [B,C,r^3]"""
    gy = np.asarray(gy, np.float64)
    B, C, N = gy.shape
    gx = np.zeros((B, C, r ** 3))
    for b in range(B):
        for k in range(8):
            for c in range(C):
                np.add.at(gx[b, c], inds[b, k], wgts[b, k].astype(np.float64) * gy[b, c])
    return gx
