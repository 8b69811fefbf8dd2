"""The cases of tests/test_cell_gather_bits_gpu.py and tests/golden/gen_cell_gather_bits.py: the smallest that reach every branch
of the cell-sorted gather backward (cell_gather.hpp) through its three operators.  digests(device) runs them all and returns
{case: {output: SHA-256 of the raw bytes}}.  Every input comes from a seeded CPU torch.Generator and is then moved to the device.

  voxel.R.C.N        B = 2: (2, 3, 257) every point of a shape in ONE cell (R = 2 has one lo corner per axis), a segment > 32;
                     (5, 7, 1000) about 15 points per cell, segments <= 32 next to a few longer ones; (8, 65, 64) most cells empty
  voxel.clustered    R = 8, C = 3: 200 points in one cell (lanes 0 .. 7 add four terms, the others three), points on integer u
                     and points the clamp holds, interleaved
  voxel.chunked      B = 8, R = 32, C = 9, N = 300: a channel of partials is 8 MiB, the 64 MiB budget holds 8: chunks of 8 + 1
  legacy.R           trilinear_devoxelize_fwd / _bwd, B = 2, C = 3, N = 257 at R = 2 and 8; some inds[:,0,:] set to -1 and to R^3
                     before the backward (the sentinel key)
  image.H.W.C.N.*    B = 2: (1, 1, 1, 100), (2, 3, 7, 257) with G = 5 global rows and A = 3 appended rows, (5, 4, 64, 1000); each
                     under zeros / border and both align_corners; uv in [-1.3, 1.3]: fully-outside points (sentinel) and
                     partly-outside cells (x0 = -1)
  image.chunked      B = 8, H = W = 64, C = 130, N = 300: 540,800 bytes of partials per channel, 62 per 32 MiB: 62 + 62 + 6
  tet_centroid       B = 3, K = 257 chosen tets of the res-8 grid, volumes (5, 32^3), (3, 16^3), (4, 16^3): two share a sort
"""
import hashlib

import torch

VOXEL = [(2, 3, 257), (5, 7, 1000), (8, 65, 64)]
LEGACY = [2, 8]
IMAGE = [(1, 1, 1, 100), (2, 3, 7, 257), (5, 4, 64, 1000)]
IMAGE_WITH_ROWS = (2, 3, 7, 257)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _voxel(dev, gen, B, R, C, pos):
    from deftet_amd import hip_ops
    N = pos.shape[1]
    vol = torch.randn(B, C, R, R, R, generator=gen).to(dev).requires_grad_(True)
    gout = torch.randn(B, C, N, generator=gen).to(dev)
    pos = pos.to(dev).requires_grad_(True)
    out = hip_ops.voxel_sample([vol], pos)
    out.backward(gout)
    return {"out": sha(out), "grad_vol": sha(vol.grad), "grad_pos": sha(pos.grad)}


def _clustered_pos(gen, B, R):
    inside = (torch.tensor([3.0, 4.0, 5.0]) + torch.rand(B, 200, 3, generator=gen)) / R - 0.5
    on_integer = torch.randint(0, R, (B, 30, 3), generator=gen).float() / R - 0.5
    held = torch.where(torch.rand(B, 30, 3, generator=gen) < 0.5, -0.5 - torch.rand(B, 30, 3, generator=gen), 0.5 + torch.rand(B, 30, 3, generator=gen))
    pos = torch.cat([inside, on_integer, held], 1)
    return pos[:, torch.randperm(pos.shape[1], generator=gen)].contiguous()


def _legacy(dev, gen, B, R, C, N):
    from deftet_amd import hip_ops
    coords = (torch.rand(B, 3, N, generator=gen) * (R + 0.6) - 0.3).to(dev)
    feat = torch.randn(B, C, R ** 3, generator=gen).to(dev)
    gout = torch.randn(B, C, N, generator=gen).to(dev)
    outs, inds, wgts = hip_ops.trilinear_devoxelize_fwd(R, True, coords, feat)
    res = {"outs": sha(outs), "inds": sha(inds), "wgts": sha(wgts)}
    inds = inds.clone()
    inds[:, 0, 3:40:9] = -1
    inds[:, 0, 5:60:11] = R ** 3
    res["grad_x"] = sha(hip_ops.trilinear_devoxelize_bwd(gout, inds, wgts, R))
    return res


def _image(dev, gen, B, H, W, C, N, mode, align, G=0, A=0):
    from deftet_amd import hip_ops
    m = torch.randn(B, C, H, W, generator=gen).to(dev).requires_grad_(True)
    uv = (2.6 * torch.rand(B, N, 2, generator=gen) - 1.3).to(dev).requires_grad_(True)
    glob = torch.randn(B, G, generator=gen).to(dev).requires_grad_(True) if G else None
    app = torch.randn(B, N, A, generator=gen).to(dev).requires_grad_(True) if A else None
    gout = torch.randn(B, G + C + A, N, generator=gen).to(dev)
    out = hip_ops.image_sample([m], uv, global_features=glob, append=app, padding_mode=mode, align_corners=align)
    out.backward(gout)
    res = {"out": sha(out), "grad_map": sha(m.grad), "grad_uv": sha(uv.grad)}
    if G:
        res["grad_global"] = sha(glob.grad)
    if A:
        res["grad_append"] = sha(app.grad)
    return res


def _tet_centroid(dev, gen):
    from deftet_amd import grids, hip_ops
    B, K = 3, 257
    verts, tets = grids.kuhn_grid(8)
    V, T = verts.shape[0], tets.shape[0]
    pos = (torch.from_numpy(verts).float() - 0.5 + 0.01 * torch.randn(B, V, 3, generator=gen)).to(dev).requires_grad_(True)
    idx = torch.from_numpy(tets).to(dev)
    select = torch.randint(0, T, (K,), generator=gen).to(dev)
    vols = [torch.randn(B, c, r, r, r, generator=gen).to(dev).requires_grad_(True) for c, r in ((5, 32), (3, 16), (4, 16))]
    gout = torch.randn(B, 12 + 3, K, generator=gen).to(dev)
    out = hip_ops.tet_centroid_sample(vols, pos, idx, csr=hip_ops.tet_vertex_csr(idx, V), select=select)
    out.backward(gout)
    res = {"out": sha(out), "grad_pos": sha(pos.grad)}
    res.update({"grad_vol%d" % k: sha(v.grad) for k, v in enumerate(vols)})
    return res


def digests(dev):
    gen = torch.Generator().manual_seed(20240607)
    out = {}
    for R, C, N in VOXEL:
        out["voxel.%d.%d.%d" % (R, C, N)] = _voxel(dev, gen, 2, R, C, 1.05 * (torch.rand(2, N, 3, generator=gen) - 0.5))
    out["voxel.clustered"] = _voxel(dev, gen, 2, 8, 3, _clustered_pos(gen, 2, 8))
    out["voxel.chunked"] = _voxel(dev, gen, 8, 32, 9, 1.05 * (torch.rand(8, 300, 3, generator=gen) - 0.5))
    for R in LEGACY:
        out["legacy.%d" % R] = _legacy(dev, gen, 2, R, 3, 257)
    for H, W, C, N in IMAGE:
        G, A = (5, 3) if (H, W, C, N) == IMAGE_WITH_ROWS else (0, 0)
        for mode in ("zeros", "border"):
            for align in (False, True):
                out["image.%d.%d.%d.%d.%s.%d" % (H, W, C, N, mode, align)] = _image(dev, gen, 2, H, W, C, N, mode, align, G, A)
    out["image.chunked"] = _image(dev, gen, 8, 64, 64, 130, 300, "zeros", False)
    out["tet_centroid"] = _tet_centroid(dev, gen)
    return out
