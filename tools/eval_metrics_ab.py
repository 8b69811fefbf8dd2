#!/usr/bin/env python
"""A/B of eval.py's metric block (eval.py:237-260) for a batch of shapes, two ways on the same inputs:

  (lib)    deftet_amd.metrics.surface_metrics: sampling, both sided distances, both point-to-mesh queries, the fused reduction
  (torch)  a torch-only restatement: torch.multinomial face choice, chunked torch.cdist minima, a chunked torch point-triangle
           scan (Ericson, fp32) and the same formulas

Default sizes are the evaluation's: 100k surface points, 100k samples, 100k SDF points (IoU by check_sign, both paths), a
predicted surface made of the boundary faces of a sphere-like occupancy on the res-70 grid, and a closed ground-truth mesh of
about 100k faces (a UV sphere; the reference does not record how large its ground-truth meshes are, so 100k is an assumption).
Both paths alternate in one process, timed with device events after warm-up; one JSON line with the medians, spreads and ratio
and the largest difference of the outputs.

    python tools/eval_metrics_ab.py [--points 100000] [--gt-faces 100000] [--res 70] [--batch 1] [--reps 20] [--warmup 2]
    python tools/eval_metrics_ab.py --dry-run      # build the inputs up to the first GPU call
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402


def predicted_surface(res, radius=0.35):
    """boundary faces (outward or not: unsigned distances) of the tets of the res grid whose centroid lies in a ball"""
    verts, tets = grids.kuhn_grid(res)
    verts = verts.astype(np.float32) - 0.5
    occ = np.linalg.norm(verts[tets].mean(1), axis=1) < radius
    t = tets[occ]
    faces = np.concatenate([t[:, [0, 1, 2]], t[:, [0, 1, 3]], t[:, [0, 2, 3]], t[:, [1, 2, 3]]])
    key = np.sort(faces, axis=1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return verts, faces[cnt[inv.reshape(-1)] == 1]


def uv_sphere(n_faces, radius=0.36):
    """closed sphere of about n_faces faces (rings x segments, one vertex per pole)"""
    n_lat = max(int(np.sqrt(n_faces / 4)), 3)
    n_lon = 2 * n_lat
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph), np.repeat(np.cos(th)[:, None], n_lon, 1)], -1)
    v = np.concatenate([[[0, 0, 1]], ring.reshape(-1, 3), [[0, 0, -1]]]) * radius
    idx = lambda r, s: 1 + r * n_lon + (s % n_lon)                      # noqa: E731
    f = [[0, idx(0, s), idx(0, s + 1)] for s in range(n_lon)]
    for r in range(n_lat - 2):
        for s in range(n_lon):
            f += [[idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)], [idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)]]
    last = len(v) - 1
    f += [[last, idx(n_lat - 2, s + 1), idx(n_lat - 2, s)] for s in range(n_lon)]
    return v.astype(np.float32), np.array(f, np.int64)


def make_inputs(a):
    rng = np.random.default_rng(5)
    pv, pf = predicted_surface(a.res)
    gv, gf = uv_sphere(a.gt_faces)
    gtri = gv[gf]
    # ground-truth surface cloud: area-uniform on the GT mesh
    ar = np.linalg.norm(np.cross(gtri[:, 1] - gtri[:, 0], gtri[:, 2] - gtri[:, 0]), axis=1)
    ch = rng.choice(len(gf), size=(a.batch, a.points), p=ar / ar.sum())
    u = rng.random((2, a.batch, a.points, 1)).astype(np.float32)
    s = np.sqrt(u[0])
    surf = (1 - s) * gtri[ch, 0] + s * (1 - u[1]) * gtri[ch, 1] + s * u[1] * gtri[ch, 2]
    sdf = (rng.random((a.batch, a.points, 3)).astype(np.float32) - 0.5) * 1.05
    occ = (np.linalg.norm(sdf, axis=-1) < 0.36).astype(np.float32)
    return dict(pv=pv, pf=pf, gv=gv, gf=gf, surf=surf.astype(np.float32), sdf=sdf, occ=occ)


def torch_tri_dist(p, a, b, c):
    """Ericson in fp32 torch: p [n,1,3], a/b/c [1,F,3] -> squared distance [n,F] (branch order kept through where)"""
    import torch
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]   # noqa: E731
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    den = 1.0 / (va + vb + vc)
    q = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    e43, e56 = d4 - d3, d5 - d6
    q = torch.where(((va <= 0) & (e43 >= 0) & (e56 >= 0))[..., None], b + (e43 / (e43 + e56))[..., None] * (c - b), q)
    q = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + (d2 / (d2 - d6))[..., None] * ac, q)
    q = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c.expand_as(q), q)
    q = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + (d1 / (d1 - d3))[..., None] * ab, q)
    q = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b.expand_as(q), q)
    q = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a.expand_as(q), q)
    return ((p - q) ** 2).sum(-1)


def torch_metrics(surf, pred_tri, gt_tri, n_samples, gen, chunk=2048, tri_chunk=128):
    import torch
    B = surf.shape[0]
    out = []
    for bi in range(B):
        t = pred_tri[bi]
        area = 0.5 * torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).norm(dim=-1)
        ch = torch.multinomial(area, n_samples, replacement=True, generator=gen)
        u = torch.rand(n_samples, 2, device=t.device, generator=gen)
        s = u[:, :1].sqrt()
        pts = (1 - s) * t[ch, 0] + s * (1 - u[:, 1:]) * t[ch, 1] + s * u[:, 1:] * t[ch, 2]
        S1 = surf[bi]

        def sided(x, y):
            d, i = [], []
            for k in range(0, x.shape[0], chunk):
                m = torch.cdist(x[k:k + chunk], y).min(1)
                d.append(m.values ** 2)
                i.append(m.indices)
            return torch.cat(d), torch.cat(i)

        def p2m(x, tri):
            a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
            return torch.cat([torch_tri_dist(x[k:k + tri_chunk, None], a, b, c).min(1).values for k in range(0, x.shape[0], tri_chunk)])

        d12, i12 = sided(S1, pts)
        d21, i21 = sided(pts, S1)
        pd, gd = (d12 + 1e-15).sqrt(), (d21 + 1e-15).sqrt()
        prec = (gd <= 0.01).float().sum() / gd.numel()
        rec = (pd <= 0.01).float().sum() / pd.numel()
        da, db = p2m(S1, t), p2m(pts, gt_tri[bi])
        sa, sb = (da + 1e-15).sqrt(), (db + 1e-15).sqrt()
        out.append(torch.stack([(pd.mean() + gd.mean()) / 2, (S1 - pts[i12]).abs().sum(-1).mean() + (pts - S1[i21]).abs().sum(-1).mean(),
                                2 * prec * rec / (prec + rec + 1e-8), ((sa + sb) / 2).mean(), (sa.max() + sb.max()) / 2]))
    return torch.stack(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--gt-faces", type=int, default=100000)
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args(argv)
    inp = make_inputs(a)
    if a.dry_run:
        print("dry run: %d predicted faces, %d ground-truth faces, %d points x %d shapes" % (len(inp["pf"]), len(inp["gf"]), a.points, a.batch))
        return 0
    import torch
    from deftet_amd import metrics
    dev = torch.device("cuda:0")
    B = a.batch
    pv, gv = torch.from_numpy(inp["pv"]).to(dev), torch.from_numpy(inp["gv"]).to(dev)
    pf, gf = torch.from_numpy(inp["pf"]).to(dev), torch.from_numpy(inp["gf"]).to(dev)
    pred_tri = pv[pf][None].expand(B, -1, -1, -1).contiguous()
    gt_tri = gv[gf][None].expand(B, -1, -1, -1).contiguous()
    surf, sdf = torch.from_numpy(inp["surf"]).to(dev), torch.from_numpy(inp["sdf"]).to(dev)
    occ = torch.from_numpy(inp["occ"]).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def run_lib():
        r = metrics.surface_metrics(pred_tri, None, gt_tri, None, surf, num_samples=a.points, generator=gen, pred_verts=[pv] * B,
                                    pred_faces_idx=[pf] * B, sdf_points=sdf, gt_occ=occ)
        return torch.stack([r[k] for k in ("chamfer", "chamfer_l1", "f_score", "mean_hausdorff", "max_hausdorff", "iou")], 1)

    def run_torch():
        m = torch_metrics(surf, pred_tri, gt_tri, a.points, gen)
        inside = torch.stack([metrics.hip_ops.check_sign(pv[None], pf, sdf[b:b + 1])[0] for b in range(B)]).float()
        g = (occ > 0).float()
        return torch.cat([m, ((inside * g).sum(-1) / (inside + g).clamp(0, 1).sum(-1))[:, None]], 1)

    times = {"lib": [], "torch": []}
    outs = {}
    with torch.no_grad():
        for it in range(a.warmup + a.reps):
            for name, fn in (("lib", run_lib), ("torch", run_torch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[name] = fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: [float(np.min(v)), float(np.max(v))] for k, v in times.items()}
    diff = (outs["lib"].double() - outs["torch"].double()).abs().max(0).values.cpu().tolist()
    print(json.dumps(dict(tool="eval_metrics_ab", batch=B, points=a.points, pred_faces=int(len(inp["pf"])), gt_faces=int(len(inp["gf"])),
                          reps=a.reps, median_ms=med, spread_ms=spread, ratio=med["torch"] / med["lib"],
                          max_abs_diff=dict(zip(["chamfer", "chamfer_l1", "f_score", "mean_hausdorff", "max_hausdorff", "iou"], diff)),
                          lib=outs["lib"].cpu().tolist(), torch=outs["torch"].cpu().tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
