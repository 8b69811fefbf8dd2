#!/usr/bin/env python
"""A/B of the generalised winding number on the same GPU, at the size of the per-step centroid labelling:

  (a) fast            hip_ops.winding_number(algo="fast"): octree build + point sort + wave-shared walk, every call
  (b) fast_unsorted   the same without the point sort (what the sort costs or saves)
  (c) exact           hip_ops.winding_number(algo="exact"): every point against every face
  (d) torch           the same sum as fp32 torch ops, points in chunks of 2^25 / F (on --torch-points points of ONE shape when the whole
                      job would take minutes; the line says so and scales the time up)
  (e) check_sign      hip_ops.check_sign, +x ray parity, for scale (closed meshes only)

Sizes: all tet centroids of the res 70 Kuhn grid (257,250), --batch (8) jittered shapes, against (1) the boundary of the tets within
0.3 of the centre (4,056 faces: the check_sign size of the README) and (2) a UV sphere of --big-lat (160) latitudes (101,760 faces).
Each timed step ends in a synchronise and is timed with the host clock; the variants alternate inside one process; medians over
--steps after --warmup.  Every size also reports the largest difference of (a), (b), (c) from (d) / from each other and whether (a)
and (b) are the same bits.  One JSON line per variant and size, then one line with what AUTO resolves to.

--sweep adds the crossover of AUTO: fast against exact on UV spheres of 48 to 2,208 faces, for all centroids of the batch and for the
first 4,096 centroids of one shape (one JSON line per size with both medians), and what the point sort is for: fast with and without
it on the same centroids in a random order.

    python tools/winding_number_ab.py [--steps 5] [--warmup 2] [--res 70 --batch 8] [--no-big] [--sweep]
    python tools/winding_number_ab.py --check      # a tiny size; argument parsing and input generation up to the first GPU call
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402


def tet_boundary(verts, tets, radius=0.3):
    """outward faces of the union of the tets whose centroid lies within `radius` of the centre (int64 [F,3])"""
    keep = np.linalg.norm((verts - 0.5)[tets].mean(1), axis=1) < radius
    t = tets[keep].astype(np.int64)
    f = np.concatenate([t[:, [0, 2, 1]], t[:, [0, 1, 3]], t[:, [0, 3, 2]], t[:, [1, 2, 3]]])     # outward for positive tets
    _, first, count = np.unique(np.sort(f, 1), axis=0, return_index=True, return_counts=True)
    return np.ascontiguousarray(f[np.sort(first[count == 1])])


def uv_sphere(n_lat, radius=0.4):
    n_lon = 2 * n_lat
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2.0 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.repeat(np.cos(th)[:, None], n_lon, 1)], -1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]]) * radius
    s = np.arange(n_lon)
    s1 = (s + 1) % n_lon
    r0 = (1 + np.arange(n_lat - 2) * n_lon)[:, None]
    a, b, c, d = r0 + s[None], r0 + n_lon + s[None], r0 + n_lon + s1[None], r0 + s1[None]
    rl = 1 + (n_lat - 2) * n_lon
    f = np.concatenate([np.stack([np.zeros(n_lon, np.int64), 1 + s, 1 + s1], 1),
                        np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3),
                        np.stack([np.full(n_lon, v.shape[0] - 1), rl + s1, rl + s], 1)])
    return v.astype(np.float32), np.ascontiguousarray(f.astype(np.int64))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-lat", type=int, default=160)
    ap.add_argument("--torch-points", type=int, default=16384, help="points of one shape the torch row runs on when the whole job is too long")
    ap.add_argument("--no-big", action="store_true", help="skip the 100k-face mesh")
    ap.add_argument("--sweep", action="store_true", help="also time fast against exact on small meshes (the crossover of AUTO)")
    ap.add_argument("--check", action="store_true", help="tiny size, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.batch, args.big_lat = 8, 2, 6
    verts, tets = grids.kuhn_grid(args.res)
    pos = grids.jittered_positions(verts, args.res, args.batch, 0.1)
    cen = pos[:, tets.astype(np.int64)].mean(2).astype(np.float32)
    faces = tet_boundary(verts, tets)
    sv, sf = uv_sphere(args.big_lat)
    if args.check:
        print(json.dumps({"check": "ok", "B": args.batch, "N": int(cen.shape[1]), "faces": int(faces.shape[0]), "big_faces": int(sf.shape[0])}))
        return 0

    import torch
    from deftet_amd import _lib, hip_ops
    dev = torch.device("cuda:0")

    def torch_wn(v, f, p, budget=1 << 25):
        """fp32, v [V,3], f [F,3], p [P,3] -> [P]"""
        c = v[f]
        out = []
        step = max(1, budget // max(int(f.shape[0]), 1))
        for s in range(0, p.shape[0], step):
            q = p[s:s + step, None, :]
            a, b, cc = c[None, :, 0] - q, c[None, :, 1] - q, c[None, :, 2] - q
            la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), cc.norm(dim=-1)
            det = (a * torch.linalg.cross(b, cc)).sum(-1)
            den = la * lb * lc + (a * b).sum(-1) * lc + (b * cc).sum(-1) * la + (cc * a).sum(-1) * lb
            out.append(torch.atan2(det, den).sum(1) / (2.0 * np.pi))
        return torch.cat(out)

    def run_size(label, v, f, p, closed):
        B, N, F = p.shape[0], p.shape[1], f.shape[0]
        whole = B * N * F <= 2e10
        tp = p if whole else p[:1, :args.torch_points]

        def torch_step():
            return torch.stack([torch_wn(v[b], f, tp[b]) for b in range(tp.shape[0])])
        variants = [("fast", lambda: hip_ops.winding_number(v, f, p, algo="fast", check=False)),
                    ("fast_unsorted", lambda: hip_ops.winding_number(v, f, p, algo="fast_unsorted", check=False)),
                    ("exact", lambda: hip_ops.winding_number(v, f, p, algo="exact", check=False)),
                    ("torch", torch_step)]
        if closed:
            variants.append(("check_sign", lambda: hip_ops.check_sign(v, f, p, check=False)))
        times, outs = {n: [] for n, _ in variants}, {}
        for step in range(args.warmup + args.steps):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        ref = outs["torch"]
        sl = (slice(None), slice(None)) if whole else (slice(0, 1), slice(0, args.torch_points))
        for name, _ in variants:
            t = np.asarray(times[name])
            line = {"variant": name, "size": label, "B": B, "N": N, "F": F, "L": int(_lib.load().deftet_winding_number_levels(F)),
                    "steps": len(t), "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}
            if name == "torch" and not whole:
                scale = B * N / float(tp.shape[0] * tp.shape[1])
                line.update(points_timed=int(tp.shape[0] * tp.shape[1]), median_ms_scaled_to_all_points=round(float(np.median(t)) * scale, 1))
            if name in ("fast", "fast_unsorted", "exact"):
                line["max_abs_diff_vs_torch_fp32"] = float((outs[name][sl] - ref).abs().max())
            if name == "fast":
                line.update(same_bits_as_unsorted=bool(torch.equal(outs["fast"], outs["fast_unsorted"])),
                            max_abs_diff_vs_exact=float((outs["fast"] - outs["exact"]).abs().max()))
            if name == "check_sign":
                line["parity_rule_mismatches_vs_exact"] = int((hip_ops.winding_inside(outs["exact"], "parity") != outs[name]).sum())
            print(json.dumps(line), flush=True)
        return {n: float(np.median(times[n])) for n in times}

    p = torch.from_numpy(cen).to(dev)
    med = run_size("tet boundary, res %d" % args.res, torch.from_numpy(pos).to(dev), torch.from_numpy(faces).to(dev), p, True)
    sizes = {int(faces.shape[0]): med}
    if not args.no_big:
        vb = torch.from_numpy(np.stack([sv * (1.0 - 0.02 * b) for b in range(args.batch)]).astype(np.float32)).to(dev)
        sizes[int(sf.shape[0])] = run_size("uv sphere %d" % args.big_lat, vb, torch.from_numpy(sf).to(dev), p, True)
    lib = _lib.load()
    if args.sweep:
        for pts in (p, p[:1, :4096].contiguous()):
            for n_lat in (4, 6, 8, 12, 16, 24):
                v1, f1 = uv_sphere(n_lat)
                v = torch.from_numpy(np.repeat(v1[None], pts.shape[0], 0)).to(dev)
                f = torch.from_numpy(f1).to(dev)
                t = {"fast": [], "exact": []}
                for step in range(args.warmup + args.steps):
                    for name in t:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        hip_ops.winding_number(v, f, pts, algo=name, check=False)
                        torch.cuda.synchronize()
                        if step >= args.warmup:
                            t[name].append((time.perf_counter() - t0) * 1e3)
                F, n_all = int(f1.shape[0]), int(pts.shape[0] * pts.shape[1])
                print(json.dumps({"sweep": "uv sphere %d" % n_lat, "B": int(pts.shape[0]), "N": int(pts.shape[1]), "F": F,
                                  "fast_median_ms": round(float(np.median(t["fast"])), 4), "exact_median_ms": round(float(np.median(t["exact"])), 4),
                                  "auto": {1: "exact", 2: "fast"}[lib.deftet_winding_number_resolve_algo(0, F, n_all)]}), flush=True)
        # what the point sort is for: the same centroids in a random order per shape (every wave's 64 points all over the box)
        order = torch.stack([torch.randperm(p.shape[1], device=dev, generator=torch.Generator(device=dev).manual_seed(b)) for b in range(p.shape[0])])
        shuffled = torch.gather(p, 1, order[:, :, None].expand(-1, -1, 3)).contiguous()
        meshes = [("tet boundary, res %d" % args.res, torch.from_numpy(pos).to(dev), torch.from_numpy(faces).to(dev))]
        if not args.no_big:
            meshes.append(("uv sphere %d" % args.big_lat, vb, torch.from_numpy(sf).to(dev)))
        for label, v, f in meshes:
            t = {"fast": [], "fast_unsorted": []}
            for step in range(args.warmup + args.steps):
                for name in t:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hip_ops.winding_number(v, f, shuffled, algo=name, check=False)
                    torch.cuda.synchronize()
                    if step >= args.warmup:
                        t[name].append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"shuffled_points": label, "B": int(p.shape[0]), "N": int(p.shape[1]), "F": int(f.shape[0]),
                              "fast_median_ms": round(float(np.median(t["fast"])), 4),
                              "fast_unsorted_median_ms": round(float(np.median(t["fast_unsorted"])), 4)}), flush=True)
    print(json.dumps({"auto": {str(F): {1: "exact", 2: "fast"}[lib.deftet_winding_number_resolve_algo(0, F, args.batch * int(cen.shape[1]))] for F in sizes},
                      "faster": {str(F): min(("fast", "exact"), key=lambda n: m[n]) for F, m in sizes.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
