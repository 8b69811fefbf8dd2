#!/usr/bin/env python
"""A/B of the occupancy query's fwd + bwd for a caller that owns the vertices, at BASELINE configs[2] (res 70 Kuhn grid, 100k
queries, B = 8; inputs made as bench.py makes them, 3 rotating sets):

  (a) gathered  tet_gather + point_in_tet(want_bary, pred, hits, order="auto", query_box="track") + point_in_tet_bwd_to_vertices
  (b) indexed   point_in_tet_indexed + point_in_tet_indexed_bwd_to_vertices, the same hints
  (c) dense     point_in_tet + point_in_tet_bwd_to_vertices on tets gathered beforehand (reference line: no gather in the step)

The variants alternate inside one process, each step timed with device events; every timed step of (a) and (b) is checked to
give the same bits (cond, weights, occ, grad_pos, grad_pts, grad_pred).  One JSON line per variant: median ms, spread, and the
algorithmic bytes of its tet-side inputs.  Kernel times: run it under rocprofv3 --kernel-trace --stats.

    python tools/occupancy_indexed_ab.py [--steps 30] [--warmup 5] [--res 70 --n-query 100000 --batch 8]
    python tools/occupancy_indexed_ab.py --check      # a tiny size; argument parsing and input generation up to the first GPU call
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402


def make_sets(res, n_query, batch, n_sets):
    """bench.py's recipe (N = 1): jittered Kuhn grid, uniform queries, per-set seeds"""
    verts, tets = grids.kuhn_grid(res)
    T = len(tets)
    sets = []
    for s in range(n_sets):
        base = s * 100_000
        pos = grids.jittered_positions(verts, res, batch, 0.1, seed0=1000 + base).astype(np.float32)
        pts = grids.random_queries(batch, n_query, seed0=2000 + base)
        gw = np.stack([np.random.default_rng(4000 + base + b).standard_normal((n_query, 4)).astype(np.float32) for b in range(batch)])
        pred = np.stack([np.random.default_rng(5000 + base + b).random(T).astype(np.float32) for b in range(batch)])
        gout = np.stack([np.random.default_rng(6000 + base + b).standard_normal(n_query).astype(np.float32) for b in range(batch)])
        sets.append(dict(pos=pos, pts=pts, gw=gw, pred=pred, gout=gout))
    return verts, tets, sets


def algorithmic_bytes(B, V, T):
    """bytes of the tet-side inputs each variant reads or writes per fwd + bwd (traversal, finalize, backward: three passes)"""
    dense = B * T * 48
    return {"gathered": B * V * 12 + T * 32 + dense + 3 * dense,   # the gather reads vertices + int64 list, writes the tets; 3 passes read them
            "indexed": 3 * (B * V * 12 + T * 16),                 # three passes read the vertices and the shared int32 list
            "dense": 3 * dense}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--n-query", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--check", action="store_true", help="tiny size, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.n_query, args.batch, args.sets, args.steps, args.warmup = 4, 200, 2, 2, 20, 1
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    verts, tets, sets = make_sets(args.res, args.n_query, args.batch, args.sets)
    B, V, T, Q = args.batch, len(verts), len(tets), args.n_query
    nbytes = algorithmic_bytes(B, V, T)
    if args.check:
        print(json.dumps({"check": "ok", "B": B, "V": V, "T": T, "Q": Q, "bytes": nbytes}))
        return 0

    import torch
    from deftet_amd import hip_ops
    dev = torch.device("cuda:0")
    idx32 = torch.from_numpy(tets.astype(np.int32)).to(dev)
    idx64 = idx32.long()                                         # what tet_gather reads
    csr = hip_ops.tet_vertex_csr(idx32, V)
    dsets = []
    for s in sets:
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in s.items()}
        d["tet"] = hip_ops.tet_gather(d["pos"], idx64)               # (c)'s input, gathered outside the timed region
        dsets.append(d)
    hints = dict(want_bary=True, want_hits=True, order="auto", query_box="track")

    def run_gathered(d):
        tet = hip_ops.tet_gather(d["pos"], idx64)
        cond, w, occ, hits = hip_ops.point_in_tet(tet, d["pts"], pred_bxt=d["pred"], **hints)
        g = hip_ops.point_in_tet_bwd_to_vertices(tet, d["pts"], cond, d["gw"], csr, V, want_grad_pts=True, grad_occ=d["gout"], hits=hits)
        return (cond, w, occ) + tuple(g)

    def run_indexed(d):
        cond, w, occ, hits = hip_ops.point_in_tet_indexed(d["pos"], idx32, d["pts"], pred_bxt=d["pred"], **hints)
        g = hip_ops.point_in_tet_indexed_bwd_to_vertices(d["pos"], idx32, d["pts"], cond, d["gw"], csr, want_grad_pts=True,
                                                         grad_occ=d["gout"], hits=hits)
        return (cond, w, occ) + tuple(g)

    def run_dense(d):
        cond, w, occ, hits = hip_ops.point_in_tet(d["tet"], d["pts"], pred_bxt=d["pred"], **hints)
        g = hip_ops.point_in_tet_bwd_to_vertices(d["tet"], d["pts"], cond, d["gw"], csr, V, want_grad_pts=True, grad_occ=d["gout"], hits=hits)
        return (cond, w, occ) + tuple(g)

    variants = [("gathered", run_gathered), ("indexed", run_indexed), ("dense", run_dense)]
    times = {n: [] for n, _ in variants}
    for step in range(args.warmup + args.steps):
        d = dsets[step % len(dsets)]
        outs = {}
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = fn(d)
            e1.record()
            e1.synchronize()
            if step >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
        for k, (x, y) in enumerate(zip(outs["gathered"], outs["indexed"])):
            if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
                raise SystemExit("step %d: output %d of the indexed path differs from the gathered path" % (step, k))
    for name, _ in variants:
        t = np.asarray(times[name])
        print(json.dumps({"variant": name, "config": "res=%d B=%d Q=%d T=%d V=%d" % (args.res, B, Q, T, V), "steps": len(t),
                          "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                          "max_ms": round(float(t.max()), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
                          "p90_ms": round(float(np.percentile(t, 90)), 4), "tet_side_bytes": nbytes[name]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
