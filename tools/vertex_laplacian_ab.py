#!/usr/bin/env python
"""A/B of the vertex Laplacian regulariser, fwd + bwd, on the same seeded inputs:

  (torch)  the path callers have today: torch.sparse.mm + elementwise + sum (DefTet.laplacian_sparse with a torch sparse
           adjacency) for the training form; pad, gather [P·m, C], sum, divide, mse_loss(reduction='none') for the render form
           (Deftet.get_featlap, diff_render/diftet_6_subdiv/3_model/deftet.py:221-241)
  (fused)  hip_ops.vertex_laplacian on a hip_ops.VertexAdjacency built once

Cases:
  train_res70   res 70 Kuhn grid, B = 8, C = 3, D⁻¹A (Tet_point_adj().run(..., normalize=True))
  train_res100  res 100, B = 8, C = 3
  render_res70  res 70 point table (hip_ops.point_adj_idx, stored as the reference does: +1, weights + 1e-10), B = 1, C = 7
                (the gridmov branch: torch.cat([color, weights, mov]))

Loss = (out * R).sum() with seeded R.  Build times are those of a second build (host syncs included).  The two paths alternate inside one process, each fwd+bwd timed with device events after
warm-ups; one JSON line per case with the median of the timed steps, the adjacency build times and the largest relative difference
of the outputs and of the gradients, which are first checked against the test tolerances (1e-5 relative).  Launch counts: run one
path alone (--only torch|fused) under rocprofv3 --kernel-trace --stats and divide the launches by the steps (--warmup + --steps).

    python tools/vertex_laplacian_ab.py [--cases train_res70 train_res100 render_res70] [--steps 20] [--warmup 5] [--only torch|fused]
    python tools/vertex_laplacian_ab.py --check      # tiny sizes; argument parsing and input generation up to the first GPU call
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402

CASES = {"train_res70": dict(form="train", res=70, B=8, C=3), "train_res100": dict(form="train", res=100, B=8, C=3),
         "render_res70": dict(form="render", res=70, B=1, C=7)}
RTOL = 1e-5


def make_inputs(case, res=None):
    """host side of a case: the Kuhn grid's tets, x [B,V,C] and the loss weights R (seeded)"""
    cfg = dict(CASES[case])
    if res is not None:
        cfg["res"] = res
    verts, tets = grids.kuhn_grid(cfg["res"])
    V = verts.shape[0]
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((cfg["B"], V, cfg["C"])) * 0.05).astype(np.float32)
    R_shape = (cfg["B"],) if cfg["form"] == "train" else (V, cfg["C"])
    R = rng.random(R_shape).astype(np.float32)
    return dict(cfg, V=V, tets=tets.astype(np.int32), x=x, R=R)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max().item() / max(b.abs().max().item(), 1e-30))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["torch", "fused"], help="time one path alone (for a kernel trace)")
    ap.add_argument("--check", action="store_true", help="tiny sizes, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.steps < 5:
        ap.error("--steps must be at least 5")
    inputs = {c: make_inputs(c, res=4 if args.check else None) for c in args.cases}
    if args.check:
        print(json.dumps({"check": "ok", "cases": {c: {k: d[k] for k in ("form", "res", "B", "C", "V")} for c, d in inputs.items()}}))
        return 0

    import torch
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    from deftet_amd.utils.lib.tet_point_adj.interface import Tet_point_adj
    dev = torch.device("cuda:0")
    layer = DefTet(device=dev)

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def build_ms(fn):
        """an adjacency build's time after one untimed build (first-call allocations, the library's workspace)"""
        fn()
        return timed(fn)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = events()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)

    for case in args.cases:
        d = inputs[case]
        x0, R = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["R"]).to(dev)
        tets = torch.from_numpy(d["tets"]).to(dev)
        build = {}
        if d["form"] == "train":
            torch_adj = Tet_point_adj().run(d["V"], d["tets"], normalize=True).to(dev)
            adj, build["from_sparse_ms"] = build_ms(lambda: hip_ops.VertexAdjacency.from_sparse(torch_adj))
            adj_t, build["from_tets_ms"] = build_ms(lambda: hip_ops.VertexAdjacency.from_tets(tets, d["V"], normalize=True))
            assert all(torch.equal(getattr(adj, k), getattr(adj_t, k)) for k in ("offsets", "cols", "vals", "t_offsets", "t_rows", "t_vals"))

            def torch_path(x):
                return layer.laplacian_sparse(x, torch_adj)

            def fused_path(x):
                return hip_ops.vertex_laplacian(x, adj, reduction="shape")
        else:
            table, adjsum = hip_ops.point_adj_idx(d["V"], tets)
            table1, w = table + 1, adjsum + 1e-10                 # as 3_model/deftet.py:160-161 stores them
            adj, build["from_table_ms"] = build_ms(lambda: hip_ops.VertexAdjacency.from_table(table1, w, index_base=1))
            P, m = table1.shape

            def torch_path(x):
                f = x[0]
                f1 = torch.nn.functional.pad(f, (0, 0, 1, 0))
                nei = f1[table1.view(-1), :].view(P, m, -1).sum(1) / w
                return torch.nn.functional.mse_loss(nei, f, reduction="none")

            def fused_path(x):
                return hip_ops.vertex_laplacian(x, adj, reduction="none")[0]
        paths = [("torch", torch_path), ("fused", fused_path)]
        if args.only:
            paths = [p for p in paths if p[0] == args.only]

        def step(fn):
            x = x0.clone().requires_grad_(True)
            out = fn(x)
            (out * R).sum().backward()
            return out.detach(), x.grad

        diff = None
        if not args.only:
            (o_t, g_t), (o_f, g_f) = step(torch_path), step(fused_path)
            diff = {"out": _rel(o_f, o_t), "grad": _rel(g_f, g_t)}
            if not (diff["out"] <= RTOL and diff["grad"] <= RTOL):
                raise SystemExit("%s: torch and fused paths disagree: %s" % (case, diff))
        times = {n: [] for n, _ in paths}
        for it in range(args.warmup + args.steps):
            for name, fn in paths:
                _, ms = timed(lambda: step(fn))
                if it >= args.warmup:
                    times[name].append(ms)
        row = {"case": case, "config": "res=%d V=%d B=%d C=%d nnz=%d" % (d["res"], d["V"], d["B"], d["C"], adj.nnz),
               "steps": args.steps, "warmup": args.warmup, "build": {k: round(v, 3) for k, v in build.items()},
               "max_rel_diff": diff}
        for name, _ in paths:
            t = np.asarray(times[name])
            row[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
