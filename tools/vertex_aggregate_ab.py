#!/usr/bin/env python
"""A/B of the GCN decoder's sparse product M·x (layers/gcn_decoder.py:55-56), fwd + bwd, on the same seeded inputs:

  (torch)  the reference-shaped path: transpose [B,V,C] to [V, B·C], torch.sparse.mm, transpose back, then .contiguous() as the
           nn.Linear that follows forces (utils/matrix_utils.py:22-33)
  (fused)  hip_ops.vertex_aggregate on a hip_ops.VertexAdjacency built once

Cases (M = D⁻¹A of the Kuhn grid, Tet_point_adj().run(..., normalize=True)):
  res70_c256  res 70 (V = 46,656), B = 8, C = 256      the decoder's four products at the headline size
  res70_c128  res 70, B = 8, C = 128                    a decoder configured half as wide
  res40_c256  res 40 (V = 9,261), B = 8, C = 256

Every step is out = path(x_s); grad = autograd.grad(out, x_s, g_s), timed with device events after warm-ups.  The inputs rotate
over as many (x_s, g_s) sets as it takes for the x_s together to exceed twice the 256 MiB Infinity Cache, so no step finds its
input cached by the step before.  The two paths alternate inside one process.  One JSON line per case: the median, smallest
and largest step time of each path, the rate on the algorithmic traffic — 2·B·V·C·4 bytes per direction (x read once, out
written once), two directions per step — and the largest difference of the outputs and gradients relative to their largest
entry, which is first checked against 1e-5.

    python tools/vertex_aggregate_ab.py [--cases res70_c256 res70_c128 res40_c256] [--steps 30] [--warmup 5] [--only torch|fused]
    python tools/vertex_aggregate_ab.py --check      # tiny sizes; argument parsing and input generation up to the first GPU call
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402

CASES = {"res70_c256": dict(res=70, B=8, C=256), "res70_c128": dict(res=70, B=8, C=128), "res40_c256": dict(res=40, B=8, C=256)}
RTOL = 1e-5
ROTATE_BYTES = 2 * 256 * 1024 * 1024


def make_inputs(case, res=None):
    """host side of a case: the Kuhn grid's tets, the sizes, the traffic and the number of rotating input sets"""
    cfg = dict(CASES[case])
    if res is not None:
        cfg["res"] = res
    verts, tets = grids.kuhn_grid(cfg["res"])
    V = verts.shape[0]
    x_bytes = cfg["B"] * V * cfg["C"] * 4
    return dict(cfg, V=V, tets=tets.astype(np.int32), pass_bytes=2 * x_bytes, sets=max(2, -(-ROTATE_BYTES // x_bytes)))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["torch", "fused"], help="time one path alone (for a kernel trace)")
    ap.add_argument("--check", action="store_true", help="tiny sizes, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.steps < 5:
        ap.error("--steps must be at least 5")
    inputs = {c: make_inputs(c, res=4 if args.check else None) for c in args.cases}
    if args.check:
        print(json.dumps({"check": "ok", "cases": {c: {k: d[k] for k in ("res", "B", "C", "V", "pass_bytes", "sets")}
                                                   for c, d in inputs.items()}}))
        return 0

    import torch
    from deftet_amd import hip_ops
    from deftet_amd.utils.lib.tet_point_adj.interface import Tet_point_adj
    dev = torch.device("cuda:0")

    def torch_path(x):
        b, n, p = x.shape
        flat = x.transpose(0, 1).reshape(n, b * p)
        return torch.sparse.mm(torch_adj, flat).reshape(n, b, p).transpose(0, 1).contiguous()

    def fused_path(x):
        return hip_ops.vertex_aggregate(x, adj)

    def step(fn, x, g):
        out = fn(x)
        (gx,) = torch.autograd.grad(out, x, g)
        return out.detach(), gx

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)

    for case in args.cases:
        d = inputs[case]
        B, V, C = d["B"], d["V"], d["C"]
        torch_adj = Tet_point_adj().run(V, d["tets"], normalize=True).to(dev)
        adj = hip_ops.VertexAdjacency.from_sparse(torch_adj)
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        sets = [(torch.randn(B, V, C, device=dev, generator=gen).requires_grad_(True), torch.randn(B, V, C, device=dev, generator=gen))
                for _ in range(d["sets"])]
        paths = [("torch", torch_path), ("fused", fused_path)]
        if args.only:
            paths = [p for p in paths if p[0] == args.only]
        diff = None
        if not args.only:
            (o_t, g_t), (o_f, g_f) = step(torch_path, *sets[0]), step(fused_path, *sets[0])
            diff = {"out": _rel(o_f, o_t), "grad": _rel(g_f, g_t)}
            if not (diff["out"] <= RTOL and diff["grad"] <= RTOL):
                raise SystemExit("%s: torch and fused paths disagree: %s" % (case, diff))
            del o_t, g_t, o_f, g_f
        times = {n: [] for n, _ in paths}
        for it in range(args.warmup + args.steps):
            x, g = sets[it % len(sets)]
            for name, fn in paths:
                _, ms = timed(lambda: step(fn, x, g))
                if it >= args.warmup:
                    times[name].append(ms)
        row = {"case": case, "config": "res=%d V=%d B=%d C=%d nnz=%d" % (d["res"], V, B, C, adj.nnz), "steps": args.steps,
               "warmup": args.warmup, "input_sets": len(sets), "step_bytes": 2 * d["pass_bytes"], "max_rel_diff": diff}
        for name, _ in paths:
            t = np.asarray(times[name])
            med = float(np.median(t))
            row[name] = {"median_ms": round(med, 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                         "gbytes_per_s": round(2 * d["pass_bytes"] / (med * 1e-3) / 1e9, 1)}
        if not args.only:
            row["torch_over_fused"] = round(row["torch"]["median_ms"] / row["fused"]["median_ms"], 2)
        print(json.dumps(row), flush=True)
        del sets, torch_adj, adj
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
