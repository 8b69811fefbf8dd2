#!/usr/bin/env python
"""A/B of rasterize + composite, fwd + bwd, at BASELINE configs[4] scale (unique faces of the res 70 Kuhn grid projected by
grids.project_faces, 512 x 512 pixels from grids.pixel_grid, D = 4), for knum 64 and 300 and both saturation policies:

  (a) unfused  deftet_sparse_render (the [B,P,knum,D] layer stack) + alpha_composite (torch)
  (b) fused    deftet_sparse_render_composite (no layer stack)

Loss = (colour * R).sum() + (coverage * R').sum() with seeded R, R'.  The variants alternate inside one process, each step timed
with device events.  One JSON line per (knum, policy, variant): median ms and spread, the largest difference between (a) and (b)
in colour, coverage, grad_xy and grad_feat, and the variant's memory footprint.  The footprint is measured in a fresh child
process per variant (two fwd+bwd steps, nothing else): the absolute torch.cuda.max_memory_allocated of the second step
(peak_alloc_mb) and of the first (first_step_peak_alloc_mb, which also holds the workspace while it grows), both including the
inputs and the library workspace that _lib.workspace caches (grow-only, 1.25 x the largest request, kept for the process's
life), the cached workspace's size, and the forward / backward workspace requests.  Kernel times: run it under rocprofv3 --kernel-trace
--stats.

    python tools/render_composite_ab.py [--steps 20] [--warmup 3] [--res 70 --pixels 512] [--knum 64 300]
    python tools/render_composite_ab.py --check      # a tiny size; argument parsing and input generation up to the first GPU call
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402

NEAREST, FIRST = 0, 1


def make_inputs(res, pixels):
    """the faces and pixels of tests/test_raster_gpu.py's configs[4] scene, and the loss weights R, R' (seeded)"""
    from oracle import oracle as O
    verts, tets = grids.kuhn_grid(res)
    f3, _, _, _, _ = O.tet_to_face(tets, verts.shape[0], with_boundary=True)
    fz, fxy, ff = grids.project_faces(verts, f3)
    pix, rngs = grids.pixel_grid(pixels)
    P = pix.shape[1]
    rng = np.random.default_rng(7)
    R = rng.random((1, P, ff.shape[-1] - 1)).astype(np.float32)
    R2 = rng.random((1, P, 1)).astype(np.float32)
    return dict(pix=pix, rngs=rngs, fz=fz, fxy=fxy, ff=ff, R=R, R2=R2)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--pixels", type=int, default=512)
    ap.add_argument("--knum", type=int, nargs="+", default=[64, 300])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="tiny size, stop before the first GPU call")
    ap.add_argument("--memory-of", nargs=3, metavar=("VARIANT", "KNUM", "POLICY"), help=argparse.SUPPRESS)   # the child process
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.pixels, args.steps, args.warmup = 4, 16, 5, 1
    if args.steps < 5:
        ap.error("--steps must be at least 5")
    d = make_inputs(args.res, args.pixels)
    F, P = d["fz"].shape[1], d["pix"].shape[1]
    if args.check:
        print(json.dumps({"check": "ok", "F": F, "P": P, "knum": args.knum}))
        return 0

    import torch
    from deftet_amd import _lib
    from deftet_amd.render import alpha_composite, deftet_sparse_render, deftet_sparse_render_composite
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}

    def unfused(knum, policy):
        xy, ff = t["fxy"].clone().requires_grad_(True), t["ff"].clone().requires_grad_(True)
        layers, _ = deftet_sparse_render(t["pix"], t["rngs"], t["fz"], xy, ff, knum=knum, policy=policy)
        colour, cov, _ = alpha_composite(layers)
        del layers
        loss = (colour * t["R"]).sum() + (cov * t["R2"]).sum()
        loss.backward()
        return colour.detach(), cov.detach(), xy.grad, ff.grad

    def fused(knum, policy):
        xy, ff = t["fxy"].clone().requires_grad_(True), t["ff"].clone().requires_grad_(True)
        colour, cov, _, _ = deftet_sparse_render_composite(t["pix"], t["rngs"], t["fz"], xy, ff, knum=knum, policy=policy)
        loss = (colour * t["R"]).sum() + (cov * t["R2"]).sum()
        loss.backward()
        return colour.detach(), cov.detach(), xy.grad, ff.grad

    variants = [("unfused", unfused), ("fused", fused)]
    if args.memory_of:
        name, knum, policy = args.memory_of[0], int(args.memory_of[1]), int(args.memory_of[2])
        inputs = torch.cuda.memory_allocated(dev)
        dict(variants)[name](knum, policy)                         # first step: the workspace grows to its size
        torch.cuda.synchronize()
        first = torch.cuda.max_memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        dict(variants)[name](knum, policy)                         # second step: what every later step takes
        torch.cuda.synchronize()
        lib, D = _lib.load(), d["ff"].shape[-1]
        ws = {"unfused": (lib.deftet_sparse_render_workspace_bytes(1, P, F, knum), lib.deftet_sparse_render_bwd_workspace_bytes(1, P, F, knum)),
              "fused": (lib.deftet_sparse_render_composite_workspace_bytes(1, P, F, D, knum),
                        lib.deftet_sparse_render_composite_bwd_workspace_bytes(1, P, F, D, knum))}[name]
        print(json.dumps({"peak_alloc_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
                          "first_step_peak_alloc_mb": round(first / 2 ** 20, 1), "inputs_mb": round(inputs / 2 ** 20, 1),
                          "cached_workspace_mb": round(sum(b.numel() for b in _lib._ws.values()) / 2 ** 20, 1),
                          "fwd_workspace_mb": round(ws[0] / 2 ** 20, 1), "bwd_workspace_mb": round(ws[1] / 2 ** 20, 1)}))
        return 0

    def footprint(name, knum, policy):
        """the variant's memory, measured alone in a fresh process (one GPU process at a time)"""
        import subprocess
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--res", str(args.res), "--pixels", str(args.pixels),
                            "--memory-of", name, str(knum), str(policy)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("memory child for %s knum=%d failed (%d):\n%s" % (name, knum, r.returncode, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    for knum in args.knum:
        for policy in (NEAREST, FIRST):
            times = {n: [] for n, _ in variants}
            diff = None
            for step in range(args.warmup + args.steps):
                outs = {}
                for name, fn in variants:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    outs[name] = fn(knum, policy)
                    e1.record()
                    e1.synchronize()
                    if step >= args.warmup:
                        times[name].append(e0.elapsed_time(e1))
                if diff is None:
                    diff = {k: float((a.double() - b.double()).abs().max().item())
                            for k, a, b in zip(("colour", "coverage", "grad_xy", "grad_feat"), outs["unfused"], outs["fused"])}
                    diff.update({"max_abs_" + k: float(a.double().abs().max().item())
                                 for k, a in zip(("grad_xy", "grad_feat"), outs["unfused"][2:])})
                del outs
            for name, _ in variants:
                mem = footprint(name, knum, policy)
                x = np.asarray(times[name])
                print(json.dumps({"variant": name, "config": "res=%d pixels=%d^2 F=%d D=4" % (args.res, args.pixels, F), "knum": knum,
                                  "policy": "NEAREST" if policy == NEAREST else "FIRST", "steps": len(x),
                                  "median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4),
                                  "max_ms": round(float(x.max()), 4), "p10_ms": round(float(np.percentile(x, 10)), 4),
                                  "p90_ms": round(float(np.percentile(x, 90)), 4), "memory": mem, "max_diff_a_b": diff}),
                      flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
