#!/usr/bin/env python
"""A/B of marching tetrahedra, forward + backward, on the same GPU:

  (a) hip      hip_ops.marching_tets (count + scan + finish, one read-back of the offsets, fill) and its CSR backward
  (b) torch    the DMTet-style restatement in torch: gather the edge ends, sign codes, `nonzero` for the crossing edges and the
               mixed tets (each a synchronisation), table look-ups for the faces, autograd for the backward (`index_put_` /
               `index_add_` with atomics)

Sizes: the jittered Kuhn grid at --res (70) with --batch (8) sphere fields of different radii, and the res 40 grid after two
hip_ops.subdivide levels with one shape.  Both sides get the same precomputed topology (edge list, tet -> edge table); the
timed step is forward + backward with N(0,1) gradients on the vertices, ends in a synchronise and is timed with the host clock;
the variants alternate inside one process and rotate over three input sets; medians over --steps after --warmup.  Every step
compares the vertices and faces of the two sides bit for bit and the gradients by their max-norm difference.  The vertex
gradients are made before the timed steps; the hip side's step includes the two `torch.cat` of its per-shape lists.  One JSON line
per variant and size, with the number of kernel launches per step as the profiler counts them.

    python tools/marching_tets_ab.py [--steps 20] [--warmup 3] [--res 70 --batch 8] [--no-subdivided]
    python tools/marching_tets_ab.py --check      # a tiny size; argument parsing and input generation up to the first GPU call
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

# case code -> crossing local edges (cyclic from the lowest id, -1 padded) and triangle count: DESIGN.md §6l
TABLE = [[-1, -1, -1, -1], [0, 1, 2, -1], [0, 4, 3, -1], [1, 2, 4, 3], [1, 3, 5, -1], [0, 3, 5, 2], [0, 4, 5, 1], [2, 4, 5, -1],
         [2, 5, 4, -1], [0, 1, 5, 4], [0, 2, 5, 3], [1, 5, 3, -1], [1, 3, 4, 2], [0, 3, 4, -1], [0, 2, 1, -1], [-1, -1, -1, -1]]
NTRI = [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def make_inputs(res, batch, sets=3):
    verts, tets = grids.kuhn_grid(res)
    pos = [grids.jittered_positions(verts, res, batch, 0.1, seed0=1000 + 50 * s) for s in range(sets)]
    radii = [[0.2 + 0.2 * (b + 0.3 * s) / max(batch, 1) for b in range(batch)] for s in range(sets)]
    field = [np.stack([(np.float32(r) - np.linalg.norm(p[b], axis=-1)).astype(np.float32) for b, r in enumerate(rs)])
             for p, rs in zip(pos, radii)]
    return tets.astype(np.int64), pos, field


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-subdivided", action="store_true", help="skip the res 40 grid after two subdivision levels")
    ap.add_argument("--check", action="store_true", help="tiny size, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.batch = 4, 2
    tets, pos, field = make_inputs(args.res, args.batch)
    if args.check:
        print(json.dumps({"check": "ok", "B": args.batch, "V": int(pos[0].shape[1]), "T": int(tets.shape[0]),
                          "inside": [int((f > 0).sum()) for f in field]}))
        return 0

    import torch
    from deftet_amd import hip_ops
    dev = torch.device("cuda:0")
    table, ntri = torch.tensor(TABLE, device=dev), torch.tensor(NTRI, device=dev)
    weights = torch.tensor([1, 2, 4, 8], device=dev)

    def torch_route(p, f, top, iso=0.0):
        B, E = f.shape[0], top.n_edge
        e0, e1, tt, te = top.edges[:, 0].long(), top.edges[:, 1].long(), top.tets.long(), top.tet_edge.long()
        inside = f.detach() > iso
        cross = inside[:, e0] != inside[:, e1]
        b, e = torch.nonzero(cross).unbind(1)                                       # (sync)
        lo, hi = e0[e], e1[e]
        f0, f1 = f[b, lo], f[b, hi]
        t = (iso - f0) / (f1 - f0)
        verts = p[b, lo] + t[:, None] * (p[b, hi] - p[b, lo])
        nv = torch.cumsum(cross.sum(1), 0)
        first_v = torch.cat([nv.new_zeros(1), nv])
        ev = torch.full((B, E), -1, dtype=torch.long, device=dev)
        ev[b, e] = torch.arange(b.numel(), device=dev) - first_v[b]
        code = (inside[:, tt] * weights).sum(-1)
        n = ntri[code]
        tb, ti = torch.nonzero(n > 0).unbind(1)                                     # (sync)
        q = ev[tb[:, None], te[ti[:, None], table[code[tb, ti]].clamp(min=0)]]      # [M,4]
        both = torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1)                   # [M,2,3]
        keep = torch.stack([torch.ones_like(tb, dtype=torch.bool), n[tb, ti] == 2], 1)
        faces = both[keep]                                                          # (sync)
        first_f = torch.cat([nv.new_zeros(1), torch.cumsum(n.sum(1), 0)])
        offs = torch.stack([first_v, first_f]).tolist()                             # the read-back the caller splits by
        return verts, faces, offs

    def run_size(label, top, pos_sets, field_sets):
        B, V = field_sets[0].shape
        leaves = [(p.clone().requires_grad_(True), f.clone().requires_grad_(True)) for p, f in zip(pos_sets, field_sets)]
        gen = torch.Generator(device=dev).manual_seed(3)
        # the vertex gradients of every input set, made before anything is timed (one untimed forward gives the row count)
        grads_out = []
        with torch.no_grad():
            for p, f in leaves:
                n = sum(int(v.shape[0]) for v in hip_ops.marching_tets(p, f, top).verts)
                grads_out.append(torch.randn(n, 3, device=dev, generator=gen))

        def hip_step(s):
            p, f = leaves[s]
            m = hip_ops.marching_tets(p, f, top)
            verts = torch.cat(m.verts)                                              # (the per-shape lists joined for the comparison:
            return verts, torch.cat(m.faces), torch.autograd.grad((verts * grads_out[s]).sum(), (p, f))   # two launches only this side pays)

        def torch_step(s):
            p, f = leaves[s]
            verts, faces, _offs = torch_route(p, f, top)
            return verts, faces, torch.autograd.grad((verts * grads_out[s]).sum(), (p, f))
        times = {"hip": [], "torch": []}
        same_bits, grad_err, rows = True, 0.0, (0, 0)
        for step in range(args.warmup + args.steps):
            s = step % len(leaves)
            outs = {}
            for name, fn in (("hip", hip_step), ("torch", torch_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn(s)
                torch.cuda.synchronize()
                if step >= args.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
            (va, fa, ga), (vb, fb, gb) = outs["hip"], outs["torch"]
            same_bits = same_bits and torch.equal(va, vb) and torch.equal(fa, fb)
            for x, y in zip(ga, gb):
                grad_err = max(grad_err, float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)))
            rows = (int(va.shape[0]), int(fa.shape[0]))
        launches = {}
        for name, fn in (("hip", hip_step), ("torch", torch_step)):
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn(0)
                    torch.cuda.synchronize()
                ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
                launches[name] = {"kernels": sum(1 for e in ev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()),
                                  "copies_and_memsets": sum(1 for e in ev if "memcpy" in e.name.lower() or "memset" in e.name.lower())}
            except Exception as exc:                                                # the profiler is not what is measured here
                launches[name] = "not counted (%s)" % type(exc).__name__
        for name in ("hip", "torch"):
            t = np.asarray(times[name])
            line = {"variant": name, "size": label, "B": B, "V": V, "T": top.n_tet, "E": top.n_edge, "verts": rows[0], "faces": rows[1],
                    "steps": len(t), "fwd_bwd_median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                    "max_ms": round(float(t.max()), 4), "launches_per_step": launches[name]}
            if name == "hip":
                line.update(same_bits_as_torch=bool(same_bits), grad_maxnorm_diff_vs_torch=grad_err,
                            speedup_vs_torch=round(float(np.median(times["torch"]) / np.median(t)), 2))
            print(json.dumps(line), flush=True)

    t64 = torch.from_numpy(tets).to(dev)
    top = hip_ops.TetEdges(t64, pos[0].shape[1])
    run_size("kuhn res %d" % args.res, top, [torch.from_numpy(p).to(dev) for p in pos], [torch.from_numpy(f).to(dev) for f in field])
    if not args.no_subdivided:
        verts, tets40 = grids.kuhn_grid(40)
        pos2, fields = [], []
        for s, r in enumerate((0.28, 0.3, 0.32)):                                  # three jitter seeds: the subdivided list is the same
            p = torch.from_numpy(grids.jittered_positions(verts, 40, 1, 0.1, seed0=1000 + 50 * s)[0]).to(dev)
            t = torch.from_numpy(tets40.astype(np.int64)).to(dev)
            for _level in range(2):
                p, _f, t = hip_ops.subdivide(t, p, p[:, :1].contiguous())
            pos2.append(p[None].contiguous())
            fields.append((r - p.norm(dim=1))[None].contiguous())
        run_size("kuhn res 40, two subdivision levels", hip_ops.TetEdges(t, p.shape[0]), pos2, fields)
    return 0


if __name__ == "__main__":
    sys.exit(main())
