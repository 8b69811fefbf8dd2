#!/usr/bin/env python
"""A/B of conforming selective refinement at res 70 (Kuhn grid, T = 257,250): the tets selected are occupancy_band(rings=1) of the
occupancy of a sphere of radius 0.3 — the band a surface needs refined.

  (a) refine        hip_ops.refine_tets: tet_edges, the closure sweeps (4 per read-back), count and fill
  (b) refine_edges  the same with edges / tet_edge handed in (a caller that refines one topology repeatedly)
  (c) uniform       hip_ops.subdivide(..., None) on the same grid: what reaches the band's resolution without this operator,
                    eight times the tets everywhere
  (d) host          the numpy restatement tests/refine_ref.py on the host (inputs already there, nothing uploaded)

The GPU variants alternate inside one process; every call ends in a synchronise and is timed with the host clock; every timed
step checks (a) against (b) bit for bit, and the first one (a) against (d).  One JSON line per variant: median ms with min and
max, T' and M, the sweeps and read-backs of the closure and the marks every sweep set (sweeps_per_sync 1 and 4), per-kernel times
of (a) from deftet_profile_select.

    python tools/tet_refine_ab.py [--steps 20] [--warmup 3] [--host-steps 3] [--res 70]
    python tools/tet_refine_ab.py --check      # a tiny size; argument parsing, input generation and the host variant, no GPU call
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402
from tests import refine_ref as R  # noqa: E402

KERNELS = ("k_refine_init", "k_refine_sweep", "k_refine_edge_check", "k_refine_children", "k_refine_totals", "k_refine_copy",
           "k_refine_midpoints", "k_refine_split", "k_refine_tets")


def make_inputs(res, n_feat=4):
    verts, tets = grids.kuhn_grid(res)
    pts = (verts - 0.5).astype(np.float32)
    feat = np.random.default_rng(res).random((pts.shape[0], n_feat)).astype(np.float32)
    return tets.astype(np.int64), pts, feat, R.sphere_inside(pts, tets, 0.3)


def stats(t):
    t = np.asarray(t)
    return {"steps": int(t.size), "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="tiny size, host variant only, no GPU call")
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.host_steps = 8, 1
    tets, pts, feat, inside = make_inputs(args.res)
    T, P = tets.shape[0], pts.shape[0]
    config = "res=%d T=%d P=%d K=%d" % (args.res, T, P, feat.shape[1])
    if args.check:
        select = R.occupancy_band(inside, R.neighbour_table(tets), 1)
        want = R.refine(tets, pts, feat, select)
        print(json.dumps({"check": "ok", "config": config, "selected": int(select.sum()), "T_new": int(want.tet_new.shape[0]),
                          "M": int(want.edges_split.shape[0]), "jacobi_rounds": want.rounds}))
        return 0

    import torch
    from deftet_amd import _lib, hip_ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    tet_d, pts_d, feat_d = (torch.from_numpy(x).to(dev) for x in (tets, pts, feat))
    nbr = hip_ops.tet_face_neighbours(tet_d, P, dev)
    sel_d = hip_ops.occupancy_band(torch.from_numpy(inside).to(dev), nbr, rings=1)
    select = sel_d.cpu().numpy()
    edges_d, tet_edge_d = hip_ops.tet_edges(tet_d, P)
    E = int(edges_d.shape[0])

    variants = (("refine", lambda: hip_ops.refine_tets(tet_d, pts_d, feat_d, sel_d)),
                ("refine_edges", lambda: hip_ops.refine_tets(tet_d, pts_d, feat_d, sel_d, edges=edges_d, tet_edge=tet_edge_d)),
                ("uniform", lambda: hip_ops.subdivide(tet_d, pts_d, feat_d, None)))
    times = {name: [] for name, _ in variants}
    host_ms, want = [], None
    for _ in range(args.host_steps):
        t0 = time.perf_counter()
        want = R.refine(tets, pts, feat, select)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    for step in range(args.warmup + args.steps):
        outs = {}
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
        if not all(torch.equal(a, b) for a, b in zip(outs["refine"], outs["refine_edges"])):
            raise SystemExit("step %d: refine with and without the edges handed in differ" % step)
        if step == 0 and want is not None:
            for got, ref in zip(outs["refine"], want[:6]):
                if got.cpu().numpy().tobytes() != np.ascontiguousarray(ref).tobytes():
                    raise SystemExit("refine differs from the numpy restatement")
    closure = {}
    for S in (1, 4):
        _marks, counts = hip_ops.refine_marks(tet_edge_d, sel_d, E, S)
        closure["sweeps_per_sync=%d" % S] = {"sweeps": len(counts), "read_backs": len(counts) // S, "marks_set_per_sweep": counts}
    kern_ms = {}
    for kname in KERNELS:
        lib.deftet_profile_select(kname.encode())
        for _ in range(10):
            variants[0][1]()
        torch.cuda.synchronize()
        ms, n = ctypes.c_double(), ctypes.c_longlong()
        lib.deftet_profile_read(ctypes.byref(ms), ctypes.byref(n))
        lib.deftet_profile_select(b"")
        kern_ms[kname] = {"ms_per_call": round(ms.value / 10, 5), "launches_per_call": n.value / 10}
    r, u = outs["refine"], outs["uniform"]
    sizes = {"selected": int(select.sum()), "E": E, "T_new": int(r.tet_new.shape[0]), "M": int(r.edges_split.shape[0]),
             "kinds": np.bincount(r.kind.cpu().numpy(), minlength=7).tolist()}
    for name, _ in variants:
        line = dict(variant=name, config=config, **stats(times[name]))
        if name == "uniform":
            line.update(T_new=int(u[2].shape[0]), P_new=int(u[0].shape[0]))
        else:
            line.update(sizes)
        if name == "refine":
            line.update(closure=closure, kernels=kern_ms, vs_uniform=round(float(np.median(times["uniform"]) / np.median(times[name])), 3))
        print(json.dumps(line), flush=True)
    if host_ms:
        print(json.dumps(dict(variant="host", config=config, jacobi_rounds=want.rounds, **stats(host_ms))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
