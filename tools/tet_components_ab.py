#!/usr/bin/env python
"""A/B of the occupancy clean-up at res 70, B = 8 (Kuhn grid; the shapes alternate between a sphere of radius 0.3 with three
floaters of radius 0.05 in corners and a shell with radii 0.2 and 0.35), keep_largest=True, fill_voids=True:

  (a) hip      hip_ops.occupancy_cleanup: two labellings (the complement, then the filled mask) and the selection, one device
               sequence, four bytes read back (the bad-neighbour count)
  (b) torch    what a user writes without the operator, on the same GPU: min-label propagation — gather the neighbours' labels
               through the table, amin, iterate to a fixed point (tested every 8 rounds) — then sizes by scatter_add, the open
               flag by scatter amax, the same four selection steps
  (c) host     the route the reference's comments point at: read the mask back, scipy connected_components per shape, the
               selection in numpy, upload

The variants alternate inside one process; every call ends in a synchronise and is timed with the host clock; every timed step
checks that the three masks are equal.  One JSON line per variant: median ms with min and max, the propagation rounds (b) needed,
per-kernel times of (a) from deftet_profile_select, and the bytes (a) moves at least, computed from the shapes.

    python tools/tet_components_ab.py [--steps 20] [--warmup 3] [--res 70 --batch 8]
    python tools/tet_components_ab.py --check      # a tiny size; argument parsing and input generation up to the first GPU call
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

CORNER = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]])
KERNELS = ("k_tc_init", "k_tc_hook", "k_tc_flatten", "k_tc_fill", "k_tc_best", "k_tc_keep")


def neighbour_table(tets):
    tets = np.asarray(tets, np.int64)
    T, V = tets.shape[0], int(tets.max()) + 1
    f = np.sort(tets[:, CORNER], axis=2).reshape(-1, 3)
    key = (f[:, 0] * V + f[:, 1]) * V + f[:, 2]
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    a, b = order[:-1][same], order[1:][same]
    nbr = -np.ones(4 * T, np.int64)
    nbr[a], nbr[b] = b // 4, a // 4
    return nbr.reshape(T, 4)


def make_inputs(res, batch):
    verts, tets = grids.kuhn_grid(res)
    cen = verts[tets.astype(np.int64)].mean(1) - 0.5
    r = np.linalg.norm(cen, axis=1)
    sphere = r < 0.3
    for c in ((0.4, 0.4, 0.4), (-0.4, 0.4, -0.4), (0.4, -0.4, -0.4)):
        sphere |= np.linalg.norm(cen - np.asarray(c), axis=1) < 0.05
    shell = (r > 0.2) & (r < 0.35)
    return tets, neighbour_table(tets), np.stack([sphere if b % 2 == 0 else shell for b in range(batch)])


def host_components(inside, nbr):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    T = inside.shape[0]
    valid = nbr >= 0
    link = valid & inside[:, None] & inside[np.where(valid, nbr, 0)]
    rows = np.repeat(np.arange(T), 4).reshape(T, 4)
    n, comp = connected_components(coo_matrix((np.ones(int(link.sum()), np.int8), (rows[link], nbr[link])), shape=(T, T)), directed=False)
    sizes = np.bincount(comp[inside], minlength=n)
    opn = np.zeros(n, bool)
    opn[comp[inside & (nbr == -1).any(1)]] = True
    first = np.full(n, T, np.int64)
    np.minimum.at(first, comp, np.arange(T))
    return comp, sizes, opn, first


def host_cleanup(inside, nbr):
    """keep_largest + fill_voids of one shape"""
    comp, _sizes, opn, _first = host_components(~inside, nbr)
    filled = inside | (~inside & ~opn[comp])
    comp, sizes, _opn, first = host_components(filled, nbr)
    if not filled.any():
        return filled
    best = max(np.nonzero(sizes)[0], key=lambda c: (sizes[c], -first[c]))
    return filled & (comp == best)


def torch_cleanup(inside, table):
    """(keep, propagation rounds of both labellings): keep_largest + fill_voids of inside bool [B,T] over table int64 [T,4]"""
    import torch
    B, T = inside.shape
    dev = inside.device
    valid, nb = (table >= 0)[None], table.clamp(min=0)
    boundary = (table == -1).any(1)[None]
    idx = torch.arange(T, device=dev)[None].expand(B, T)
    big = torch.full_like(idx, T)
    rounds = 0

    def labels(mask):
        nonlocal rounds
        lab = torch.where(mask, idx, big)
        while True:
            for _ in range(8):
                near = torch.where(valid, lab[:, nb], big[:, :, None]).amin(2)
                prev, lab = lab, torch.where(mask, torch.minimum(lab, near), big)
                rounds += 1
            if torch.equal(prev, lab):
                return lab

    def stats(mask, lab):
        at = lab.clamp(max=T - 1)
        sizes = torch.zeros(B, T, dtype=torch.int64, device=dev).scatter_add_(1, at, mask.long())
        opn = torch.zeros(B, T, dtype=torch.int64, device=dev).scatter_reduce_(1, at, (mask & boundary).long(), "amax")
        return at, sizes, opn

    out = ~inside
    at, _sizes, opn = stats(out, labels(out))
    filled = inside | (out & (opn.gather(1, at) == 0))
    lab = labels(filled)
    at, sizes, _opn = stats(filled, lab)
    best = (sizes * (T + 1) + (T - idx)).argmax(1, keepdim=True)          # the most tets; the smaller label among equals
    return filled & (lab == best), rounds


def moved_bytes(B, T):
    """what (a) reads and writes at least, per element of [B,T]: the mask 1, a table row 16, parent / accumulator / label words 4"""
    label = B * T * ((1 + 16 + 4 + 4) + (1 + 16 + 4) + (1 + 16 + 4 + 4))          # init, hook, flatten (atomics and neighbours' bytes not counted)
    return dict(label_pass=label, fill=B * T * (1 + 4 + 1), best=B * T * 4, keep=B * T * (4 + 1), total=2 * label + B * T * 15)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="tiny size, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.batch = 8, 2
    tets, nbr, masks = make_inputs(args.res, args.batch)
    B, T = masks.shape
    if args.check:
        keep = np.stack([host_cleanup(m, nbr) for m in masks])
        print(json.dumps({"check": "ok", "B": B, "T": T, "inside": masks.sum(1).tolist(), "kept": keep.sum(1).tolist(), "bytes": moved_bytes(B, T)}))
        return 0

    import torch
    from deftet_amd import _lib, hip_ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    t64 = torch.from_numpy(nbr).to(dev)
    dn = hip_ops.TetFaceNeighbours(t64, t64.to(torch.int32))
    m_d = torch.from_numpy(masks).to(dev)
    rounds = [0]

    def torch_route():
        keep, rounds[0] = torch_cleanup(m_d, t64)
        return keep

    def hip_route():
        return hip_ops.occupancy_cleanup(m_d, dn, keep_largest=True, fill_voids=True)

    def host_route():
        m = m_d.cpu().numpy()
        return torch.from_numpy(np.stack([host_cleanup(x, nbr) for x in m])).to(dev)

    variants = (("hip", hip_route), ("torch", torch_route), ("host", host_route))
    times = {name: [] for name, _ in variants}
    for step in range(args.warmup + args.steps):
        outs = {}
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
        if not (torch.equal(outs["hip"], outs["torch"]) and torch.equal(outs["hip"], outs["host"])):
            raise SystemExit("step %d: the three routes differ" % step)
    kern_ms = {}
    for kname in KERNELS:
        lib.deftet_profile_select(kname.encode())
        for _ in range(10):
            hip_route()
        torch.cuda.synchronize()
        ms, n = ctypes.c_double(), ctypes.c_longlong()
        lib.deftet_profile_read(ctypes.byref(ms), ctypes.byref(n))
        lib.deftet_profile_select(b"")
        kern_ms[kname] = {"ms_per_call": round(ms.value / 10, 5), "launches_per_call": n.value // 10}
    kept = outs["hip"].sum(1).tolist()
    for name, _ in variants:
        t = np.asarray(times[name])
        line = {"variant": name, "config": "res=%d B=%d T=%d" % (args.res, B, T), "options": "keep_largest fill_voids", "steps": len(t),
                "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}
        if name == "hip":
            line.update(kept=kept, kernels=kern_ms, bytes=moved_bytes(B, T), speedup_vs_torch=round(float(np.median(times["torch"]) / np.median(t)), 2),
                        speedup_vs_host=round(float(np.median(times["host"]) / np.median(t)), 2))
        if name == "torch":
            line.update(propagation_rounds_both_labellings=rounds[0])
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
