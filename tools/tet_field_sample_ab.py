#!/usr/bin/env python
"""A/B of a per-vertex field read at query points on the res-70 grid of deftet_amd.grids (V = 46,656,
T = 257,250), B = 8, Q = 100,000 queries of grids.random_queries per shape, C = 1 (an SDF or occupancy) and C = 4 (RGBA features):

  A  TetTopology.field_sample (hip_ops.tet_field_sample): the indexed query, one forward launch, the gradient on the field as a
     gather over the incidence CSR, the gradient on the positions through grad_w and the existing backward to the vertices
  B  the torch composition after the same query: point_in_tet_occ_indexed, the tet list indexed with cond, the [B,Q,4,C] field rows
     gathered with index_select, multiplied by the weights and summed over the corners (--einsum: torch.einsum instead, which
     runs as B Q tiny batched matrix products and is the slower way to write it); its backward scatters 4 Q C floats per shape into the field with float
     atomics (index_add_) and hands grad_w to the same backward to the vertices.  A miss (cond = -1, weights 0) is sent to tet
     q % T; with --clamp-misses to tet 0, the way paste_occ clamps: then every miss of a shape adds its zeros to the same four
     field rows and the atomics queue up on them

Per C two steps, forward + backward: `field` (the gradient on the field alone: labels at points supervising the field) and
`field+pos` (also the gradient on the vertex positions).  Per step and side: the time (HIP events, median / min / max of `--repeat`
after `--warmup`, the sides alternated inside the process), the device launches as the profiler counts them, and the peak memory
above the inputs (torch.cuda.max_memory_allocated; this library's cached workspace counts once it has grown).  A timed step starts
from fresh leaves, so building the autograd graph is included on both sides alike.  One JSON line per step.

    python tools/tet_field_sample_ab.py [--repeat 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import grids  # noqa: E402
from deftet_amd.layers.DefTet.check_condition_tetrahedron_base.utils import point_in_tet_occ_indexed  # noqa: E402
from deftet_amd.layers.DefTet.deftet import TetTopology  # noqa: E402

SIDES = ("A", "B")


def sample(side, topo, tets_tx4, pred0, field, pos, pts, clamp_misses=False, use_einsum=False):
    if side == "A":
        return topo.field_sample(field, pos, pts)
    cond, w, _occ = point_in_tet_occ_indexed(pos, pts, pred0, topo)
    B, V, C = field.shape
    t = cond[..., 0].long()
    if clamp_misses:
        t = t.clamp(min=0)                                                                # a miss reads tet 0, as paste_occ has it
    else:
        t = torch.where(t >= 0, t, torch.arange(t.shape[1], device=t.device)[None] % tets_tx4.shape[0])    # ... tet q % T; zero weights
    vi = tets_tx4[t]                                                                      # [B,Q,4]
    flat = (vi + torch.arange(B, device=field.device)[:, None, None] * V).reshape(-1)
    rows = field.reshape(B * V, C).index_select(0, flat).view(B, -1, 4, C)                # (its backward is index_add_)
    if use_einsum:
        return torch.einsum("bqk,bqkc->bqc", w, rows)                                     # (lowered to B Q batched 1x4 by 4xC products)
    return (w[..., None] * rows).sum(2)


def measure(name, step, repeat, warmup):
    rec = {"case": name}
    times = {s: [] for s in SIDES}
    for it in range(warmup + repeat):
        for side in SIDES:                                          # alternated in the same process
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            step(side)
            e.record()
            e.synchronize()
            if it >= warmup:
                times[side].append(s.elapsed_time(e))
    for side in SIDES:
        ts = times[side]
        rec[side] = {"ms": {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(side)
        torch.cuda.synchronize()
        rec[side]["peak_mib_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(side)
                torch.cuda.synchronize()
            ev = [x for x in prof.events() if str(x.device_type).endswith("CUDA")]
            rec[side]["kernels"] = sum(1 for x in ev if "memcpy" not in x.name.lower() and "memset" not in x.name.lower())
            rec[side]["copies_and_memsets"] = sum(1 for x in ev if "memcpy" in x.name.lower() or "memset" in x.name.lower())
        except Exception as exc:                                    # the profiler is not what is measured here
            rec[side]["kernels"] = "not measured (%s)" % type(exc).__name__
    rec["A_over_B"] = round(rec["A"]["ms"]["median"] / rec["B"]["ms"]["median"], 4)
    rec["B_spread_ms"] = round(rec["B"]["ms"]["max"] - rec["B"]["ms"]["min"], 4)
    rec["A_minus_B_ms"] = round(rec["A"]["ms"]["median"] - rec["B"]["ms"]["median"], 4)
    rec["peak_B_minus_A_mib"] = round(rec["B"]["peak_mib_above_inputs"] - rec["A"]["peak_mib_above_inputs"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--clamp-misses", action="store_true")
    ap.add_argument("--einsum", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tet_field_sample_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B, Q = "cuda", a.batch, a.queries
    verts, tets = grids.kuhn_grid(a.res)
    pos0 = torch.from_numpy(grids.jittered_positions(verts, a.res, B)).float().to(dev)
    pts0 = torch.from_numpy(grids.random_queries(B, Q)).to(dev)
    tets_tx4 = torch.from_numpy(tets).long().to(dev)
    V, T = pos0.shape[1], tets_tx4.shape[0]
    topo = TetTopology(tets_tx4[None].expand(B, -1, -1).contiguous(), V)
    pred0 = torch.zeros(B, T, device=dev)
    g = torch.Generator().manual_seed(0)
    tag = "res%d.B%d.V%d.T%d.Q%d" % (a.res, B, V, T, Q)
    lines = []
    for C in a.channels:
        field0 = torch.randn(B, V, C, generator=g).to(dev)
        gout = torch.randn(B, Q, C, generator=g).to(dev)
        with torch.no_grad():                                       # the two sides compute the same thing
            va, vb = (sample(s, topo, tets_tx4, pred0, field0, pos0, pts0, a.clamp_misses, a.einsum) for s in SIDES)
            agree = float((va - vb).abs().max() / vb.abs().max())

        def step(side, with_pos):
            field, pos = field0.clone().requires_grad_(True), pos0.clone().requires_grad_(with_pos)
            sample(side, topo, tets_tx4, pred0, field, pos, pts0, a.clamp_misses, a.einsum).backward(gout)

        for what, with_pos in (("field", False), ("field+pos", True)):
            rec = measure("C%d.grad_%s.%s" % (C, what, tag), lambda side: step(side, with_pos), a.repeat, a.warmup)
            rec["values_max_norm_A_vs_B"], rec["B_clamps_misses"], rec["B_einsum"] = agree, bool(a.clamp_misses), bool(a.einsum)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
