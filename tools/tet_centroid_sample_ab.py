#!/usr/bin/env python
"""A/B/C of the occupancy decoder's input on the res-70 grid of deftet_amd.grids (V = 46,656, T = 257,250), B = 8,
the four encoder volumes (64 ch at 32^3, 128 at 16^3, 128 at 16^3, 512 at 8^3):

  training   K = 10,000 tets of a randperm, forward + backward to the vertices and the volumes (decode_occ, pc_model.py:269-314)
  inference  all T tets in ranges of 12,500 under no_grad (split_decode_occ, pc_model.py:332-366: 21 calls)

  A  TetTopology.centroid_sample (hip_ops.tet_centroid_sample): nothing of size [B,T,4,3]
  B  the best route from the operators that existed before it: TetTopology.gather -> mean -> index -> hip_ops.voxel_sample
     (in the inference case one gather and mean for the whole walk, then a slice per range)
  C  the reference's torch composition: torch.gather, mean, gather of center_idx, four grid_sample, two torch.cat

Per case and side: the time of one step (HIP events, median / min / max of `--repeat` after `--warmup`, the three sides alternated
inside the process), the device launches of one step as the profiler counts them, and the peak memory of one step above the
inputs (torch.cuda.max_memory_allocated; this library's cached workspace counts once it has grown).  A timed training step starts
from fresh leaves, so building the autograd graph is included on every side alike.  One JSON line per case.

    python tools/tet_centroid_sample_ab.py [--repeat 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import grids, hip_ops  # noqa: E402
from deftet_amd.layers.DefTet.deftet import TetTopology  # noqa: E402

VOLUMES = [(64, 32), (128, 16), (128, 16), (512, 8)]
SIDES = ("A", "B", "C")


def torch_sample(pos, vols):
    p = (pos + 0.5).permute(0, 2, 1)
    outs = []
    for c in vols:
        r = c.shape[-1]
        u = torch.clamp(p * r, 0, r - 1)
        g = (u * 2 + 1.0) / r - 1.0
        g = torch.flip(g.permute(0, 2, 1).reshape(c.shape[0], 1, 1, -1, 3), dims=[-1])
        outs.append(torch.nn.functional.grid_sample(c, g, padding_mode="border", align_corners=False).squeeze(2).squeeze(2))
    return torch.cat([torch.cat(outs, dim=1), pos.permute(0, 2, 1)], 1)


def features(side, topo, tet_bxfx4, pos, vols, select=None, first=0, count=None, center=None):
    if side == "A":
        return topo.centroid_sample(vols, pos, select=select, first=first, count=count)
    if side == "B":
        center = topo.gather(pos).mean(dim=2) if center is None else center
        center = center[:, select] if select is not None else center[:, first:first + count]
        return hip_ops.voxel_sample(vols, center, append_pos=True)
    n_batch = pos.shape[0]
    tets = tet_bxfx4 if select is not None else tet_bxfx4[:, first:first + count]     # split_decode_occ slices the list per range
    gather_input = pos.unsqueeze(2).expand(n_batch, pos.shape[1], 4, 3)
    gather_index = tets.unsqueeze(-1).expand(n_batch, tets.shape[1], 4, 3)
    center = torch.mean(torch.gather(input=gather_input, dim=1, index=gather_index), dim=2)
    if select is not None:
        center = torch.gather(input=center, dim=1, index=select.unsqueeze(0).unsqueeze(-1).expand(n_batch, select.shape[0], 3))
    return torch_sample(center, vols)


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
    ap.add_argument("--select", type=int, default=10000)
    ap.add_argument("--split", type=int, default=12500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tet_centroid_sample_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B = "cuda", a.batch
    verts, tets = grids.kuhn_grid(a.res)
    pos0 = torch.from_numpy(grids.jittered_positions(verts, a.res, B)).float().to(dev)
    tet_bxfx4 = torch.from_numpy(tets).long().to(dev)[None].expand(B, -1, -1).contiguous()
    V, T = pos0.shape[1], tet_bxfx4.shape[1]
    topo = TetTopology(tet_bxfx4, V)
    g = torch.Generator().manual_seed(0)
    vols0 = [torch.randn(B, c, r, r, r, generator=g).to(dev) for c, r in VOLUMES]
    K = min(a.select, T)
    select = torch.randperm(T, generator=g)[:K].to(dev)
    gout = torch.randn(B, sum(c for c, _ in VOLUMES) + 3, K, device=dev)
    tag = "res%d.B%d.V%d.T%d" % (a.res, B, V, T)

    def train_step(side):
        pos, vols = pos0.clone().requires_grad_(True), [v.clone().requires_grad_(True) for v in vols0]
        features(side, topo, tet_bxfx4, pos, vols, select=select).backward(gout)

    def infer_step(side):
        with torch.no_grad():
            center = topo.gather(pos0).mean(dim=2) if side == "B" else None    # B at its best: one gather for the whole walk
            for first in range(0, T, a.split):
                features(side, topo, tet_bxfx4, pos0, vols0, first=first, count=min(a.split, T - first), center=center)

    lines = []
    for name, step in (("training.K%d.%s" % (K, tag), train_step), ("inference.split%d.%s" % (a.split, tag), infer_step)):
        lines.append(measure(name, step, a.repeat, a.warmup))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
