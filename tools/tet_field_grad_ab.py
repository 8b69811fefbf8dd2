#!/usr/bin/env python
"""A/B of the field gradients on the tets on the res-70 grid of deftet_amd.grids (V = 46,656, T = 257,250), B = 8,
C = 1 (an SDF or occupancy) and C = 4, forward + backward with the gradient on the field and on the vertex positions:

  gradient   A  TetTopology.field_gradient (hip_ops.tet_field_gradient) with the volumes, [B,T,C,3] and [B,T]
             B  the torch composition: the positions and field rows of the four corners by advanced indexing of the flattened
                [B V, .] arrays (no tet_gather), the edge matrix, its adjugate by three cross products, det, g = adj df / det,
                the live mask by torch.where; autograd's backward of the indexing is index_add_ (float atomics)
  energies   A  TetTopology.field_energies, [B,C,2]
             B  the same composition followed by the two volume-weighted means (fp32 sums)
  iso        A  DefTet.iso_surface: per-tet occupancy to the vertices (hip_ops.tet_to_vertex, volume weights), marching_tets
             B  the vertex field as two index_add_ over the 4 T incidences (sum of w occ, sum of w) and a division, then the same
                marching_tets; C does not enter (run once)

Per step and side: the time (HIP events, median / min / max of `--repeat` after `--warmup`, the sides alternated inside the
process), the device launches as the profiler counts them, and the peak memory above the inputs.  A timed step starts from
fresh leaves, so building the autograd graph is included on both sides alike.  One JSON line per step.

    python tools/tet_field_grad_ab.py [--repeat 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import grids, hip_ops  # noqa: E402
from deftet_amd.layers.DefTet.deftet import DefTet, TetTopology  # noqa: E402

SIDES = ("A", "B")


def torch_gradient(field, pos, tets_tx4):
    """(g [B,T,C,3], vol [B,T]) composed in torch"""
    B, V, C = field.shape
    flat = (tets_tx4[None] + torch.arange(B, device=pos.device)[:, None, None] * V).reshape(-1)
    x = pos.reshape(B * V, 3)[flat].view(B, -1, 4, 3)
    f = field.reshape(B * V, C)[flat].view(B, -1, 4, C)
    e = x[:, :, 1:] - x[:, :, :1]
    cr = lambda a, b: torch.linalg.cross(a, b, dim=-1)
    n = torch.stack([cr(e[:, :, 1], e[:, :, 2]), cr(e[:, :, 2], e[:, :, 0]), cr(e[:, :, 0], e[:, :, 1])], 2)
    det = (e[:, :, 0] * n[:, :, 0]).sum(-1)
    live = det > 0
    safe = torch.where(live, det, torch.ones_like(det))
    df = f[:, :, 1:] - f[:, :, :1]
    g = (n[:, :, :, None, :] * df[:, :, :, :, None]).sum(2) / safe[:, :, None, None]
    return torch.where(live[:, :, None, None], g, torch.zeros_like(g)), torch.where(live, det / 6, torch.zeros_like(det))


def torch_energies(field, pos, tets_tx4, target):
    g, vol = torch_gradient(field, pos, tets_tx4)
    s2 = (g * g).sum(-1)
    s = torch.sqrt(s2)
    w = vol[:, :, None]
    return torch.stack([(w * s2).sum(1), (w * (s - target) ** 2).sum(1)], -1) / w.sum(1)[:, :, None]


def torch_volumes(pos, tets_tx4):
    B, V = pos.shape[:2]
    flat = (tets_tx4[None] + torch.arange(B, device=pos.device)[:, None, None] * V).reshape(-1)
    x = pos.reshape(B * V, 3)[flat].view(B, -1, 4, 3)
    e = x[:, :, 1:] - x[:, :, :1]
    return ((e[:, :, 0] * torch.linalg.cross(e[:, :, 1], e[:, :, 2], dim=-1)).sum(-1) / 6).clamp_min(0)


def torch_to_vertices(occ_bxt, vol, tets_tx4, V):
    B, T = occ_bxt.shape
    flat = (tets_tx4[None] + torch.arange(B, device=occ_bxt.device)[:, None, None] * V).reshape(-1)
    num = torch.zeros(B * V, device=occ_bxt.device).index_add_(0, flat, (vol * occ_bxt)[:, :, None].expand(-1, -1, 4).reshape(-1))
    den = torch.zeros(B * V, device=occ_bxt.device).index_add_(0, flat, vol[:, :, None].expand(-1, -1, 4).reshape(-1))
    return (num / den.clamp_min(1e-30)).view(B, V)


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
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tet_field_grad_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B, target = "cuda", a.batch, 1.0
    verts, tets = grids.kuhn_grid(a.res)
    pos0 = torch.from_numpy(grids.jittered_positions(verts, a.res, B)).float().to(dev)
    tets_tx4 = torch.from_numpy(tets).long().to(dev)
    V, T = pos0.shape[1], tets_tx4.shape[0]
    tets_b = tets_tx4[None].expand(B, -1, -1).contiguous()
    topo = TetTopology(tets_b, V)
    layer = DefTet()
    g = torch.Generator().manual_seed(0)
    tag = "res%d.B%d.V%d.T%d" % (a.res, B, V, T)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for C in a.channels:
        field0 = torch.randn(B, V, C, generator=g).to(dev)
        gout, gvol, ge = torch.randn(B, T, C, 3, generator=g).to(dev), torch.randn(B, T, generator=g).to(dev), torch.rand(B, C, 2, generator=g).to(dev)
        with torch.no_grad():                                       # the two sides compute the same thing
            ga, va = topo.field_gradient(field0, pos0, return_volume=True)
            gb, vb = torch_gradient(field0, pos0, tets_tx4)
            agree_g = float((ga - gb).abs().max() / gb.abs().max())
            ea, eb = topo.field_energies(field0, pos0, target=target), torch_energies(field0, pos0, tets_tx4, target)
            agree_e = float((ea - eb).abs().max() / eb.abs().max())

        def leaves():
            return field0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)

        def gradient_step(side):
            field, pos = leaves()
            gg, vol = topo.field_gradient(field, pos, return_volume=True) if side == "A" else torch_gradient(field, pos, tets_tx4)
            torch.autograd.backward([gg, vol], [gout, gvol])

        def energies_step(side):
            field, pos = leaves()
            e = topo.field_energies(field, pos, target=target) if side == "A" else torch_energies(field, pos, tets_tx4, target)
            e.backward(ge)

        rec = measure("gradient.C%d.%s" % (C, tag), gradient_step, a.repeat, a.warmup)
        rec["values_max_norm_A_vs_B"] = agree_g
        emit(rec)
        rec = measure("energies.C%d.%s" % (C, tag), energies_step, a.repeat, a.warmup)
        rec["values_max_norm_A_vs_B"] = agree_e
        emit(rec)

    cent = pos0.reshape(B * V, 3)[(tets_tx4[None] + torch.arange(B, device=dev)[:, None, None] * V).reshape(-1)].view(B, T, 4, 3).mean(2)
    occ0 = torch.sigmoid((0.3 - cent.norm(dim=-1)) * 20)
    edges = topo.edges()

    def iso_step(side):
        occ, pos = occ0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)
        if side == "A":
            mesh = layer.iso_surface(pos, tets_b, occ, iso=0.5)
        else:
            vol = torch_volumes(pos0, tets_tx4)                                           # (constant weights, as on side A)
            mesh = hip_ops.marching_tets(pos, torch_to_vertices(occ, vol, tets_tx4, V), edges, iso=0.5)
        sum(v.sum() for v in mesh.verts).backward()

    emit(measure("iso_surface.%s" % tag, iso_step, a.repeat, a.warmup))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
