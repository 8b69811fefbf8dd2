#!/usr/bin/env python
"""A/B of the iso-solid measures on the tets on the res-70 grid of deftet_amd.grids (V = 46,656, T = 257,250),
B = 8, forward + backward with the gradient on the field and on the vertex positions, for two fields: `sdf`, the distance to a
sphere of radius 0.3 (few tets are cut), and `noise`, N(0,1) values (seven tets in eight are cut):

  fraction   A  TetTopology.iso_fraction (hip_ops.tet_iso_fraction), frac [B,T]
             B  the torch composition: the four corner values by advanced indexing of the flattened [B V] array, sorted, the
                simplex-spline closed form 1 - sum_i (iso - f_i)_+^3 / prod_{j != i} (f_j - f_i) in fp32; autograd's backward of
                the sort and of the indexing (index_add_, float atomics)
  measures   A  TetTopology.iso_measures (hip_ops.tet_iso_measures) with a per-tet occupancy as weights, [B,5]
             B  the same fraction, the volumes by the edge matrix's determinant, the area by the coarea identity
                area = vol |grad f| sum_i 3 (iso - f_i)_+^2 / prod_{j != i} (f_j - f_i) with the gradient composed as in
                tools/tet_field_grad_ab.py, then the five sums (fp32)

Per step and side: the time (HIP events, median / min / max of `--repeat` after `--warmup`, the sides alternated inside the
process) and the peak memory above the inputs.  A timed step starts from fresh leaves, so building the autograd graph is included
on both sides alike.  Side B divides by differences of corner values in fp32 and is not exact where two of them are close; the
agreement printed with each case is the max-norm difference of the two sides' values.  One JSON line per step.

    python tools/tet_iso_measures_ab.py [--repeat 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import grids  # noqa: E402
from deftet_amd.layers.DefTet.deftet import TetTopology  # noqa: E402

SIDES = ("A", "B")


def corners(x_bxvxc, tets_tx4):
    B, V = x_bxvxc.shape[:2]
    flat = (tets_tx4[None] + torch.arange(B, device=x_bxvxc.device)[:, None, None] * V).reshape(-1)
    return x_bxvxc.reshape(B * V, -1)[flat].view(B, -1, 4, x_bxvxc.shape[-1])


def spline_terms(f_bxtx4, iso, power):
    """sum_i (iso - f_i)_+^power / prod_{j != i} (f_j - f_i) over the sorted corner values"""
    f = torch.sort(f_bxtx4, dim=-1).values
    d = f[..., None, :] - f[..., :, None]                              # [.., i, j] = f_j - f_i
    d = d + torch.eye(4, device=f.device)                              # (the diagonal leaves the product alone)
    return ((iso - f).clamp_min(0) ** power / d.prod(-1)).sum(-1)


def torch_fraction(field, tets_tx4, iso):
    return 1.0 - spline_terms(corners(field[:, :, None], tets_tx4)[..., 0], iso, 3)


def torch_measures(field, pos, tets_tx4, iso, w):
    x, f = corners(pos, tets_tx4), corners(field[:, :, None], tets_tx4)[..., 0]
    e = x[:, :, 1:] - x[:, :, :1]
    cr = lambda a, b: torch.linalg.cross(a, b, dim=-1)
    n = torch.stack([cr(e[:, :, 1], e[:, :, 2]), cr(e[:, :, 2], e[:, :, 0]), cr(e[:, :, 0], e[:, :, 1])], 2)
    det = (e[:, :, 0] * n[:, :, 0]).sum(-1)
    live = det > 0
    safe = torch.where(live, det, torch.ones_like(det))
    g = (n * (f[:, :, 1:] - f[:, :, :1])[..., None]).sum(2) / safe[..., None]
    vol = torch.where(live, det / 6, torch.zeros_like(det))
    frac = 1.0 - spline_terms(f, iso, 3)
    area = vol * g.norm(dim=-1) * 3.0 * spline_terms(f, iso, 2)
    fv = frac * vol
    return torch.stack([fv.sum(1), area.sum(1), (w * fv).sum(1), (w * vol).sum(1), vol.sum(1)], -1)


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tet_iso_measures_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B, iso = "cuda", a.batch, 0.0
    verts, tets = grids.kuhn_grid(a.res)
    pos0 = torch.from_numpy(grids.jittered_positions(verts, a.res, B)).float().to(dev)
    tets_tx4 = torch.from_numpy(tets).long().to(dev)
    V, T = pos0.shape[1], tets_tx4.shape[0]
    topo = TetTopology(tets_tx4[None].expand(B, -1, -1).contiguous(), V)
    g = torch.Generator().manual_seed(0)
    tag = "res%d.B%d.V%d.T%d" % (a.res, B, V, T)
    w = (torch.rand(B, T, generator=g) < 0.5).float().to(dev)
    gfrac, gm = torch.randn(B, T, generator=g).to(dev), torch.rand(B, 5, generator=g).to(dev)
    lines = []
    for kind, field0 in (("sdf", 0.3 - pos0.norm(dim=-1)), ("noise", torch.randn(B, V, generator=g).to(dev))):
        with torch.no_grad():                                       # the two sides compute the same thing, as far as fp32 lets side B
            fa, fb = topo.iso_fraction(field0, pos0, iso=iso), torch_fraction(field0, tets_tx4, iso)
            ma, mb = topo.iso_measures(field0, pos0, iso=iso, weights=w), torch_measures(field0, pos0, tets_tx4, iso, w)
            agree_f = float((fa - fb).abs().max())
            agree_m = float(((ma - mb).abs() / mb.abs().clamp_min(1e-30)).max())

        def leaves():
            return field0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)

        def fraction_step(side):
            field, pos = leaves()
            frac = topo.iso_fraction(field, pos, iso=iso) if side == "A" else torch_fraction(field, tets_tx4, iso)
            frac.backward(gfrac)

        def measures_step(side):
            field, pos = leaves()
            m = topo.iso_measures(field, pos, iso=iso, weights=w) if side == "A" else torch_measures(field, pos, tets_tx4, iso, w)
            m.backward(gm)

        for name, step, agree in (("fraction", fraction_step, agree_f), ("measures", measures_step, agree_m)):
            rec = measure("%s.%s.%s" % (name, kind, tag), step, a.repeat, a.warmup)
            rec["values_A_vs_B"] = agree
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
