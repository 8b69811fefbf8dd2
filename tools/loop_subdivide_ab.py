#!/usr/bin/env python
"""A/B of one level of Loop subdivision, forward + backward, on the same GPU:

  A  hip_ops.loop_subdivide on a LoopTopology (one launch forward, one launch backward, no atomics)
  B  the torch composition: forward torch.sparse.mm with the assembled matrix S [(V+E) x V] on the positions laid out as
     [V, B*3] (and the attributes as [V, B*C]), backward index_add_ of the weighted output-gradient rows onto the input rows
     (float atomics); the transposes between [B,V,.] and [V,B*.] are part of the step

Scene: the marching-tetrahedra surface of the sphere of radius 0.3 on the res-70 grid of deftet_amd.grids, one topology, B = 8
perturbed copies of its vertices.  Run once for positions only and once for positions + 3 colours.  Topology and matrix are
built before the timed steps on both sides (they are per face list, not per step).

Per step and side: the time (HIP events, median / min / max of `--repeat` after `--warmup`, the sides alternated inside the
process), the device launches as the profiler counts them, the peak memory above the inputs and, for side A, the mean time of
its two kernels from the library's own events (deftet_profile_select).  A timed step starts from fresh leaves.  The two sides are compared before they are timed.  One JSON line per run.

    python tools/loop_subdivide_ab.py [--repeat 20] [--warmup 5] [--res 70 --batch 8] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import _lib, grids, hip_ops  # noqa: E402

SIDES = ("A", "B")


def assemble(top):
    """(rows, cols, vals) of S from the tables of a LoopTopology, in torch on its device"""
    V, E, dev = top.n_vertex, top.n_edge, top.device
    kind = top.vertex_kind.long()
    n = (top.ev_offsets[1:] - top.ev_offsets[:-1]).float()
    beta = torch.where(n == 3, torch.full_like(n, 3.0 / 16.0), 3.0 / (8.0 * n.clamp_min(1)))
    v = torch.arange(V, device=dev)
    own = torch.where(kind == 0, 1.0 - n * beta, torch.where(kind == 1, torch.full_like(n, 0.75), torch.ones_like(n)))
    rows, cols, vals = [v], [v], [own]
    a, b = top.edges[:, 0].long(), top.edges[:, 1].long()
    for p, q in ((a, b), (b, a)):                                   # the smooth vertex p reads its neighbour q
        m = kind[p] == 0
        rows.append(p[m]); cols.append(q[m]); vals.append(beta[p[m]])
    cv = v[kind == 1]
    for k in (0, 1):
        rows.append(cv); cols.append(top.crease_nbr[cv, k].long()); vals.append(torch.full((cv.numel(),), 0.125, device=dev))
    e = torch.arange(E, device=dev)
    inner = top.edge_nface == 2
    w = torch.where(inner, torch.full((E,), 0.375, device=dev), torch.full((E,), 0.5, device=dev))
    for q in (a, b):
        rows.append(V + e); cols.append(q); vals.append(w)
    for k in (0, 1):
        rows.append(V + e[inner]); cols.append(top.edge_opp[inner, k].long()); vals.append(torch.full((int(inner.sum()),), 0.125, device=dev))
    return torch.cat(rows), torch.cat(cols), torch.cat(vals)


class TorchLoop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, S, rows, cols, vals):
        B, V, C = x.shape
        ctx.save_for_backward(rows, cols, vals)
        ctx.shape = (B, V, C)
        y = torch.sparse.mm(S, x.permute(1, 0, 2).reshape(V, B * C))
        return y.view(-1, B, C).permute(1, 0, 2).contiguous()

    @staticmethod
    def backward(ctx, g):
        rows, cols, vals = ctx.saved_tensors
        B, V, C = ctx.shape
        gr = g.permute(1, 0, 2).reshape(-1, B * C)
        gx = torch.zeros(V, B * C, device=g.device, dtype=g.dtype).index_add_(0, cols, vals[:, None] * gr[rows])
        return gx.view(V, B, C).permute(1, 0, 2).contiguous(), None, None, None, None


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
    rec["A"]["kernel_us"] = kernel_times(step, repeat)
    return rec


def kernel_times(step, repeat):
    """mean time of side A's two kernels in microseconds, from the library's own HIP events around each launch (a run of its
    own after the timed steps: the events slow the step)"""
    lib, out = _lib.load(), {}
    for k in ("k_loop_fwd", "k_loop_bwd"):
        lib.deftet_profile_select(k.encode())
        for _ in range(repeat):
            step("A")
        torch.cuda.synchronize()
        tot, cnt = ctypes.c_double(0), ctypes.c_longlong(0)
        lib.deftet_profile_read(ctypes.byref(tot), ctypes.byref(cnt))
        lib.deftet_profile_select(b"")
        if cnt.value:
            out[k] = round(tot.value / cnt.value * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loop_subdivide_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B = "cuda", a.batch
    verts, tets = grids.kuhn_grid(a.res)
    pos = torch.from_numpy(verts).float().to(dev)
    field = 0.3 - (pos - 0.5).norm(dim=1)                           # the grid spans [0,1]^3
    mesh = hip_ops.marching_tets(pos, field[None], hip_ops.TetEdges(torch.from_numpy(tets).long().to(dev), pos.shape[0]))
    v0, faces = mesh.verts[0], mesh.faces[0]
    top = hip_ops.LoopTopology(faces, v0.shape[0])
    V, E, F = top.n_vertex, top.n_edge, top.n_face
    rows, cols, vals = assemble(top)
    S = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (V + E, V)).coalesce().to_sparse_csr()
    g = torch.Generator().manual_seed(0)
    x0 = (v0[None] + 0.002 * torch.randn(B, V, 3, generator=g).to(dev)).contiguous()
    lines = []
    for C in (0, 3):
        a0 = torch.rand(B, V, C, generator=g).to(dev) if C else None
        gv, ga = torch.randn(B, V + E, 3, generator=g).to(dev), torch.randn(B, V + E, C, generator=g).to(dev) if C else None

        def step(side, keep=None):
            x = x0.clone().requires_grad_(True)
            at = a0.clone().requires_grad_(True) if C else None
            if side == "A":
                ov, oa = hip_ops.loop_subdivide(x, top, at)
            else:
                ov = TorchLoop.apply(x, S, rows, cols, vals)
                oa = TorchLoop.apply(at, S, rows, cols, vals) if C else None
            grads = torch.autograd.grad([ov] + ([oa] if C else []), [x] + ([at] if C else []), [gv] + ([ga] if C else []))
            if keep is not None:
                keep[side] = (ov, oa) + tuple(grads)

        kept = {}
        step("A", kept)
        step("B", kept)
        agree = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(kept["A"], kept["B"]) if p is not None)
        if agree > 1e-5:
            raise SystemExit("loop_subdivide_ab: the two sides differ by %.3g of the largest entry" % agree)
        rec = measure("loop_subdivide.fwd+bwd.res%d.B%d.V%d.E%d.F%d.C%d" % (a.res, B, V, E, F, C), step, a.repeat, a.warmup)
        rec["sides_agree_maxnorm"] = agree
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
