#!/usr/bin/env python
"""A/B of the point-voxel operators against torch's own path on the same GPU, at the workload's sizes:

  sampler       B = 8, N = 46,656 (decode_pos at res 70) and N = 10,000 (decode_occ in training), the four encoder volumes
                (64 ch at 32^3, 128 at 16^3, 128 at 16^3, 512 at 8^3), pos appended.
                A: hip_ops.voxel_sample.  B: four grid_sample calls, torch.cat, torch.cat with the positions; autograd backward.
  voxelization  B = 8, N = 5,000, R = 32, C in {3, 64, 128}.  A: pointvoxel.avg_voxelize.  B: an index_add_ restatement.

Per case: forward and forward-plus-backward time (HIP events, median of `--repeat` after `--warmup`, the two sides alternated)
with the spread (min / max) of each side, and the peak memory of one forward-plus-backward above the inputs (the result, the
saved tensors and the gradients count; this library's cached workspace counts once it has grown).  A timed call starts from
fresh clones of the inputs, so it includes building the autograd graph, on both sides alike.  One JSON line per case.

    python tools/pointvoxel_ab.py [--repeat 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import hip_ops, pointvoxel  # noqa: E402

VOLUMES = [(64, 32), (128, 16), (128, 16), (512, 8)]


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


def torch_voxelize(feat, coords, R):
    B, C, N = feat.shape
    ind = (coords[:, 0].long() * R + coords[:, 1].long()) * R + coords[:, 2].long()                   # [B,N]
    flat = (ind + torch.arange(B, device=feat.device)[:, None] * R ** 3).reshape(-1)                    # one index_add_ for the batch
    cnt = torch.zeros(B * R ** 3, device=feat.device).index_add_(0, flat, torch.ones(B * N, device=feat.device))
    out = torch.zeros(B * R ** 3, C, device=feat.device).index_add_(0, flat, feat.permute(0, 2, 1).reshape(B * N, C))
    out = out / cnt.clamp(min=1)[:, None]
    return out.view(B, R ** 3, C).permute(0, 2, 1).reshape(B, C, R, R, R)


def timed(fn, sync_grad):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    if sync_grad is not None:
        out.backward(sync_grad)
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def ab(name, make_inputs, fa, fb, gout, repeat, warmup):
    rec = {"case": name}
    for mode in ("fwd", "fwd_bwd"):
        times = {"ours": [], "torch": []}
        for it in range(warmup + repeat):
            for side, fn in (("ours", fa), ("torch", fb)):           # alternated in the same process
                inputs = make_inputs(mode == "fwd_bwd")
                t = timed(lambda: fn(*inputs), gout if mode == "fwd_bwd" else None)
                if it >= warmup:
                    times[side].append(t)
        for side, ts in times.items():
            rec["%s_%s_ms" % (side, mode)] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
    for side, fn in (("ours", fa), ("torch", fb)):
        inputs = make_inputs(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()                        # the inputs are allocated; their gradients are not yet
        fn(*inputs).backward(gout)
        torch.cuda.synchronize()
        rec["%s_peak_mib_above_inputs" % side] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del inputs
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointvoxel_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B = "cuda", a.batch
    g = torch.Generator().manual_seed(0)
    lines = []
    vols0 = [torch.randn(B, c, r, r, r, generator=g).to(dev) for c, r in VOLUMES]
    for N in (46656, 10000):
        pos0 = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)
        gout = torch.randn(B, sum(c for c, _ in VOLUMES) + 3, N, device=dev)

        def make(grad, pos0=pos0):
            return pos0.clone().requires_grad_(grad), [v.clone().requires_grad_(grad) for v in vols0]
        lines.append(ab("sample_f.B%d.N%d" % (B, N), make, lambda p, v: hip_ops.voxel_sample(v, p, append_pos=True), torch_sample, gout,
                        a.repeat, a.warmup))
        print(json.dumps(lines[-1]), flush=True)
        del gout
    N, R = 5000, 32
    coords = torch.randint(0, R, (B, 3, N), generator=g, dtype=torch.int32).to(dev)
    for C in (3, 64, 128):
        feat0 = torch.randn(B, C, N, generator=g).to(dev)
        gout = torch.randn(B, C, R, R, R, device=dev)

        def make(grad, feat0=feat0):
            return (feat0.clone().requires_grad_(grad),)
        lines.append(ab("avg_voxelize.B%d.N%d.C%d.R%d" % (B, N, C, R), make, lambda f: pointvoxel.avg_voxelize(f, coords, R),
                        lambda f: torch_voxelize(f, coords, R), gout, a.repeat, a.warmup))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
