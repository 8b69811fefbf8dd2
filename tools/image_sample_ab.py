#!/usr/bin/env python
"""A/B of the pixel-aligned image-feature operator against torch's own path on the same GPU, at the DISN shape:

  B = 8, the five VGG-16 maps (64, 128, 256, 512, 512 channels) at 64 x 64, G = 1000 global features, the positions appended;
  N = 46,656 (every vertex of the res-70 grid: decode_pos) and N = 10,000 (a random subset: decode_occ in training).  The uv are
  the grid's vertices under the camera of grids.project_faces (the render configuration: grid scaled by 2.5, radius 4).
  A: imagefeat.sample_f (hip_ops.image_sample).  B: five F.grid_sample calls, expand of the global features, two torch.cat;
  autograd backward.  Both sides project with imagefeat.project_to_image.  Each N also without the global rows.

Per case: forward and forward-plus-backward time (HIP events, median of `--repeat` after `--warmup`, the two sides alternated)
with the spread (min / max) of each side, and the peak memory of one forward-plus-backward above the inputs.  A timed call starts
from fresh clones of the inputs, so it includes building the autograd graph, on both sides alike.  One JSON line per case.

    python tools/image_sample_ab.py [--repeat 10] [--warmup 3] [--batch 8] [--res 70] [--out FILE]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import grids, imagefeat  # noqa: E402

MAPS = [(64, 64), (128, 64), (256, 64), (512, 64), (512, 64)]       # (channels, side): VGG-16's five stages resized to 64 x 64
N_GLOBAL = 1000


def grid_camera():
    """(rotation [1,3,3], position [1,3], projection [3,1], grid scale) of grids.project_faces' defaults"""
    d = {k: v.default for k, v in inspect.signature(grids.project_faces).parameters.items() if v.default is not inspect.Parameter.empty}
    ax, ay = d["rot"]
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    R = Rx @ Ry
    return (torch.from_numpy(R).float()[None], torch.from_numpy(R.T @ np.array([0.0, 0.0, d["cam_z"]])).float()[None],
            torch.tensor([[d["focal"]], [d["focal"]], [-1.0]]), d["coef"])


def torch_sample_f(pos, feats, cam_pos, cam_rot, cam_proj):
    uv = imagefeat.project_to_image(pos, cam_rot, cam_pos, cam_proj)
    parts = [feats[0][:, :, None].expand(-1, -1, pos.shape[1])] if feats[0] is not None else []
    parts += [F.grid_sample(m, uv.unsqueeze(2), mode="bilinear", padding_mode="zeros", align_corners=False).squeeze(3) for m in feats[1:]]
    return torch.cat([torch.cat(parts, 1), pos.permute(0, 2, 1)], 1)


def ours_sample_f(pos, feats, cam_pos, cam_rot, cam_proj):
    if feats[0] is None:
        from deftet_amd import hip_ops
        uv = imagefeat.project_to_image(pos, cam_rot, cam_pos, cam_proj)
        return hip_ops.image_sample(feats[1:], uv, append=pos)
    return imagefeat.sample_f(pos, feats, cam_pos, cam_rot, cam_proj)


def timed(fn, gout):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    if gout is not None:
        out.backward(gout)
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
                del inputs
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
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_sample_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B = "cuda", a.batch
    g = torch.Generator().manual_seed(0)
    rot, cam_pos, proj, coef = grid_camera()
    rot, cam_pos, proj = rot.expand(B, 3, 3).contiguous().to(dev), cam_pos.expand(B, 3).contiguous().to(dev), proj.to(dev)
    verts = (torch.from_numpy(grids.kuhn_grid(a.res)[0]).float() - 0.5) * coef
    maps0 = [torch.randn(B, c, s, s, generator=g).to(dev) for c, s in MAPS]
    glob0 = torch.randn(B, N_GLOBAL, generator=g).to(dev)
    C_maps = sum(c for c, _ in MAPS)
    lines = []
    for N in (verts.shape[0], 10000):
        pick = torch.arange(N) if N == verts.shape[0] else torch.randperm(verts.shape[0], generator=g)[:N]
        pos0 = (verts[pick][None] + 0.002 * torch.randn(B, N, 3, generator=g)).to(dev)
        uv = imagefeat.project_to_image(pos0, rot, cam_pos, proj)
        outside = float(((uv.abs() >= 1).any(-1)).float().mean())
        for with_global in (True, False):
            G = N_GLOBAL if with_global else 0
            gout = torch.randn(B, G + C_maps + 3, N, device=dev)

            def make(grad, pos0=pos0, with_global=with_global):
                feats = [glob0.clone().requires_grad_(grad) if with_global else None] + [m.clone().requires_grad_(grad) for m in maps0]
                return pos0.clone().requires_grad_(grad), feats, cam_pos, rot, proj
            rec = ab("image_sample_f.B%d.N%d.G%d" % (B, N, G), make, ours_sample_f, torch_sample_f, gout, a.repeat, a.warmup)
            rec["uv_outside_fraction"] = outside
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            del gout
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
