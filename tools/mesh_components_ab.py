#!/usr/bin/env python
"""A/B of the mesh clean-up on a batch of marching-tetrahedra surfaces, on the same GPU:

  A   hip_ops.mesh_cleanup_list(mesh, keep_largest=True, drop_voids=True): one launch sequence and one read-back for the batch
  B1  the host round trip: read every shape back, scipy connected_components on the face graph, numpy measures, selection and
      compaction, upload the result
  B2  min-label propagation in torch on the same GPU over the concatenated mesh: torch.unique over the edge keys, labels
      lowered to the smallest neighbour until nothing changes (one .any() read-back per sweep), index_add_ for the sizes and
      the volumes (float atomics), masks and cumsum for the compaction

Scene: the hollow ball of tests/mesh_components_cases.py (a shell 0.20 < r < 0.36 with a floater in its void and two in the
corners) on the res-70 grid of deftet_amd.grids, B = 8 copies scaled by 1 - 0.01 b: per shape five closed components.  The
three sides are compared before they are timed (faces and vertices of every shape, bit for bit).

Per step and side: the time (HIP events around the step, host work included, median / min / max of `--repeat` after `--warmup`,
the sides alternated inside the process), the device launches as the profiler counts them and the peak memory above the inputs.
One JSON line per run.

    python tools/mesh_components_ab.py [--repeat 20] [--warmup 5] [--res 70 --batch 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deftet_amd import grids, hip_ops  # noqa: E402

SIDES = ("A", "B1", "B2")


def hollow_field(pos, scale):
    def ball(c, rho):
        return rho * scale - (pos - torch.tensor(c, device=pos.device) * scale).norm(dim=1)
    r = pos.norm(dim=1)
    shell = torch.minimum(0.36 * scale - r, r - 0.20 * scale)
    return torch.stack([shell, ball((0.0, 0.0, 0.0), 0.08), ball((.4, .4, .4), 0.07), ball((-.41, .4, -.4), 0.05)]).amax(0)


# ---------------------------------------------------------------------------- B1: the host round trip
def host_cleanup(verts, faces):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    F, V = f.shape[0], v.shape[0]
    a, b = f, np.roll(f, -1, axis=1)
    key = (np.minimum(a, b) * np.int64(V) + np.maximum(a, b)).reshape(-1)
    _u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    M = sp.coo_matrix((np.ones(3 * F), (np.repeat(np.arange(F), 3), inv.reshape(-1))), shape=(F, cnt.size)).tocsr()
    _n, lab = connected_components(M @ M.T, directed=False)
    n_face = np.bincount(lab)
    x = v.astype(np.float64)
    vol = np.bincount(lab, weights=np.einsum("ij,ij->i", x[f[:, 0]], np.cross(x[f[:, 1]], x[f[:, 2]])) / 6.0)
    forward = np.bincount(inv.reshape(-1), weights=(a < b).reshape(-1).astype(np.float64), minlength=cnt.size)
    bad_edge = (cnt != 2) | (forward != 1)
    open_ = np.bincount(lab[np.repeat(np.arange(F), 3)], weights=bad_edge[inv.reshape(-1)].astype(np.float64), minlength=n_face.size) > 0
    alive = ~(~open_ & (vol < 0))
    first = np.full(n_face.size, F)
    np.minimum.at(first, lab, np.arange(F))
    size = np.where(alive, n_face, -1)
    best = np.lexsort((first, -size))[0]                             # the most faces, the smaller first face among equals
    keep = (lab == best) & alive[lab]
    used = np.zeros(V, bool)
    used[f[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    return torch.from_numpy(v[used]).to(verts.device), torch.from_numpy(new[f[keep]]).to(verts.device)


# ---------------------------------------------------------------------------- B2: label propagation in torch
def torch_cleanup(verts, faces, face_shape, n_shape, vfirst):
    """the concatenated mesh: (verts', faces' global, kept-vertex mask, kept-face mask)"""
    F, V, dev = faces.shape[0], verts.shape[0], verts.device
    a, b = faces, faces.roll(-1, 1)
    key = (torch.minimum(a, b) * V + torch.maximum(a, b)).reshape(-1)
    _u, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    E = cnt.numel()
    face_of = torch.arange(F, device=dev).repeat_interleave(3)
    lab = torch.arange(F, device=dev)
    while True:                                                     # faces <-> edges, lowered until a sweep changes nothing
        edge_min = torch.full((E,), F, device=dev, dtype=torch.int64).scatter_reduce_(0, inv, lab[face_of], "amin")
        new = torch.minimum(lab, edge_min[inv].view(F, 3).amin(1))
        new = new[new]                                              # pointer jumping
        if not bool((new != lab).any()):
            break
        lab = new
    n_face = torch.zeros(F, device=dev, dtype=torch.int64).index_add_(0, lab, torch.ones_like(lab))
    x = verts.double()
    vol = torch.zeros(F, device=dev, dtype=torch.float64).index_add_(
        0, lab, (x[faces[:, 0]] * torch.linalg.cross(x[faces[:, 1]], x[faces[:, 2]])).sum(1) / 6.0)
    forward = torch.zeros(E, device=dev, dtype=torch.int64).index_add_(0, inv, (a < b).reshape(-1).long())
    bad_edge = ((cnt != 2) | (forward != 1)).long()
    open_ = torch.zeros(F, device=dev, dtype=torch.int64).index_add_(0, lab[face_of], bad_edge[inv]) > 0
    root = lab == torch.arange(F, device=dev)
    alive = root & ~(~open_ & (vol < 0))
    score = torch.where(alive, n_face * (F + 1) + (F - torch.arange(F, device=dev)), torch.zeros_like(n_face))
    best = torch.zeros(n_shape, device=dev, dtype=torch.int64).scatter_reduce_(0, face_shape, score, "amax")
    keep_root = alive & (score == best[face_shape]) & (score > 0)
    keep = keep_root[lab]
    used = torch.zeros(V, device=dev, dtype=torch.bool)
    used[faces[keep].reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    return verts[used], new[faces[keep]], used, keep


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
    for side in SIDES[1:]:
        rec["A_over_" + side] = round(rec["A"]["ms"]["median"] / rec[side]["ms"]["median"], 4)
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
        raise SystemExit("mesh_components_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev, B = "cuda", a.batch
    verts, tets = grids.kuhn_grid(a.res)
    pos = torch.from_numpy(verts).float().to(dev) - 0.5              # the grid spans [0,1]^3
    field = torch.stack([hollow_field(pos, 1.0 - 0.01 * b) for b in range(B)])
    mesh = hip_ops.marching_tets(pos[None].expand(B, -1, -1).contiguous(), field,
                                 hip_ops.TetEdges(torch.from_numpy(tets).long().to(dev), pos.shape[0]))
    vs, fs = [v.detach() for v in mesh.verts], list(mesh.faces)
    nv, nf = [int(v.shape[0]) for v in vs], [int(f.shape[0]) for f in fs]
    voff = np.concatenate([[0], np.cumsum(nv)])
    vfirst = torch.from_numpy(voff[:-1]).to(dev)
    face_shape = torch.arange(B, device=dev).repeat_interleave(torch.tensor(nf, device=dev))
    kept = {}

    def step(side, keep=None):
        if side == "A":
            out = hip_ops.mesh_cleanup_list(vs, fs, None, keep_largest=True, drop_voids=True)
            res = list(zip(out.verts, out.faces))
        elif side == "B1":
            res = [host_cleanup(v, f) for v, f in zip(vs, fs)]
        else:
            v = torch.cat(vs)
            f = torch.cat(fs) + vfirst[face_shape][:, None]
            v2, f2, used, keepf = torch_cleanup(v, f, face_shape, B, vfirst)
            if keep is not None:                                    # cut back per shape for the comparison only
                vo = [0] + torch.cumsum(torch.stack([used[voff[b]:voff[b + 1]].sum() for b in range(B)]), 0).tolist()
                fo = [0] + torch.cumsum(torch.zeros(B, device=dev, dtype=torch.int64).index_add_(0, face_shape[keepf],
                                                                                                torch.ones_like(face_shape[keepf])), 0).tolist()
                res = [(v2[vo[b]:vo[b + 1]], f2[fo[b]:fo[b + 1]] - vo[b]) for b in range(B)]
            else:
                res = [(v2, f2)]
        if keep is not None:
            keep[side] = res

    for side in SIDES:
        step(side, kept)
    for side in SIDES[1:]:
        for b in range(B):
            for x, y in zip(kept["A"][b], kept[side][b]):
                if x.shape != y.shape or not torch.equal(x, y.to(x.dtype)):
                    raise SystemExit("mesh_components_ab: side %s differs from side A at shape %d" % (side, b))
    comps = [int(hip_ops.mesh_components(f, n).count[0]) for f, n in zip(fs, nv)]
    name = "mesh_cleanup_list.keep_largest+drop_voids.res%d.B%d.V%d.F%d.kept_F%d" % (a.res, B, sum(nv), sum(nf), sum(int(f.shape[0]) for _v, f in kept["A"]))
    rec = measure(name, step, a.repeat, a.warmup)
    rec["components_per_shape"] = comps
    rec["sides_agree"] = "bit for bit"
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
