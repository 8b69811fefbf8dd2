#!/usr/bin/env python
"""Stage times of ground-truth preparation (deftet_amd.dataprep) at the reference's resolution, against the numpy
restatement of the same rules on the host (tests/dataprep_ref.py).

Input: the welded hip_ops.surface_extract of a sphere occupancy (r = 0.3) on kuhn_grid(70), rescaled and centred as
MakeSurfaceMesh does (dataloader.py:27-32).  Stages at resolution R (default 100): mesh_voxelize, voxel_fill, the unfused
extract_odms + project_odms, voxel_surface_mesh, VertexAdjacency.from_faces, smooth_vertices (3 rounds), and
make_surface_mesh as a whole.  Every stage is timed with device events around the front-end call (host work and read-backs
of the call included: that is what a data loader pays), after warm-ups, median / min / max over the steps.  The host times are
one run each of the numpy restatement (--host-stages; the voxelization restatement loops over the triangles in Python).
One JSON line.

    python tools/dataprep_ab.py [--resolution 100] [--grid 70] [--steps 20] [--warmup 3] [--no-host]
    python tools/dataprep_ab.py --check        # tiny sizes on the host restatement only, no GPU call
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402
from tests import dataprep_ref as ref  # noqa: E402


def host_stages(v, f, R, iterations=3):
    """one run of every stage of the restatement: ({stage: seconds}, outputs)"""
    t, out = {}, {}

    def run(name, fn):
        t0 = time.perf_counter()
        out[name] = fn()
        t[name] = time.perf_counter() - t0
    run("mesh_voxelize", lambda: ref.mesh_voxelize_f32(v[None], f, R))
    run("extract_project_odms", lambda: ref.project_odms(ref.extract_odms(out["mesh_voxelize"])))
    run("voxel_surface_mesh", lambda: ref.voxel_surface_mesh(out["extract_project_odms"]))
    sv, sf = out["voxel_surface_mesh"][0][0], out["voxel_surface_mesh"][1][0]
    run("from_faces", lambda: ref.edge_csr(sf, sv.shape[0]))
    run("smooth_vertices", lambda: ref.smooth(sv, sf, iterations))
    t["make_surface_mesh"] = sum(t.values())
    return t, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resolution", type=int, default=100)
    ap.add_argument("--grid", type=int, default=70)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--check", action="store_true", help="tiny sizes, host restatement only")
    args = ap.parse_args(argv)
    if args.check:
        v, f = ref.icosphere(1)
        t, out = host_stages(v, f, 12)
        print(json.dumps({"check": "ok", "set_voxels": int(out["mesh_voxelize"].sum()), "stages": sorted(t)}))
        return 0

    import torch
    from deftet_amd import dataprep, hip_ops
    dev = torch.device("cuda:0")
    R = args.resolution
    verts, tets = grids.kuhn_grid(args.grid)
    nbr = hip_ops.tet_face_neighbours(tets, verts.shape[0], dev)
    pos = np.ascontiguousarray(verts[None], np.float32)
    tet_p = torch.from_numpy(grids.gather_tets(pos, tets)).to(dev)
    occ = ((tet_p.mean(dim=2) - 0.5).norm(dim=-1) < 0.3).float()
    soup = hip_ops.surface_extract(tet_p, occ, nbr, "binary", tet_idx=torch.from_numpy(tets.astype(np.int64)), return_faces=True)
    v_in, _a, f_in, _o = hip_ops.surface_weld(torch.from_numpy(pos[0]).to(dev), soup.faces[0])
    del tet_p, occ, soup
    v = v_in / (v_in.amax(0) - v_in.amin(0)).amax() * 0.9
    v = (v - (v.amax(0) + v.amin(0)) / 2).contiguous()

    bits = hip_ops.mesh_voxelize(v[None], f_in, R, return_bits=True)
    filled = hip_ops.voxel_fill(bits)
    vox = bits.unpack()
    sv, sf = hip_ops.voxel_surface_mesh(filled)
    adj = hip_ops.VertexAdjacency.from_faces(sf[0], sv[0].shape[0])
    stages = [("mesh_voxelize", lambda: hip_ops.mesh_voxelize(v[None], f_in, R, return_bits=True)),
              ("voxel_fill", lambda: hip_ops.voxel_fill(bits)),
              ("extract_project_odms", lambda: hip_ops.project_odms(hip_ops.extract_odms(vox))),
              ("voxel_surface_mesh", lambda: hip_ops.voxel_surface_mesh(filled)),
              ("from_faces", lambda: hip_ops.VertexAdjacency.from_faces(sf[0], sv[0].shape[0])),
              ("smooth_vertices", lambda: dataprep.smooth_vertices(sv[0], adj, 3)),
              ("make_surface_mesh", lambda: dataprep.make_surface_mesh(v_in, f_in, resolution=R))]
    times = {n: [] for n, _ in stages}
    for it in range(args.warmup + args.steps):
        for name, fn in stages:                                         # the stages alternate inside one process
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    row = {"config": "grid=%d input V=%d F=%d, R=%d: set %d, filled %d, surface V=%d F=%d, edges %d" %
           (args.grid, v_in.shape[0], f_in.shape[0], R, int(vox.sum()), int(filled.unpack().sum()), sv[0].shape[0], sf[0].shape[0], adj.nnz),
           "steps": args.steps, "warmup": args.warmup, "gpu_ms": {}}
    for name, _ in stages:
        t = np.asarray(times[name])
        row["gpu_ms"][name] = {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}
    if not args.no_host:
        ht, out = host_stages(v.cpu().numpy(), f_in.cpu().numpy(), R)
        if not np.array_equal(out["extract_project_odms"], filled.unpack().cpu().numpy()):
            # general floats: the voxelizations may differ inside the fp64 margin (tests/test_dataprep_gpu.py); report, do not hide
            row["filled_voxels_differing"] = int((out["extract_project_odms"] != filled.unpack().cpu().numpy()).sum())
        row["host_ms"] = {k: round(s * 1e3, 2) for k, s in ht.items()}
        row["host_over_gpu"] = {k: round(ht[k] * 1e3 / row["gpu_ms"][k]["median"], 1) for k in ht if k in row["gpu_ms"]}
    print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
