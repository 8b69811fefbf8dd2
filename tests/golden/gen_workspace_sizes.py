#!/usr/bin/env python
"""Generates tests/golden/workspace_sizes.json: what every *_workspace_bytes function whose size comes from a layout function
returned BEFORE the layouts were introduced, at the shapes of tests/test_workspace_layout_cpu.py and at the workload's own.

    DEFTET_HIP_LIB=<libdeftet_hip.so built from the commit before the layouts> python tests/golden/gen_workspace_sizes.py [FUNCTION ...]

With function names only their rows are measured (the commit before THEIR layout: deftet_pointvoxel_workspace_bytes and
deftet_image_sample_workspace_bytes came to cell_gather.hpp's layout later than the rest); every other function keeps its rows.

The library loads without a GPU: the size functions are host arithmetic.  Each row is {"args": [...], "parent": bytes}; the rows
at the workload's own shapes carry "workload": true (compared, never run).  A row where the parent under-declared what
its entry point carves additionally carries "parent_too_small": true, set by hand with the reason next to it (the test then
asserts >= instead of <=).  Rerunning keeps such marks.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "workspace_sizes.json")


def kuhn(r):
    """(V, T, unique faces, unique edges) of the res=r Kuhn grid of deftet_amd.grids: r / 2 cubes per axis, six tets each"""
    n = r // 2
    V, T, F = (n + 1) ** 3, 6 * n ** 3, 12 * n ** 3 + 6 * n ** 2
    return V, T, F, V + F - T - 1


V2, T2, F2, E2 = kuhn(2)
V8, T8, F8, E8 = kuhn(8)
VW, TW, FW, EW = kuhn(70)                                   # the workload: T = 257250, V = 46656
BW, NW, MW = 8, 80000, 97000

# function -> (the shapes the tests run at, the workload's own shapes: compared only)
SHAPES = {
    "deftet_nn_index_workspace_bytes": ([(9, 65, 300), (1, 1, 1)], [(BW, NW, MW)]),
    "deftet_tri_dist_workspace_bytes": ([(9, 65, 70)], [(BW, NW, 2 * MW)]),
    "deftet_face_edge_adj_workspace_bytes": ([(70,)], [(2 * MW,)]),
    "deftet_face_edge_adj_ragged_workspace_bytes": ([(33, 70)], [(BW, 2 * MW)]),
    "deftet_builder_workspace_bytes": ([(V2, T2), (V8, T8)], [(VW, TW)]),
    "deftet_tet_neighbours_workspace_bytes": ([(T2,), (T8,)], [(TW,)]),
    "deftet_boundary_index_workspace_bytes": ([(2, F8)], [(BW, FW)]),
    "deftet_tet_energies_workspace_bytes2": ([(2, T8)], [(BW, TW)]),
    "deftet_surface_extract_workspace_bytes": ([(2, 257, 0), (2, 257, 1)], [(BW, TW, 0), (BW, TW, 1)]),
    "deftet_surface_weld_workspace_bytes": ([(2100,)], [(VW,)]),
    "deftet_marching_tets_workspace_bytes": ([(2, T8, E8)], [(BW, TW, EW)]),
    "deftet_mesh_voxelize_workspace_bytes": ([(2, 300)], [(BW, 2 * MW)]),
    "deftet_voxel_surface_workspace_bytes": ([(2, 33)], [(BW, 100)]),
    "deftet_face_edges_workspace_bytes": ([(400,)], [(2 * MW,)]),
    "deftet_sample_points_workspace_bytes": ([(2, 1100)], [(BW, 2 * MW)]),
    "deftet_vertex_adjacency_workspace_bytes": ([(3000, 300)], [(2 * EW, VW)]),
    "deftet_tet_vertex_csr_workspace_bytes": ([(1, 125, 600)], [(1, VW, TW)]),
    "deftet_face_vertex_csr_workspace_bytes": ([(125, 600)], [(VW, FW)]),
    "deftet_edge_vertex_csr_workspace_bytes": ([(125, 600)], [(VW, EW)]),
    "deftet_tet_order_coherence_workspace_bytes": ([(300,)], [(TW,)]),
    "deftet_pointvoxel_workspace_bytes": ([(1, 257, 2), (3, 1000, 5), (2, 64, 8)], [(BW, VW, 32), (BW, VW, 8), (BW, 10000, 16)]),
    "deftet_image_sample_workspace_bytes": ([(1, 257, 1, 1), (3, 1000, 5, 4)], [(BW, VW, 64, 64)]),
}


def main():
    if not os.environ.get("DEFTET_HIP_LIB"):
        sys.exit("set DEFTET_HIP_LIB to a library built from the commit before the layouts")
    sys.path.insert(0, ROOT)
    from deftet_amd import _lib
    lib = _lib.load()
    old = json.load(open(OUT)) if os.path.exists(OUT) else {}
    marks = {(f, tuple(r["args"])): r for f, rows in old.items() for r in rows if r.get("parent_too_small")}
    out = {}
    for name, (small, workload) in SHAPES.items():
        if sys.argv[1:] and name not in sys.argv[1:]:
            out[name] = old[name]
            continue
        rows = []
        for args in small + workload:
            row = {"args": list(args), "parent": int(getattr(lib, name)(*args))}
            if args in workload:
                row["workload"] = True
            if (name, tuple(args)) in marks:
                row.update({k: v for k, v in marks[(name, tuple(args))].items() if k not in row})
            rows.append(row)
        out[name] = rows
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": [\n  %s\n ]' % (k, ",\n  ".join(json.dumps(r) for r in rows)) for k, rows in out.items()) + "\n}\n")
    print("wrote %s: %d functions, %d rows" % (OUT, len(out), sum(len(r) for r in out.values())))


if __name__ == "__main__":
    main()
