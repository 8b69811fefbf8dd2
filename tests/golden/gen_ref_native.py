#!/usr/bin/env python
"""Generates tests/golden/ref_native_builders.npz: inputs and outputs of the reference's four native builders
(utils/lib/{tet_adj_share,tet_face_adj,tet_point_adj,colaps_v}/run.cpp, compiled with the reference's own flags into
oracle/_ref by oracle/Makefile).  Only inputs and outputs are stored — no reference source.

    make -C oracle ref && python tests/golden/gen_ref_native.py          # needs the reference tree (REF=<path> for make)

What is pinned (tests/test_cpu_oracle_golden.py compares the oracle with it):
  s<seed>_*   seeds 0-5: a Kuhn grid of res 4 / 6 / 8 with its tets shuffled, vertices relabelled, corners re-ordered and
              20 % of the tets dropped; the native tet_adj_share, tet_face_adj and tet_point_adj rows in the order the
              native code writes them; colaps_v on 500 points built to hit its rounding ties (%.5f keys, signed zeros).
  wrap_*      tet_face_adj with n_point = 70000 > 46340, where the native edge key (a 32-bit int) wraps.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402
from oracle import oracle as O  # noqa: E402


def random_mesh(rng, res):
    verts, tets = grids.kuhn_grid(res)
    tets = tets[rng.permutation(tets.shape[0])]
    relabel = rng.permutation(verts.shape[0]).astype(np.int32)
    tets = relabel[tets]
    for t in tets:                      # random local re-orderings (orientation is irrelevant to the builders)
        rng.shuffle(t)
    keep = rng.random(tets.shape[0]) > 0.2
    return tets[keep].astype(np.int32), verts.shape[0]


def colaps_points(rng):
    pts = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    pts[100:200] = pts[:100] + rng.choice([0, 1e-7, 4e-6, 1e-5], (100, 3)).astype(np.float32)
    pts[200:220] = np.round(pts[200:220], 5) + np.float32(5e-6)        # rounding ties of %.5f
    pts[220] = 0.0
    pts[221] = -0.0                                                     # "-0.00000" != "0.00000"
    pts[222] = -1e-7
    return pts


def main():
    if not O.RefBuilders.available():
        raise SystemExit("oracle/_ref is not built: make -C oracle ref REF=<reference tree>")
    ref = O.RefBuilders()
    rec = {}
    for seed in range(6):
        rng = np.random.default_rng(seed)
        tets, n_point = random_mesh(rng, 4 + 2 * (seed % 3))
        pts = colaps_points(rng)
        m, inv = ref.colaps_v(pts)
        rec.update({"s%d_tets" % seed: tets, "s%d_n_point" % seed: np.int64(n_point), "s%d_pts" % seed: pts,
                    "s%d_adj_share" % seed: ref.tet_adj_share(tets, n_point), "s%d_face_adj" % seed: ref.tet_face_adj(tets, n_point),
                    "s%d_point_adj" % seed: ref.tet_point_adj(tets, n_point), "s%d_colaps_m" % seed: m, "s%d_colaps_inv" % seed: inv})
    rng = np.random.default_rng(3)
    tets, n_small = random_mesh(rng, 4)
    n_point = 70000
    tets = np.sort(rng.choice(n_point, n_small, replace=False)).astype(np.int32)[tets]
    rec.update({"wrap_tets": tets, "wrap_n_point": np.int64(n_point), "wrap_face_adj": ref.tet_face_adj(tets, n_point)})
    out = os.path.join(HERE, "ref_native_builders.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
