#!/usr/bin/env python
"""Generates tests/golden/ref_native_builders_irregular.npz: what the reference's native builders
(utils/lib/{tet_adj_share,tet_face_adj,tet_point_adj}/run.cpp, compiled into oracle/_ref by oracle/Makefile) return on the
irregular meshes of tests/builder_cases.py — many-owner faces, duplicate tets, repeated vertices, n_point at the face-key limit,
sizes around the sort / scan switches.  Only inputs and outputs are stored — no reference source.

    make -C oracle && python tests/golden/gen_ref_native_irregular.py    # needs the reference tree (REF=<path> for make)

Per family <name>: <name>_tets, <name>_n_point, <name>_adj_share, <name>_face_adj, <name>_point_adj, rows in the order the native
code writes them (tet_point_adj in its hash order: compare lex-sorted).  Face ids are below 4 * 2,049 < 65,536 and tet ids below
2,049, so adj_share and face_adj are stored as uint16 to keep the file small; point_adj keeps int32 (vertex ids reach 2,097,150).

The reference's tet_face_adj interface allocates 4 * n_tet * 50 rows and its run.cpp writes past them unchecked.  Every family is
therefore first counted with the oracle and must stay within 200 * T rows; a family that does not is changed in builder_cases.py,
never skipped here.  `fan_dense12` (24,552 rows for T = 66) exists for the library's own capacity handling and is never handed
to the reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from tests import builder_cases as BC  # noqa: E402


def main():
    O.build()
    if not O.RefBuilders.available():
        raise SystemExit("oracle/_ref is not built: make -C oracle ref REF=<reference tree>")
    ref = O.RefBuilders()
    rec = {}
    for name in BC.REF_NATIVE:
        tets, n_point = BC.case(name)
        T = tets.shape[0]
        n_rows = O.tet_face_adj(tets, n_point, wrap32=True).shape[0]
        assert n_rows <= 200 * T, "%s: %d face-adjacency rows exceed the reference's 200*T = %d buffer" % (name, n_rows, 200 * T)
        share, fadj, padj = ref.tet_adj_share(tets, n_point), ref.tet_face_adj(tets, n_point), ref.tet_point_adj(tets, n_point)
        assert fadj.shape[0] == n_rows
        assert share.max(initial=0) < 65536 and fadj.max(initial=0) < 65536 and share.min(initial=0) >= 0 and fadj.min(initial=0) >= 0
        rec.update({name + "_tets": tets, name + "_n_point": np.int64(n_point), name + "_adj_share": share.astype(np.uint16),
                    name + "_face_adj": fadj.astype(np.uint16), name + "_point_adj": padj})
        print("%-16s T=%5d n_point=%8d share=%6d face_adj=%7d (cap %7d) point_adj=%6d" % (
            name, T, n_point, share.shape[0], n_rows, 200 * T, padj.shape[0]))
    out = os.path.join(HERE, "ref_native_builders_irregular.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
