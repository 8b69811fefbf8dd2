#!/usr/bin/env python
"""Generates tests/golden/builders_irregular.npz by IMPORTING the reference's Python twins of the builders (as gen_golden.py
does, through its prepare_reference_import) and running them on the non-degenerate irregular meshes of tests/builder_cases.py:
three_on_face, dup, fan20, maxn, one.  Only inputs and outputs are stored — no reference source.

    make -C oracle && python tests/golden/gen_golden_irregular.py              # needs the reference tree
    python tests/golden/gen_golden_irregular.py --degenerate-report            # prints only, writes nothing

Per family <name> (keys are prefixed with it):
  tets, n_point
  face_fx3, face_tetidx_fx2, face_tetfaceidx_fx2, boundary_fx3     utils/tet_utils.py tet_to_face (:208-256)
  facewb_fx3, facewb_tetidx_fx2, facewb_tetfaceidx_fx2            prepare_for_wz.py tet_to_face_idx(with_boundary=True) (:49-104)
  face_withtet_4tx2 | withtet_raises                               utils/tet_utils.py tet_to_face_withtet (:259-300)
  adj_share_nbr_tx4 | nbr_raises                                   utils_tetsv.tet_adj_share (:16-75), the T x 4 table
  adj_share_0..3    | adj_share_raises                             utils/tet_utils.py tet_adj_share (:318-367)
  edges, tet_edge                                                  prepare_for_wz.py generate_edge (:184-203), generate_tet_edge_idx (:223-236)
  adj_table, adjsum | point_adj_raises                             prepare_for_wz.py generate_point_adj_idx (:132-146)
A `*_raises` entry is 0 (returned), 1 (IndexError: the functions index an empty row list when no face is shared, before
returning the table they have already filled) or 2 (ValueError: a face with more than two owners); the outputs are stored only
when it is 0.  `maxn_point_adj_raises` is 3: generate_point_adj builds a dense float32 n_point x n_point matrix, 17.6 TB at
n_point = 2,097,151, which is not attempted.

Degenerate families (any tet with a repeated vertex) are NOT pinned to the twins.  The twins whose loop reads
`if p != face_p_a and p != face_p_b: face_p_c = p` (tet_to_face, tet_to_face_withtet, tet_to_face_adj_sparse,
prepare_for_wz.tet_to_face_idx, and tet_adj_share with its `c`) never reset that variable between faces: on a face with a
repeated vertex no corner lies strictly between the minimum and the maximum, so the key is built from whatever the PREVIOUS
face left behind — it depends on the order of the tets — and the very first face of a mesh raises UnboundLocalError.
utils_tetsv.tet_adj_share sorts the three corners instead and is well defined, but keys (a,a,b) with mid = a where the native
run.cpp keys it with the third corner.  `--degenerate-report` runs every twin once on every degenerate family and prints whether
it raised, equalled the oracle or differed.  Seen: tet_utils.tet_to_face raises UnboundLocalError on `n1` and returns tables
that differ from the oracle's on every other degenerate family; tet_utils.tet_adj_share raises UnboundLocalError on `n1` and
ValueError on all the others — also on `self_owned`, `soup256_2048` and `soup256_2049`, where no face has three owners, because
the stale value merges unrelated faces under one key; utils_tetsv.tet_adj_share equals the oracle's neighbour table on those
three and raises ValueError, as the oracle does, on the rest.  The oracle does not follow the stale
variable: it restates the native run.cpp builders, which seed `c` explicitly (third corner in tet_adj_share, first corner in
tet_face_adj's absolute face id), and the library documents that behaviour for all its face tables ("Irregular
input").  ref_native_builders_irregular.npz pins it on the degenerate families.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from tests import builder_cases as BC  # noqa: E402

RAISES = {IndexError: 1, ValueError: 2}
DENSE_LIMIT = 1 << 31                                       # bytes of the dense n_point x n_point float32 matrix we are willing to build


def attempt(fn):
    try:
        return fn(), 0
    except (IndexError, ValueError) as e:
        return None, RAISES[type(e)]


def split_adj(adj_list):
    out = []
    for a in adj_list:
        idx = a.coalesce().indices().numpy().T
        out.append(idx.astype(np.int64).copy())
    return out


def twins_fixture(name, tets, n_point, tu, pw, tsv):
    t64 = tets.astype(np.int64)
    tl = [list(map(int, t)) for t in t64]
    out = {"tets": tets, "n_point": np.int64(n_point)}
    f3, t2, tf2, b3 = tu.tet_to_face(n_point, tl)
    out.update(face_fx3=np.asarray(f3, np.int64).reshape(-1, 3), face_tetidx_fx2=np.asarray(t2, np.int64).reshape(-1, 2),
               face_tetfaceidx_fx2=np.asarray(tf2, np.int64).reshape(-1, 2), boundary_fx3=np.asarray(b3, np.int64).reshape(-1, 3))
    g3, g2, gf2 = pw.tet_to_face_idx(n_point, t64, with_boundary=True)
    out.update(facewb_fx3=g3.reshape(-1, 3), facewb_tetidx_fx2=g2.reshape(-1, 2), facewb_tetfaceidx_fx2=gf2.reshape(-1, 2))
    verts = np.zeros((n_point, 0))                          # tet_to_face_withtet reads only points.shape[0]
    wt, code = attempt(lambda: tu.tet_to_face_withtet(verts, tl))
    out["withtet_raises"] = np.int64(code)
    if not code:
        out["face_withtet_4tx2"] = wt.astype(np.int64)
    res, code = attempt(lambda: tsv.tet_adj_share(t64, n_point))
    out["nbr_raises"] = np.int64(code)
    if not code:
        out["adj_share_nbr_tx4"] = np.asarray(res[-1]).astype(np.int64)
    share, code = attempt(lambda: split_adj(tu.tet_adj_share(t64, n_point)))
    out["adj_share_raises"] = np.int64(code)
    if not code:
        for i in range(4):
            out["adj_share_%d" % i] = share[i]
    e = pw.generate_edge(t64)
    out.update(edges=e, tet_edge=pw.generate_tet_edge_idx(t64, e))
    if n_point * n_point * 4 > DENSE_LIMIT:
        out["point_adj_raises"] = np.int64(3)
    else:
        table, adjsum = pw.generate_point_adj_idx(n_point, t64)
        out.update(point_adj_raises=np.int64(0), adj_table=table, adjsum=adjsum)
    return {name + "_" + k: v for k, v in out.items()}


def degenerate_report(tu, pw, tsv):
    from oracle import oracle as O
    O.build()

    def outcome(fn, want):
        try:
            got = fn()
        except Exception as e:                              # noqa: BLE001 — the report is about which exception
            return type(e).__name__
        same = all(np.asarray(a).size == np.asarray(b).size and np.array_equal(np.asarray(a).reshape(np.asarray(b).shape), b)
                   for a, b in zip(got, want))
        return "equal" if same else "differs"

    for name in BC.DEGENERATE:
        tets, n_point = BC.case(name)
        t64 = tets.astype(np.int64)
        tl = [list(map(int, t)) for t in t64]
        of3, ot2, otf2, ob3, nm = O.tet_to_face(tets, n_point)
        r_face = outcome(lambda: tu.tet_to_face(n_point, tl), (of3, ot2, otf2, ob3))
        try:
            want_nbr = O.tet_neighbours(tets, n_point)[0]
            r_nbr = outcome(lambda: (tsv.tet_adj_share(t64, n_point)[-1],), (want_nbr,))
        except ValueError:
            r_nbr = outcome(lambda: (tsv.tet_adj_share(t64, n_point)[-1],), ()) + " (oracle: ValueError)"
        rows = O.tet_adj_share(tets, n_point)
        want_share = [BC_lex(rows[rows[:, 2] == i][:, :2].astype(np.int64)) for i in range(4)]
        r_share = outcome(lambda: split_adj(tu.tet_adj_share(t64, n_point)), want_share)
        print("%-16s many-owner=%3d  tet_utils.tet_to_face: %-18s utils_tetsv.tet_adj_share: %-32s tet_utils.tet_adj_share: %s" % (
            name, nm, r_face, r_nbr, r_share))


def BC_lex(rows):
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))] if rows.size else rows.reshape(0, 2)


def main():
    if not os.path.isdir(GG.REF):
        raise SystemExit("reference tree not present; fixtures can only be generated in the authoring container")
    GG.prepare_reference_import()
    from utils import tet_utils as tu
    import prepare_for_wz as pw
    import utils_tetsv as tsv
    if "--degenerate-report" in sys.argv:
        degenerate_report(tu, pw, tsv)
        return
    rec = {}
    for name in BC.NON_DEGENERATE:
        tets, n_point = BC.case(name)
        assert not BC.has_repeated_vertex(tets), name
        rec.update(twins_fixture(name, tets, n_point, tu, pw, tsv))
    out = os.path.join(HERE, "builders_irregular.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")
    for k in sorted(rec):
        if k.endswith("_raises"):
            print("  %-32s %d" % (k, int(rec[k])))


if __name__ == "__main__":
    main()
