"""The numpy restatement of conforming selective refinement (tests/refine_ref.py) against hand-worked refinements and against
what a conforming refinement must be on the grids the GPU test uses; and the host side of the feature: hip_ops.occupancy_band
(plain torch), the header's version note, the workspace refusals of the entry points, the refusals of the front ends."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import refine_cases as C
from tests import refine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["deftet_tet_refine_mark_i64", "deftet_tet_refine_count_i64", "deftet_tet_refine_fill_f32", "deftet_tet_refine_workspace_bytes"]
EINVAL = -1
P = ctypes.c_void_p(1 << 20)                                          # a non-null, 256-byte aligned pointer that is never followed


@pytest.fixture(autouse=True, scope="module")
def _the_operator_exists():
    """the restatement restates hip_ops.refine_tets; on a tree without the operator these tests have no subject, and fail"""
    from deftet_amd import hip_ops
    assert hasattr(hip_ops, "refine_tets") and hasattr(hip_ops, "refine_marks") and hasattr(hip_ops, "occupancy_band")


def test_child_table_is_the_contract():
    assert sorted(R.CHILDREN) == [0, 1, 2, 4, 8, 0x0B, 0x0C, 16, 0x12, 0x15, 32, 0x21, 0x26, 0x38, 63]
    assert [len(R.CHILDREN[m]) for m in (0, 1, 0x21, 0x0B, 63)] == [1, 2, 4, 4, 8]
    # a green child replaces corner i by a midpoint of an edge AT corner i (so it keeps the parent's orientation), or keeps it;
    # the eight children of a full split are the reference's, in its corner order
    for mask, kids in R.CHILDREN.items():
        for kid in kids if mask != 63 else []:
            for i, code in enumerate(kid):
                assert code == i or (code >= 4 and i in R.ENDS[code - 4] and mask >> (code - 4) & 1), (mask, kid)
    # the local fixed point: two edges of a face complete it, opposite edges stay
    assert R.LOCAL_CLOSE[0b000011] == 0x0B and R.LOCAL_CLOSE[0x21] == 0x21 and R.LOCAL_CLOSE[0b000110] == 0x26 and R.LOCAL_CLOSE[0b000111] == 63


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_worked(name):
    h = C.HAND[name]
    pts, feat = C.hand_points(h["n_point"])
    r = R.refine(h["tets"], pts, feat, h["select"])
    assert r.tet_new.tolist() == h["tet_new"].tolist()
    assert r.parent.tolist() == h["parent"].tolist() and r.kind.tolist() == h["kind"].tolist() and r.kind.dtype == np.uint8
    assert r.edges_split.tolist() == h["edges_split"].tolist()
    Pn = h["n_point"]
    assert r.points_new.dtype == np.float32 and r.points_new[:Pn].tobytes() == pts.tobytes() and r.feat_new[:Pn].tobytes() == feat.tobytes()
    for k, (a, b) in enumerate(h["edges_split"]):
        assert (r.points_new[Pn + k] == (pts[a] + pts[b]) / 2).all() and (r.feat_new[Pn + k] == (feat[a] + feat[b]) / 2).all()


def test_the_five_patterns_are_the_closed_ones():
    """no face with exactly two marked slots <=> none, one edge, two opposite edges, a face, all six: so closed marks never hold
    another pattern, whatever edge ids the slots carry (repeated vertices put one id into several slots)"""
    closed = [m for m in range(64) if all(bin(m & f).count("1") != 2 for f in R.FACE_MASK)]
    assert closed == R.LEGAL == [m for m in range(64) if R.LOCAL_CLOSE[m] == m]
    kinds = {0: [0], 1: [1 << e for e in range(6)], 2: [(1 << e) | (1 << (5 - e)) for e in range(3)], 3: R.FACE_MASK, 6: [63]}
    assert sorted(m for v in kinds.values() for m in v) == closed


@pytest.mark.parametrize("name", ["degenerate", "self_owned", "n1", "dup", "collapsed8_dups", "soup40_171"])
def test_irregular_lists_refine_without_an_illegal_pattern(name):
    from tests import builder_cases as B
    tets, n_point = B.case(name)
    pts = np.random.default_rng(1).random((n_point, 3)).astype(np.float32)
    for seed in range(3):
        sel = np.random.default_rng(seed).random(len(tets)) < 0.3
        r = R.refine(tets, pts, pts[:, :1], sel)
        assert (np.bincount(r.parent, minlength=len(tets)) == np.array([1, 2, 4, 4, 0, 0, 8])[r.kind[np.unique(r.parent, return_index=True)[1]]]).all()
    e, te = R.tet_edges(tets, n_point)
    te[len(tets) // 2, 2] = e.shape[0]
    with pytest.raises(IndexError):
        R.refine(tets, pts, pts, np.ones(len(tets), bool), e, te)


@pytest.mark.parametrize("sel", C.SELECTIONS)
@pytest.mark.parametrize("name", C.GRIDS)
def test_refinement_is_conforming(name, sel):
    tets, pts, _ = C.grid(name)
    select = C.selection(name, sel)
    r = C.reference(name, sel)
    T, Pn = tets.shape[0], pts.shape[0]
    edges, tet_edge = R.tet_edges(tets, Pn)
    first = R.initial_marks(tet_edge, select, edges.shape[0])
    assert select.sum() > 0 and first.sum() > 0
    # the closed marks hold the initial ones, and an in-place iteration in reversed tet order ends at the same marks
    assert (r.marks >= first).all()
    gs, _ = R.close_gauss_seidel(tet_edge, first, range(T - 1, -1, -1))
    assert (gs == r.marks).all()
    # only the five patterns
    pat = R.patterns(tet_edge, r.marks)
    assert R.IS_LEGAL[pat].all() and set(R.POPCOUNT[pat].tolist()) <= {0, 1, 2, 3, 6}
    assert (r.kind == R.POPCOUNT[pat][r.parent]).all() and (np.bincount(r.parent, minlength=T) == R.N_CHILD[pat]).all()
    assert r.edges_split.tolist() == edges[r.marks].tolist() and r.points_new.shape[0] == Pn + int(r.marks.sum())
    # conforming: no face with more than two owners, and every one-owner face lies in a one-owner face of the input
    _, owners = R.face_owner_counts(r.tet_new)
    assert R.face_owner_counts(tets)[1].max() <= 2 and owners.max() <= 2
    assert R.hull_faces_subdivide(tets, r)
    # children keep the orientation, and fill their parents (fp64 on the exact midpoints)
    assert R.volumes(pts, tets).min() > 0
    vol = R.volumes(R.points64(pts, r.edges_split), r.tet_new)
    assert vol.min() > 0
    want = R.volumes(pts, tets).sum()
    assert abs(vol.sum() - want) <= 1e-12 * want
    per_parent = np.bincount(r.parent, weights=vol, minlength=T)
    assert np.allclose(per_parent, R.volumes(pts, tets), rtol=1e-9, atol=0)


def test_the_unclosed_selective_split_is_not_conforming():
    """what the closure is for: splitting the selected tets only leaves a midpoint on faces the neighbour owns whole"""
    tets, pts, _ = C.grid("kuhn8")
    select = C.selection("kuhn8", "band")
    edges, tet_edge = R.tet_edges(tets, pts.shape[0])
    kids = np.asarray(R.CHILDREN[63])
    src = np.concatenate([tets, pts.shape[0] + tet_edge], 1)
    split = np.concatenate([tets[~select], src[select][:, kids].reshape(-1, 4)], 0)
    assert len(R.one_owner_faces(split)) > len(R.one_owner_faces(C.reference("kuhn8", "band").tet_new))


def test_all_and_none():
    tets, pts, _ = C.grid("kuhn8")
    feat = C.features(pts, 2)
    r = R.refine(tets, pts, feat, np.zeros(len(tets), bool))
    assert r.tet_new.tolist() == tets.tolist() and r.parent.tolist() == list(range(len(tets))) and r.edges_split.shape == (0, 2)
    assert r.points_new.tobytes() == pts.tobytes() and not r.kind.any()
    r = R.refine(tets, pts, feat, np.ones(len(tets), bool))
    edges, tet_edge = R.tet_edges(tets, pts.shape[0])
    assert r.edges_split.tolist() == edges.tolist() and (r.kind == 6).all() and r.tet_new.shape[0] == 8 * len(tets)
    src = np.concatenate([tets, pts.shape[0] + tet_edge], 1)
    assert r.tet_new.tolist() == src[:, np.asarray(R.CHILDREN[63])].reshape(-1, 4).tolist()


def test_random_selection_needs_many_rounds():
    """the case the GPU test uses to cross a read-back group: even swept in place, tet after tet, it needs more than four sweeps"""
    tets, pts, _ = C.grid("kuhn20")
    select = C.selection("kuhn20", "random")
    edges, tet_edge = R.tet_edges(tets, pts.shape[0])
    first = R.initial_marks(tet_edge, select, edges.shape[0])
    assert C.reference("kuhn20", "random").rounds > 8
    for order in (range(len(tets)), range(len(tets) - 1, -1, -1)):
        assert R.close_gauss_seidel(tet_edge, first, order)[1] >= 4      # changing sweeps; the one that proves closure comes on top


# ---------------------------------------------------------------------------- hip_ops.occupancy_band (plain torch: runs anywhere)
@pytest.mark.parametrize("name", ["kuhn8", "cube40"])
def test_occupancy_band_is_the_restated_one(name):
    from deftet_amd import hip_ops
    tets, pts, nbr = C.grid(name)
    rng = np.random.default_rng(3)
    ins = np.stack([R.sphere_inside(pts, tets), rng.random(len(tets)) < 0.02, np.zeros(len(tets), bool)])
    tn = torch.from_numpy(nbr)
    for rings in (0, 1, 3):
        for x in (ins, ins[0], ins[2:]):
            got = hip_ops.occupancy_band(torch.from_numpy(x), tn, rings)
            assert got.dtype == torch.bool and got.shape == (len(tets),) and got.numpy().tolist() == R.occupancy_band(x, nbr, rings).tolist()
    assert not hip_ops.occupancy_band(torch.from_numpy(ins[2]), tn, 2).any()
    assert hip_ops.occupancy_band(torch.from_numpy(ins[0].astype(np.float32)), tn).numpy().tolist() == R.occupancy_band(ins[0], nbr).tolist()
    band0, band1 = R.occupancy_band(ins[0], nbr, 0), R.occupancy_band(ins[0], nbr, 1)
    assert 0 < band0.sum() < band1.sum() < len(tets) and (band1 >= band0).all()
    with pytest.raises(RuntimeError, match="occupancy_band"):
        hip_ops.occupancy_band(torch.from_numpy(ins[0][:-1]), tn)
    with pytest.raises(ValueError, match="rings"):
        hip_ops.occupancy_band(torch.from_numpy(ins[0]), tn, -1)
    assert "Plain torch ops" in hip_ops.occupancy_band.__doc__


# ---------------------------------------------------------------------------- the host side of the entry points
@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


def test_header_note_ctypes_table_and_library_agree(lib):
    from deftet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    note = re.search(r"^/?\*? *380:(.*?)^ \* 370:", txt, flags=re.S | re.M)
    assert note, "no 380: version note"
    for s in SYMBOLS:
        assert s in note.group(1), s
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 380


@pytest.mark.parametrize("T,E", [(0, 0), (1, 6), (6000, 7930), (47472, 60000)])
def test_workspace_is_the_layout_and_one_byte_short_is_refused(lib, T, E):
    size = lib.deftet_tet_refine_workspace_bytes
    want = size(T, E)
    assert want > 0 and want % 256 == 0 and want >= 4 * E + 8 * T
    assert size(T + 4096, E) > want and size(-3, -3) == size(0, 0)
    before = lib.deftet_builder_workspace_bytes(1000, 6000)
    count = lambda ws, n: lib.deftet_tet_refine_count_i64(P, P, P, 10, T, E, P, ws, n, None)
    fill = lambda ws, n: lib.deftet_tet_refine_fill_f32(P, P, P, P, P, P, 10, T, E, 2, E, 8 * T, P, P, P, P, P, P, ws, n, None)
    for call in (count, fill):
        assert call(P, want - 1) == EINVAL and b"workspace null, misaligned or too small: need %d bytes" % want in lib.deftet_last_error()
        assert call(None, want) == EINVAL and b"workspace" in lib.deftet_last_error()
        assert call(ctypes.c_void_p(P.value + 16), want) == EINVAL and b"aligned" in lib.deftet_last_error()
    assert lib.deftet_builder_workspace_bytes(1000, 6000) == before


def test_bad_arguments_are_refused_by_name(lib):
    mark = lambda T=10, E=20, reset=1, n=4, marks=P, counts=P, bad=P, te=P, sel=P: lib.deftet_tet_refine_mark_i64(te, sel, T, E, reset, n, marks, counts, bad, None)
    assert mark(T=-1) == EINVAL and b"negative size" in lib.deftet_last_error()
    assert mark(E=61) == EINVAL and b"6 n_tet" in lib.deftet_last_error()
    assert mark(n=65) == EINVAL and b"n_sweeps" in lib.deftet_last_error()
    assert mark(n=-1) == EINVAL
    assert mark(bad=None) == EINVAL and mark(counts=None) == EINVAL and mark(marks=None) == EINVAL and mark(te=None) == EINVAL
    assert mark(sel=None) == EINVAL and b"select" in lib.deftet_last_error()
    ws = lib.deftet_tet_refine_workspace_bytes(10, 20)
    assert lib.deftet_tet_refine_count_i64(P, P, P, 10, 10, 20, None, P, ws, None) == EINVAL and b"totals" in lib.deftet_last_error()
    assert lib.deftet_tet_refine_count_i64(P, P, P, -1, 10, 20, P, P, ws, None) == EINVAL
    fill = lambda M=5, Tn=30, K=2, tet_new=P, split=P: lib.deftet_tet_refine_fill_f32(P, P, P, P, P, P, 10, 10, 20, K, M, Tn, P, P, tet_new, P, P, split, P, ws,
                                                                                     None)
    assert fill(M=21) == EINVAL and b"count pass" in lib.deftet_last_error()
    assert fill(Tn=81) == EINVAL and fill(K=-1) == EINVAL
    assert fill(tet_new=None) == EINVAL and b"tet_new" in lib.deftet_last_error()
    assert fill(split=None) == EINVAL and b"edges_split" in lib.deftet_last_error()


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    from deftet_amd import hip_ops
    from deftet_amd.render import prepare_for_wz
    tet, pts = torch.tensor([[0, 1, 2, 3]]), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.refine_tets(tet, pts, pts, torch.ones(1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.refine_marks(torch.zeros(1, 6, dtype=torch.long), torch.ones(1, dtype=torch.bool), 6)
    assert hip_ops.RefinedTets._fields == ("points_new", "feat_new", "tet_new", "parent", "kind", "edges_split")
    assert callable(prepare_for_wz.generate_conforming_subdivision)
