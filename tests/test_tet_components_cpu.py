"""CPU tests of the connected tet components and the occupancy clean-up: the numpy restatement of
tests/tet_components_ref.py against hand cases and a plain-Python breadth-first search, the figures of the masks the GPU tests
use, the three symbols of the C ABI, the workspace size and the argument checks (all refused by name before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tet_components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SYMBOLS = ["deftet_tet_components_workspace_bytes", "deftet_tet_components_u8", "deftet_occupancy_cleanup_u8"]

_raw = ctypes.create_string_buffer(1 << 12)
P = ctypes.c_void_p((ctypes.addressof(_raw) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def grid16():
    return R.grid(16)


def got(inside, nbr):
    c = R.components(inside, np.asarray(nbr))
    return c["labels"].tolist(), c["sizes"].tolist(), c["open"].tolist(), c["count"]


# ---------------------------------------------------------------------------- the restatement
def test_hand_cases():
    one = [[-1, -1, -1, -1]]
    assert got([1], one) == ([0], [1], [1], 1)
    assert got([0], one) == ([-1], [0], [0], 0)
    two = [[1, -1, -1, -1], [-1, -1, 0, -1]]
    assert got([1, 1], two) == ([0, 0], [2, 0], [1, 0], 1)
    assert got([0, 1], two) == ([-1, 1], [0, 1], [0, 1], 1)
    assert got([1, 0], two) == ([0, -1], [1, 0], [1, 0], 1)
    assert got([0, 0], two) == ([-1, -1], [0, 0], [0, 0], 0)
    # the table is undirected: a link written in one row only still joins; an entry outside [0, T) is never followed
    assert got([1, 1], [[1, -1, -1, -1], [-1, -1, -1, -1]])[0] == [0, 0]
    assert got([1, 1], [[2, -1, -1, -1], [-7, -1, -1, -1]]) == ([0, 1], [1, 1], [1, 1], 2)
    # no -1 in any row of the component: closed
    ring = [[1, 2, 1, 2], [0, 2, 0, 2], [0, 1, 0, 1]]
    assert got([1, 1, 1], ring) == ([0, 0, 0], [3, 0, 0], [0, 0, 0], 1)


def test_cube_of_six_tets():
    tets, _V, nbr, _cen = R.grid(2)
    assert tets.shape == (6, 4) and (nbr >= 0).sum() == 12             # six Kuhn tets around the diagonal: a ring
    ring = {t: set(int(u) for u in nbr[t] if u >= 0) for t in range(6)}
    assert all(len(v) == 2 for v in ring.values())
    mask = np.zeros(6, bool)
    mask[[0, 3]] = True
    c = R.components(mask, nbr)
    if 3 in ring[0]:
        assert c["labels"].tolist() == [0, -1, -1, 0, -1, -1] and c["sizes"][0] == 2 and c["count"] == 1
    else:
        assert c["labels"].tolist() == [0, -1, -1, 3, -1, -1] and c["sizes"].tolist() == [1, 0, 0, 1, 0, 0] and c["count"] == 2
    assert c["open"][c["labels"][mask]].all()                           # every tet of one cube has faces on the boundary
    # the outside tets: 1, 2, 4, 5 in the pieces the ring leaves between 0 and 3
    o = R.components(~mask, nbr)
    assert o["count"] == (2 if 3 not in ring[0] else 1) and o["sizes"].sum() == 4
    assert R.cleanup(mask, nbr, keep_largest=True).tolist() == (R.components(mask, nbr)["labels"] == 0).tolist()
    assert not R.cleanup(mask, nbr, min_size=3).any()
    assert np.array_equal(R.cleanup(mask, nbr, fill_voids=True), mask)  # nothing is enclosed in one cube


@pytest.mark.parametrize("res,density,seed", [(4, 0.3, 1), (4, 0.5, 2), (6, 0.3, 3), (6, 0.5, 4), (6, 0.9, 5)])
def test_restatement_equals_breadth_first_search(res, density, seed):
    _tets, _V, nbr, _cen = R.grid(res)
    mask = R.random_mask(nbr.shape[0], density, seed)
    assert got(mask, nbr) == R.bfs_components(mask, nbr)
    # a one-sided table (every second row cleared) must give the same answer as the search on it
    half = nbr.copy()
    half[::2] = -1
    assert got(mask, half) == R.bfs_components(mask, half)


def test_selection_order_and_tie_rule():
    # a path 0-1-2-3-4-5-6 of tets, closed at both ends by a self-free table without -1: nothing reaches the boundary
    T = 9
    nbr = np.full((T, 4), -1, np.int64)
    for t in range(T - 1):
        nbr[t, 0] = t + 1
        nbr[t + 1, 1] = t
    mask = np.array([1, 1, 0, 1, 1, 0, 1, 0, 1], bool)                  # components {0,1} {3,4} {6} {8}
    assert R.cleanup(mask, nbr, keep_largest=True).tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]       # 2 = 2: the smaller label wins
    assert R.cleanup(mask, nbr, min_size=2).tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0]
    assert not R.cleanup(mask, nbr, min_size=3, keep_largest=True).any()
    assert not R.cleanup(np.zeros(T, bool), nbr, keep_largest=True).any()                         # an empty shape stays empty
    # outside {2} {5} {7}: every row of the path has a -1, so all are open and nothing is filled
    assert np.array_equal(R.cleanup(mask, nbr, fill_voids=True), mask)
    closed = np.where(nbr < 0, np.arange(T)[:, None], nbr)              # the -1 entries point at the row itself: no boundary at all
    closed[0, 2] = -1                                                   # ... but for tet 0
    filled = R.cleanup(mask, closed, fill_voids=True)
    assert filled.all()                                                 # {2} {5} {7} are enclosed: one component of nine
    assert R.cleanup(~mask, closed, fill_voids=True).tolist() == (~mask | np.array([0, 0, 0, 1, 1, 0, 1, 0, 1], bool)).tolist()
    # filling comes first: the filled path is one piece, so min_size = 9 keeps it and keep_largest has one candidate
    assert R.cleanup(mask, closed, fill_voids=True, min_size=9, keep_largest=True).all()


def test_figures_of_the_gpu_masks(grid16):
    """the sizes and counts the GPU file relies on, asserted on the reference side: a changed generator cannot hollow it out"""
    _tets, _V, nbr, cen = grid16
    T = nbr.shape[0]
    assert T == 3072
    m = R.shell(cen)
    c, o = R.components(m, nbr), R.components(~m, nbr)
    assert c["count"] == 1 and c["sizes"][c["labels"].max()] == 696
    assert sorted(zip(o["sizes"][o["sizes"] > 0].tolist(), o["open"][o["sizes"] > 0].tolist())) == [(108, 0), (2268, 1)]
    filled = R.cleanup(m, nbr, fill_voids=True)
    assert filled.sum() == 696 + 108 and filled[m].all()
    m = R.two_balls(cen)
    c = R.components(m, nbr)
    roots = np.nonzero(c["sizes"])[0]
    assert c["sizes"][roots].tolist() == [48, 48]
    assert np.array_equal(R.cleanup(m, nbr, keep_largest=True), c["labels"] == roots[0])
    assert not R.cleanup(m, nbr, min_size=49).any() and np.array_equal(R.cleanup(m, nbr, min_size=48), m)
    m = R.snake(16)
    assert m.sum() == 888 and R.components(m, nbr)["count"] == 1
    assert R.eccentricity(m, nbr, int(np.nonzero(m)[0][0])) == 399
    for k in range(6):
        c = R.components(R.every_sixth(T, k), nbr)
        assert c["count"] == 512 and c["sizes"].max() == 1
    assert R.components(R.random_mask(T, 0.3), nbr)["count"] == 444
    assert R.components(R.random_mask(T, 0.5), nbr)["count"] == 213


def test_permuted_numbering_carries_the_partition(grid16):
    tets, _V, nbr, cen = grid16
    for m in (R.shell(cen), R.snake(16), R.random_mask(tets.shape[0], 0.5)):
        tets_p, nbr_p, m_p, perm = R.permuted(tets, m, 7)
        want = R.labels_through(R.components(m, nbr)["labels"], perm)
        assert np.array_equal(R.components(m_p, nbr_p)["labels"], want)


# ---------------------------------------------------------------------------- the C ABI
def test_header_ctypes_table_and_library_agree_on_the_symbols(lib):
    from deftet_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deftet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", txt))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 350


def align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("B,T", [(1, 1), (1, 48), (3, 3072), (8, 257250)])
def test_workspace_is_the_total_of_the_layout(lib, B, T):
    """parent, accumulator and labels int32 [B,T], the filled mask uint8 [B,T], the winner uint64 [B], the count int32 [B]: each
    on its own 256-byte line"""
    size = lib.deftet_tet_components_workspace_bytes
    n = B * T
    want = 3 * align(4 * n) + align(n) + align(8 * B) + align(4 * B)
    assert size(B, T) == want and want % 256 == 0
    assert size(B, 2 * T + 256) > want and size(B + 1, T + 64) > want
    # both entry points carve with the same layout: one byte short is refused, the exact size passes on to the pointer checks
    comp, clean = lib.deftet_tet_components_u8, lib.deftet_occupancy_cleanup_u8
    assert comp(P, P, B, T, P, P, P, P, P, P, want - 1, None) == EINVAL and b"workspace" in lib.deftet_last_error()
    assert comp(P, P, B, T, None, P, P, P, P, P, want, None) == EINVAL and b"null pointer: labels" in lib.deftet_last_error()
    assert clean(P, P, B, T, 1, 0, 1, P, None, None, None, None, P, P, want - 1, None) == EINVAL and b"workspace" in lib.deftet_last_error()
    assert clean(P, P, B, T, 1, 0, 1, None, None, None, None, None, P, P, want, None) == EINVAL and b"null pointer: keep" in lib.deftet_last_error()


def test_bad_arguments_are_refused_by_name(lib):
    comp, clean = lib.deftet_tet_components_u8, lib.deftet_occupancy_cleanup_u8
    big = 1 << 30
    off = ctypes.c_void_p(P.value + 4)

    def both(inside=P, nbr=P, B=2, T=20, bad=P, ws=P, nbytes=big):
        rc = comp(inside, nbr, B, T, P, P, P, P, bad, ws, nbytes, None)
        msg = lib.deftet_last_error()
        assert b"tet_components:" in msg
        rc2 = clean(inside, nbr, B, T, 1, 0, 1, P, None, None, None, None, bad, ws, nbytes, None)
        msg2 = lib.deftet_last_error()
        assert b"occupancy_cleanup:" in msg2 and msg2.split(b": ", 1)[1] == msg.split(b": ", 1)[1]
        assert rc == rc2
        return rc, msg

    for kw, text in ((dict(B=0), b"n_batch=0"), (dict(B=-3), b"n_batch=-3"), (dict(B=65536), b"n_batch=65536"),
                     (dict(T=0), b"n_tet=0"), (dict(T=-1), b"n_tet=-1"), (dict(B=60000, T=60000), b"31 bits"),
                     (dict(inside=None), b"null pointer: inside_bxt"), (dict(nbr=None), b"nbr32_tx4"), (dict(nbr=off), b"misaligned pointer: nbr32_tx4"),
                     (dict(bad=None), b"null pointer: bad"), (dict(ws=None), b"workspace null"),
                     (dict(ws=ctypes.c_void_p(P.value + 16)), b"misaligned"),
                     (dict(nbytes=lib.deftet_tet_components_workspace_bytes(2, 20) - 1), b"too small: need %d bytes" % lib.deftet_tet_components_workspace_bytes(2, 20))):
        rc, msg = both(**kw)
        assert rc == EINVAL and text in msg, (kw, msg)
    for k in range(4):                                                  # each of the four outputs by itself
        outs = [P, P, P, P]
        outs[k] = None
        assert comp(P, P, 2, 20, *outs, P, P, big, None) == EINVAL and b"labels / sizes / open / count" in lib.deftet_last_error()
        assert clean(P, P, 2, 20, 0, 0, 0, P, *outs, P, P, big, None) == EINVAL and b"go together" in lib.deftet_last_error()
    assert clean(P, P, 2, 20, 0, -1, 0, P, None, None, None, None, P, P, big, None) == EINVAL and b"min_size=-1" in lib.deftet_last_error()
    assert lib.deftet_tet_components_workspace_bytes(0, 20) == 256 and lib.deftet_tet_components_workspace_bytes(2, -1) == 256


def test_front_end_refuses_cpu_tensors_and_foreign_tables():
    from deftet_amd import _lib, hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    t32 = torch.full((5, 4), -1, dtype=torch.int32)
    nbr = hip_ops.TetFaceNeighbours(t32.long(), t32)
    for call in (lambda: hip_ops.tet_components(torch.ones(1, 5, dtype=torch.bool), nbr),
                 lambda: hip_ops.occupancy_cleanup(torch.ones(5), nbr, keep_largest=True),
                 lambda: DefTet.clean_occupancy(None, torch.ones(1, 5), nbr)):
        with pytest.raises(_lib.DefTetHipError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        hip_ops.tet_components(torch.ones(1, 5), t32)
    assert hip_ops.TetComponents._fields == ("labels", "sizes", "open", "count")
    import inspect
    from deftet_amd.render import export
    sig = inspect.signature(export.save_surface_objs).parameters
    assert [sig[k].default for k in ("keep_largest", "min_component", "fill_voids")] == [False, 0, False]
    sig = inspect.signature(DefTet.clean_occupancy).parameters
    assert [sig[k].default for k in ("thres", "keep_largest", "min_size", "fill_voids")] == [0.5, True, 0, False]
