"""The two-level query sort (k_slab_local / k_slab_sort) seen through what it feeds: with the grid box measured by the call,
handed in as a hint and tracked from call to call, the binned query returns the brute-force index on EVERY query, and the
backward that walks the sorted structure is reproducible bit for bit.  Sizes: BASELINE configs[1] and configs[2], and sets that
hit the sort's edges (queries outside the hint, NaN / Inf, one cell, a ragged last chunk, fewer queries than a workgroup).
The sorted structure itself is read back from a prepared workspace (deftet_debug_point_in_tet_layout) and checked against cells
worked out on the CPU: every query index once, every binned query inside the run the cell-start table gives its cell."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu


def _check(tet, pts, dev, hint=None):
    from deftet_amd import hip_ops
    t = torch.from_numpy(np.ascontiguousarray(tet)).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    B, Q = p.shape[0], p.shape[1]
    assert hip_ops.bwd_uses_records(t.shape[1], Q)            # the atomic-free backward: the one that is reproducible bit for bit
    want = hip_ops.point_in_tet(t, p, algo=hip_ops.PIT_BRUTE)
    hip_ops.clear_query_box_cache()
    boxes = [None, "track", "track", "track"]                 # measured; tracked: the first call measures, the next two take the hint
    if hint is not None:
        boxes.append(torch.from_numpy(np.ascontiguousarray(hint, np.float32)).to(dev))
    gen = torch.Generator(device=dev).manual_seed(11)
    gw = torch.randn(B, Q, 4, device=dev, generator=gen)
    go = torch.randn(B, Q, device=dev, generator=gen)
    for box in boxes:
        cond, w, hits = hip_ops.point_in_tet(t, p, want_bary=True, want_hits=True, query_box=box)
        same = torch.equal(cond, want)
        if not same:
            bad = (cond != want).nonzero()
            print("query_box=%r: %d of %d queries differ from brute force, first %s" % (
                box if not torch.is_tensor(box) else "hint", bad.shape[0], B * Q, bad[:4].tolist()))
        assert same
        g1 = hip_ops.point_in_tet_bwd(t, p, cond, gw, grad_occ=go, hits=hits)
        g2 = hip_ops.point_in_tet_bwd(t, p, cond, gw, grad_occ=go, hits=hits)
        for a, b in ((g1[0], g2[0]), (g1[2], g2[2])):                             # g_tet, g_pred: bit-equal runs (as bits: an Inf
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))            # query that hits leaves NaN gradients, the same ones)
        assert torch.isfinite(g1[2]).all()
    if B * Q > 0:
        tr = [v for k, v in hip_ops.query_box_trackers().items() if k[2] == B and k[3] == Q]
        assert tr and tr[0]["tracked"] >= 1                    # the hint path did run


def _check_structure(n_tet, pts, dev, box):
    """sortedQ / cell-start table / unbinned list of one prepare call against cells computed here"""
    from deftet_amd import _lib, hip_ops
    lib = _lib.load()
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    B, Q = p.shape[0], p.shape[1]
    lay = (ctypes.c_longlong * 8)()
    fn = lib.deftet_debug_point_in_tet_layout
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    _lib.check(fn(B, n_tet, Q, hip_ops.PIT_AUTO, lay), "deftet_debug_point_in_tet_layout")
    G, Gx, stride, o_gp, o_tab, o_sq, o_cnt, o_irr = [int(v) for v in lay]
    assert (G, Gx) == hip_ops.point_in_tet_grid(n_tet, Q)
    pq = hip_ops.prepare_queries(p, n_tet, query_box=box)
    torch.cuda.synchronize()
    ws = pq.workspace.cpu().numpy()

    def rd(off, n, dt):
        return ws[off:off + n * 4].view(dt)
    gp = rd(o_gp, B * 20, np.float32).reshape(B, 20)
    table = rd(o_tab, B * stride, np.int32).reshape(B, stride)
    sq = rd(o_sq, B * Q * 4, np.float32).reshape(B, Q, 4)
    cnt = rd(o_cnt, B * 4, np.int32).reshape(B, 4)
    irr = rd(o_irr, B * Q, np.int32).reshape(B, Q)
    Gp = G + 3
    for b in range(B):
        n_irr = int(cnt[b, 1])
        n_reg = Q - n_irr
        assert 0 <= n_irr <= Q
        idx = sq[b, :n_reg, 3].copy().view(np.int32)
        assert np.array_equal(np.sort(np.concatenate([idx, irr[b, :n_irr]])), np.arange(Q))      # every query exactly once
        xyz = sq[b, :n_reg, :3]
        assert np.array_equal(xyz.view(np.int32), pts[b, idx].view(np.int32))                      # the record carries its query
        o, inv = gp[b, 0:3], gp[b, 3:6]
        with np.errstate(invalid="ignore", over="ignore"):
            c = [np.clip((xyz[:, k] - o[k]) * inv[k], np.float32(0), np.float32(n - 1)).astype(np.int32)   # cell_of, in float32
                 for k, n in ((0, Gx), (1, G), (2, G))]
        at = (c[2] * (Gx + 1) + c[0]) * Gp + c[1]
        start, end = table[b, at], table[b, at + Gp]                                               # (cz, cx + 1, cy): where the next cell starts
        pos = np.arange(n_reg)
        bad = ~((start <= pos) & (pos < end))
        assert not bad.any(), "shape %d: %d of %d sorted queries lie outside their cell's run, first at %s" % (
            b, bad.sum(), n_reg, np.nonzero(bad)[0][:4])
        # unbinned queries: irregular, or outside the grid box of this call
        q = pts[b, irr[b, :n_irr]]
        lo, hi = gp[b, 6:9], gp[b, 9:12]
        with np.errstate(invalid="ignore"):
            inside = np.all(np.isfinite(q) & (np.abs(q) <= 2.0 ** 20) & (q >= lo) & (q <= hi), axis=1)
        assert not inside.any()


@pytest.mark.parametrize("res,nq", [(40, 50_000), (70, 100_000)])
def test_sorted_structure_baseline_configs(cuda, res, nq):
    tet, pts = cases.jittered(res, nq, 8)
    lo, hi = pts.min(1), pts.max(1)
    _check_structure(tet.shape[1], pts, cuda, None)
    _check_structure(tet.shape[1], pts, cuda, torch.from_numpy(np.concatenate([lo, hi], 1)).to(cuda))


@pytest.mark.parametrize("res,nq", [(40, 50_000), (70, 100_000)])
def test_sorted_queries_answer_as_brute_force_baseline_configs(cuda, res, nq):
    tet, pts = cases.jittered(res, nq, 8)
    _check(tet, pts, cuda)


def _edge_sets():
    tet, pts = cases.jittered(16, 5000, 2)          # 3,072 tets: every set below stays within 2 queries per tet (see _check)
    lo, hi = pts.min(1), pts.max(1)
    full = np.concatenate([lo, hi], 1)
    out = {}
    # hint box covering the middle half of the queries' extent: a quarter of them or more lie outside it
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    out["outside_hint"] = (tet, pts, np.concatenate([mid - half, mid + half], 1))
    p = pts.copy()
    p[:, 5::97, 0] = np.nan
    p[:, 7::101, 1] = np.inf
    p[:, 11::103, 2] = -np.inf
    p[:, 13::107, :] = 3.0e30
    out["nan_inf"] = (tet, p, full)
    p = np.repeat(pts[:, :1, :], 4099, 1) + (1e-4 * np.random.default_rng(5).standard_normal((2, 4099, 3))).astype(np.float32)
    out["one_cell"] = (tet, p, full)
    out["ragged_chunk"] = (tet, np.ascontiguousarray(pts[:, :2048 + 257]), full)        # not a multiple of the chunk, of 256 or of 64
    out["below_256"] = (tet, np.ascontiguousarray(pts[:, :201]), full)
    return out


@pytest.mark.parametrize("name", ["outside_hint", "nan_inf", "one_cell", "ragged_chunk", "below_256"])
def test_sorted_queries_answer_as_brute_force_edges(cuda, name):
    tet, pts, hint = _edge_sets()[name]
    _check(tet, pts, cuda, hint)


@pytest.mark.parametrize("name", ["outside_hint", "nan_inf", "one_cell", "ragged_chunk", "below_256"])
def test_sorted_structure_edges(cuda, name):
    tet, pts, hint = _edge_sets()[name]
    _check_structure(tet.shape[1], pts, cuda, None)
    _check_structure(tet.shape[1], pts, cuda, torch.from_numpy(np.ascontiguousarray(hint, np.float32)).to(cuda))
