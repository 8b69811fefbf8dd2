"""The surface operators (deftet_amd/csrc/{nearest_neighbor,chamfer,face_adjacency,tri_distance}.hip) past the switches that a size or a batch count selects and that
BASELINE (8 shapes, 4,056 faces, n_max_nei = 30) never reaches:

  A10 / A9   more than kBatchShapes = 8 shapes: the second and later launch groups reuse one workspace in stream order,
             with their pointers rebased by the group's first shape; a last group of 1 or 3 shapes; an all-empty group
  A9         more than 131,072 faces: the far path without its de-duplication bitset
  A8         more than kA8Shapes = 32 shapes, an all-empty group, table widths 1..32 on the hash path and > 32 on the scan
  normal     more than kNCLdsFaces = 4,096 faces (row walk, normals read back from global memory), both paths in one
             launch; cut / invalid / empty tables; zero-area faces
  chamfer    9 shapes (A10's second group through the loss), against an fp64 reference, with a sample on a cloud point

Index outputs are held bit for bit against the CPU oracle, the streaming-scan kernels and the per-shape calls; float
outputs against the fp64 references of tests/surface_ref.py.  Every branch is reached by its inputs alone."""
import numpy as np
import pytest
import torch

from tests import surface_ref as R
from tests import tol

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ------------------------------------------------------------------------------------------------ A10 across shape groups
NN_M, NN_N = 2000, 600


def _nn_case(B, oracle):
    """B clouds of 2,000 points, each with its own seed, centre and scale (a search in another shape's cloud gives other
    indices) and 20 exact duplicates; 600 queries per shape: a third inside the cloud's box, a third uniform(-5, 5) (far
    path), the rest zero-distance copies of points (of the duplicated ones too: the lower index wins)."""
    def make():
        p = np.empty((B, NN_M, 3), np.float32)
        q = np.empty((B, NN_N, 3), np.float32)
        third = NN_N // 3
        for b in range(B):
            rng = np.random.default_rng(1000 + b)
            centre, scale = rng.uniform(-1, 1, 3), 0.3 + 0.15 * (b % 5)
            p[b] = centre + scale * rng.uniform(-0.5, 0.5, (NN_M, 3))
            p[b, 500:520] = p[b, 100:120]
            q[b, :third] = centre + scale * rng.uniform(-0.5, 0.5, (third, 3))
            q[b, third:2 * third] = rng.uniform(-5, 5, (third, 3))
            pick = rng.integers(0, NN_M, NN_N - 2 * third)
            pick[:20] = np.arange(500, 520)
            q[b, 2 * third:] = p[b, pick]
        want = oracle.nn_index(q, p)
        assert (want[:, 2 * third:2 * third + 20] == np.arange(100, 120)).all()
        assert not np.array_equal(oracle.nn_index(q[B - 1:], p[:1]), want[B - 1:])     # the wrong cloud answers differently
        return q, p, want
    return _cached(("nn", B), make)


@pytest.mark.parametrize("B", [9, 11, 17])
def test_nn_index_across_shape_groups(cuda, oracle, B):
    """One or two full groups of 8 shapes, then a last group of 1, 3 and 1 shapes (0 and 2 shape bits on the far keys):
    == the oracle == the streaming scan == the per-shape calls, bit for bit; a second call on the reused workspace too."""
    from deftet_amd import hip_ops
    q, p, want = _nn_case(B, oracle)
    tq, tp = _dev(q, cuda), _dev(p, cuda)
    got = hip_ops.nn_index(tq, tp)
    assert got.dtype == torch.int32 and got.shape == (B, NN_N)
    bad = np.nonzero((got.cpu().numpy() != want).any(1))[0]
    assert bad.size == 0, "shapes that differ from the oracle: %s" % bad.tolist()
    assert np.array_equal(hip_ops.nn_index(tq, tp, brute=True).cpu().numpy(), want)
    for b in range(B):
        one = hip_ops.nn_index(tq[b:b + 1].contiguous(), tp[b:b + 1].contiguous())
        assert torch.equal(one[0], got[b]), b
    assert torch.equal(hip_ops.nn_index(tq, tp), got)                                  # same stream, same workspace


def test_nn_index_ragged_with_an_empty_group(cuda, oracle):
    """17 shapes whose second group has no query at all (skipped), then a group of one shape with half its queries."""
    from deftet_amd import hip_ops
    B = 17
    q, p, want = _nn_case(B, oracle)
    tq, tp = _dev(q, cuda), _dev(p, cuda)
    counts = [NN_N] * 8 + [0] * 8 + [NN_N // 2]
    for brute in (False, True):
        got = hip_ops.nn_index_ragged(tq, tp, counts, brute=brute).cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b, :counts[b]], want[b, :counts[b]]), (brute, b)
            assert (got[b, counts[b]:] == 0).all(), (brute, b)
    again = hip_ops.nn_index_ragged(tq, tp, counts).cpu().numpy()
    assert np.array_equal(again, got)
    # other counts on the same workspace right after: nothing of the previous call's groups may survive
    counts2 = [0] * 8 + [NN_N - 1, 1, 0, 7, NN_N, 64, 65, 0] + [NN_N]
    got2 = hip_ops.nn_index_ragged(tq, tp, counts2).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got2[b, :counts2[b]], want[b, :counts2[b]]), b
        assert (got2[b, counts2[b]:] == 0).all(), b


# ------------------------------------------------------------------------------------------------- A9 across shape groups
A9_P = 1500


def _points_about(tri, P, rng, far_scale=2.5, noise=0.02):
    """P points: the even ones near the surface (on a random face, moved by `noise` extents), the odd ones the same kind
    of point scaled by far_scale about the surface's centre (nothing is settled by the near shells: the far path)."""
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    centre, ext = 0.5 * (lo + hi), float((hi - lo).max())
    w = rng.dirichlet([1, 1, 1], P)
    pts = (tri[rng.integers(0, tri.shape[0], P)] * w[:, :, None]).sum(1) + rng.normal(0, noise * ext, (P, 3))
    pts[1::2] = centre + far_scale * (pts[1::2] - centre)
    return pts.astype(np.float32)


def _a9_case(B, oracle):
    def make():
        rng = np.random.default_rng(90 + B)
        empty = 2 if B == 9 else 10                                  # the empty surface: in the first / the second group
        shapes, pts = [], np.empty((B, A9_P, 3), np.float32)
        for b in range(B):
            n = 60 + (b * 53) % 341                                  # 60..400 faces, all different for B <= 17
            full = R.sheet(14, 15, 200 + b) * np.float32(0.5 + 0.1 * (b % 4)) + rng.uniform(-0.5, 0.5, 3).astype(np.float32)
            pts[b] = _points_about(full[:n], A9_P, rng)
            shapes.append(full[:0] if b == empty else full[:n])
        face, counts = R.pad_shapes(shapes)
        assert counts[empty] == 0 and len(set(counts)) == B and 60 <= min(c for c in counts if c) and max(counts) <= 400
        nfb = np.array(counts, np.float32)
        wd, wf = oracle.tri_dist_fwd(pts, face, nfb)
        return pts, face, nfb, wd, wf, empty
    return _cached(("a9", B), make)


@pytest.mark.parametrize("B", [9, 17])
def test_tri_dist_across_shape_groups(cuda, oracle, B):
    from deftet_amd import hip_ops
    pts, face, nfb, wd, wf, empty = _a9_case(B, oracle)
    tp, tf, tn = _dev(pts, cuda), _dev(face, cuda), _dev(nfb, cuda)
    d, f, order = hip_ops.tri_dist_fwd(tp, tf, tn, want_order=True)
    for name, got, want in (("f", f, wf), ("d", d, wd)):
        bad = np.nonzero((got.cpu().numpy() != want).any((1, 2)))[0]
        assert bad.size == 0, "closest_%s differs from the oracle in shapes %s" % (name, bad.tolist())
    assert (f[empty] == -1).all() and (d[empty] == 10000).all()
    db, fb = hip_ops.tri_dist_fwd(tp, tf, tn, brute=True)
    assert torch.equal(fb, f) and torch.equal(db, d)
    for b in range(B):
        d1, f1 = hip_ops.tri_dist_fwd(tp[b:b + 1].contiguous(), tf[b:b + 1].contiguous(), tn[b:b + 1].contiguous())
        assert torch.equal(f1[0], f[b]) and torch.equal(d1[0], d[b]), b
    # the point order of every shape, the last group's included, is a permutation
    assert order is not None and order.dtype == torch.int32 and order.shape == (B, A9_P)
    srt = torch.sort(order.long(), dim=1).values
    bad = (srt != torch.arange(A9_P, device=cuda)[None]).any(1).nonzero().flatten().tolist()
    assert not bad, "order is no permutation for shapes %s" % bad
    # the grouped backward walks that order
    g = torch.rand(d.shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(B))
    s = hip_ops.tri_dist_bwd(tp, tf, f, g, deterministic=True)
    o = hip_ops.tri_dist_bwd(tp, tf, f, g, order=order)
    assert s.abs().max().item() > 0 and (s[empty] == 0).all() and (o[empty] == 0).all()
    tol.check_close("tri_dist_bwd order vs sorted, B=%d" % B, o, s, 2e-5)
    for b in (0, B - 1):                                              # per shape as well: the scale of one shape cannot hide another
        tol.check_close("tri_dist_bwd order vs sorted, B=%d shape %d" % (B, b), o[b], s[b], 2e-5)


# ------------------------------------------------------------------------------- A9 beyond the de-duplication bitset
@pytest.mark.parametrize("F", [131072, 131073])
def test_tri_dist_far_path_at_the_bitset_limit(cuda, oracle, F):
    """131,072 faces fill the far path's LDS bitset to its last bit; with one more it is not used and duplicates are
    evaluated again.  Half the points are far (scale 2.5).  grid == streaming scan; == the oracle on 256 points."""
    from deftet_amd import hip_ops
    full = _cached("bigsheet", lambda: R.sheet(256, 257, 31))
    face = full[:F][None]
    pts = _cached("bigpts", lambda: _points_about(full, 2048, np.random.default_rng(32), noise=0.005))[None]
    tp, tf = _dev(pts, cuda), _dev(face, cuda)
    tn = torch.tensor([float(F)], device=cuda)
    d, f = hip_ops.tri_dist_fwd(tp, tf, tn)
    db, fb = hip_ops.tri_dist_fwd(tp, tf, tn, brute=True)
    assert torch.equal(f, fb)
    assert torch.equal(d, db)
    assert (f >= 0).all() and (f < F).all()
    wd, wf = oracle.tri_dist_fwd(pts[:, :256], face, np.array([F], np.float32))
    assert np.array_equal(f[:, :256].cpu().numpy(), wf) and np.array_equal(d[:, :256].cpu().numpy(), wd)


# ------------------------------------------------------------------------------ A8 across shape groups and table widths
def _a8_case(B):
    def make():
        shapes = []
        for b in range(B):
            n = 20 + (b * 41) % 281                                  # 20..300 faces
            t = R.sheet(12, 13, 300 + b, n=n)
            if b in (5, B - 1):                                      # every face twice: rows fill up, ties by index
                t = np.concatenate([t[:n // 2], t[:n - n // 2]], 0)
            if B == 65 and 32 <= b < 64:
                t = t[:0]                                            # the whole second group is empty
            shapes.append(t)
        face, counts = R.pad_shapes(shapes, 300)
        assert min(c for c in counts if c) >= 20 and max(counts) <= 300 and counts[32] != counts[0]
        return face, counts
    return _cached(("a8", B), make)


@pytest.mark.parametrize("max_nei", [1, 2, 3, 30, 32, 33, 40])
@pytest.mark.parametrize("B", [33, 65])
def test_face_edge_adj_across_shape_groups_and_widths(cuda, oracle, B, max_nei):
    """Two and three groups of 32 shapes (the last one holds a single shape), on the hash path for widths <= 32 and on
    the O(F^2) scan above: every shape == the oracle == the single-shape call == brute."""
    from deftet_amd import hip_ops
    face, counts = _a8_case(B)
    tf = _dev(face, cuda)
    adj = hip_ops.face_edge_adj_ragged(tf, counts, max_nei)
    assert adj.shape == (B, 300, max_nei) and adj.dtype == torch.float32
    assert torch.equal(hip_ops.face_edge_adj_ragged(tf, counts, max_nei, brute=True), adj)
    got = adj.cpu().numpy()
    for b in range(B):
        n = counts[b]
        assert (got[b, n:] == -1).all(), b
        if n == 0:
            continue
        want = _cached(("a8want", B, b, max_nei), lambda: oracle.face_edge_adj(face[b, :n], max_nei))
        assert np.array_equal(got[b, :n], want), b
        assert np.array_equal(hip_ops.face_edge_adj(tf[b, :n].contiguous(), max_nei).cpu().numpy(), want), b
    if max_nei <= 3:                                                  # twin + doubled neighbours: narrow rows are cut
        assert ((got[5, :counts[5]] >= 0).sum(1) == max_nei).mean() > 0.9


# ------------------------------------------------------------------------ normal consistency at its switch and its edges
NC_RTOL_LOSS, NC_ATOL_LOSS, NC_RTOL_GRAD, NC_ATOL_GRAD = 1e-5, 1e-7, 2e-4, 1e-6


def _hold_normal_consistency(name, tri_np, tab, n_face, w, cuda, mask=None):
    """Runs the operator and the fp64 reference on the same table, asserts the operator's own tolerances (loss rtol 1e-5,
    atol 1e-7; gradient rtol 2e-4, atol 1e-6 of the largest reference entry) and records the measured max-norm errors
    through tol.check_close (its bounds are the ones those tolerances imply).  mask (bool [B,F]): the gradient is compared
    separately on the masked rows and on the others, each against its own largest entry.  Returns loss, grad, grad64."""
    from deftet_amd import hip_ops
    tri = _dev(tri_np, cuda).requires_grad_(True)
    nf = torch.tensor(n_face, device=cuda, dtype=torch.int32)
    wt = torch.tensor(w, device=cuda)
    loss = hip_ops.normal_consistency(tri, tab, nf)
    (loss * wt).sum().backward()
    t64 = tri.detach().double().requires_grad_(True)
    want = R.normal_consistency64(t64, tab, n_face)
    (want * wt.double()).sum().backward()
    assert torch.isfinite(loss).all() and torch.isfinite(tri.grad).all()
    scale = want.abs().max().item()
    tol.check_close(name + " loss", loss, want, NC_RTOL_LOSS + (NC_ATOL_LOSS / scale if scale > 0 else 0.0))
    assert torch.allclose(loss.double(), want, rtol=NC_RTOL_LOSS, atol=NC_ATOL_LOSS), (name, loss, want)
    parts = [("", None)] if mask is None else [(" masked rows", mask), (" other rows", ~mask)]
    for tag, m in parts:
        mm = None if m is None else m[:, :, None, None].expand_as(t64.grad)
        g, g64 = (tri.grad, t64.grad) if mm is None else (tri.grad[mm], t64.grad[mm])
        tol.check_close(name + " grad" + tag, tri.grad, t64.grad, NC_RTOL_GRAD + NC_ATOL_GRAD, mask=mm)
        assert torch.allclose(g.double(), g64, rtol=NC_RTOL_GRAD, atol=NC_ATOL_GRAD * g64.abs().max().item()), name + tag
    return loss.detach(), tri.grad.detach(), t64.grad.detach()


def test_normal_consistency_both_paths_in_one_launch(cuda):
    """n_face = [4096, 4097, 0, 5000, 300]: the LDS path (<= 4,096 faces), the row walk right above it and well above it,
    an empty shape and a small one, in one launch."""
    from deftet_amd import hip_ops
    shapes = [R.sheet(64, 33, 41, n=4096), R.sheet(64, 33, 42, n=4097), R.sheet(2, 2, 43, n=0), R.sheet(50, 50, 44), R.sheet(12, 13, 45, n=300)]
    tri_np, counts = R.pad_shapes(shapes, 5000)
    assert counts == [4096, 4097, 0, 5000, 300]
    tab = hip_ops.face_edge_adj_ragged(_dev(tri_np, cuda), counts, 30)
    loss, grad, _ = _hold_normal_consistency("normal consistency 4096/4097/0/5000/300", tri_np, tab, counts, [0.7, 1.3, -0.4, 0.9, -1.1], cuda)
    assert loss[2] == 0 and (grad[2] == 0).all()
    assert (loss[[0, 1, 3, 4]] > 1e-3).all()
    for b, n in enumerate(counts):
        assert (grad[b, n:] == 0).all(), b


def test_normal_consistency_same_surface_on_both_paths(cuda):
    """The same 4,096 faces once alone (LDS path) and once with an isolated far-away triangle appended (4,097 faces: row
    walk; the same table plus an all -1 row): both == fp64, and they agree with each other within twice the bound."""
    from deftet_amd import hip_ops
    base = R.sheet(64, 33, 41, n=4096)
    far = (base[:1] + np.float32(40.0)).astype(np.float32)
    tab = hip_ops.face_edge_adj(_dev(base, cuda), 30)
    tab1 = torch.cat([tab, torch.full((1, 30), -1.0, device=cuda)], 0)
    assert torch.equal(hip_ops.face_edge_adj(_dev(np.concatenate([base, far], 0), cuda), 30), tab1)   # it IS isolated
    l0, g0, g64 = _hold_normal_consistency("normal consistency 4096 (LDS)", base[None], tab[None], [4096], [1.0], cuda)
    l1, g1, _ = _hold_normal_consistency("normal consistency 4096+1 (row walk)", np.concatenate([base, far], 0)[None], tab1[None], [4097], [1.0],
                                         cuda)
    assert abs(l0.item() - l1.item()) <= 2 * (NC_ATOL_LOSS + NC_RTOL_LOSS * abs(l0.item()))
    assert (g1[0, 4096] == 0).all()
    bound = 2 * (NC_ATOL_GRAD * g64.abs().max().item() + NC_RTOL_GRAD * g64.abs())
    assert ((g0.double() - g1[:, :4096].double()).abs() <= bound).all()


@pytest.mark.parametrize("max_nei", [2, 3, 33])
def test_normal_consistency_table_widths(cuda, max_nei):
    """At width 2 the rows are cut and the table is asymmetric (i lists j, j does not list i); 33 is wider than any row."""
    from deftet_amd import hip_ops
    tri_np = R.sheet(12, 13, 46, n=300)
    tab = hip_ops.face_edge_adj(_dev(tri_np, cuda), max_nei)
    t = tab.cpu().numpy().astype(np.int64)
    pairs = {(i, j) for i in range(300) for j in t[i] if j >= 0}
    asym = sum((j, i) not in pairs for i, j in pairs)
    assert (asym > 0) == (max_nei == 2)
    _hold_normal_consistency("normal consistency max_nei=%d" % max_nei, tri_np[None], tab[None], [300], [1.0], cuda)


def test_normal_consistency_bad_table_entries(cuda):
    """NaN, F, 1e9 and -7 count as "no neighbour"; 2.5 is neighbour 2 — in valid and in padding slots."""
    from deftet_amd import hip_ops
    tri_np = R.sheet(12, 13, 47, n=300)
    tab = hip_ops.face_edge_adj(_dev(tri_np, cuda), 30).clone()
    bad = {(5, 0): float("nan"), (6, 1): 300.0, (7, 0): 1e9, (8, 0): -7.0, (9, 1): 2.5, (10, 7): float("nan"), (11, 8): 300.0,
           (12, 9): 1e9, (13, 29): -7.0, (14, 29): 2.5, (299, 0): 2.5, (0, 0): float("inf")}
    was_valid = [bool(tab[f, k] >= 0) for f, k in bad]
    assert any(was_valid) and not all(was_valid)                      # neighbours are overwritten, and padding slots
    for (f, k), v in bad.items():
        tab[f, k] = v
    _hold_normal_consistency("normal consistency bad entries", tri_np[None], tab[None], [300], [1.0], cuda)


def test_normal_consistency_zero_area_faces(cuda):
    """Ten faces with a repeated vertex (the cross product is exactly 0 in fp32 and fp64 alike), each a neighbour of
    ordinary faces: normal 0 by the guard, gradient rows of order 1e6; compared separately from the ordinary rows."""
    from deftet_amd import hip_ops
    tri_np = R.sheet(12, 13, 48, n=300).copy()
    deg = np.arange(30, 130, 10)
    tri_np[deg, 2] = tri_np[deg, 1]
    c = np.cross(tri_np[:, 1] - tri_np[:, 0], tri_np[:, 2] - tri_np[:, 0])
    assert (c[deg] == 0).all() and (np.abs(np.delete(c, deg, 0)).max(1) > 0).all()
    tab = hip_ops.face_edge_adj(_dev(tri_np, cuda), 30)
    t = tab.cpu().numpy()
    assert ((t[deg] >= 0).sum(1) >= 1).all() and not np.isin(t[deg], deg).any()     # neighbours of ordinary faces only
    mask = torch.zeros(1, 300, dtype=torch.bool, device=cuda)
    mask[0, torch.from_numpy(deg).to(cuda)] = True
    _, grad, g64 = _hold_normal_consistency("normal consistency zero-area", tri_np[None], tab[None], [300], [1.0], cuda, mask=mask)
    assert g64[mask].abs().max().item() > 1e3 * g64[~mask].abs().max().item()        # the guard's 1e6


def test_normal_consistency_without_any_neighbour(cuda):
    from deftet_amd import hip_ops
    tri_np, counts = R.pad_shapes([R.sheet(5, 5, 49), R.sheet(12, 13, 50, n=300)], 300)
    tab = torch.full((2, 300, 30), -1.0, device=cuda)
    tab[1] = hip_ops.face_edge_adj(_dev(tri_np[1], cuda), 30)
    loss, grad, _ = _hold_normal_consistency("normal consistency no neighbour", tri_np, tab, counts, [1.5, 0.5], cuda)
    assert counts[0] == 50 and loss[0].item() == 0.0 and (grad[0] == 0).all() and loss[1].item() > 0


# ---------------------------------------------------------------------------------------------------------- chamfer term
CH_B, CH_M = 9, 1500
CH_COUNTS = [200, 57, 0, 123, 40, 199, 88, 150, 64]                  # 40..200 faces, one empty shape


def _chamfer_inputs(K, counts, seed):
    rng = np.random.default_rng(seed)
    B, F = len(counts), max(counts)
    shapes = [R.sheet(10, 10, 500 + b, n=counts[b]) * np.float32(0.6 + 0.05 * b) + rng.uniform(-0.3, 0.3, 3).astype(np.float32)
              for b in range(B)]
    tri, _ = R.pad_shapes(shapes, F)
    gt = np.empty((B, CH_M, 3), np.float32)
    for b in range(B):
        full = R.sheet(10, 10, 500 + b) * np.float32(0.6 + 0.05 * b)
        gt[b] = _points_about(full, CH_M, rng, far_scale=1.0, noise=0.05) + (shapes[b][0, 0] - full[0, 0] if counts[b] else 0)
    uv = rng.random((2, B, F, K)).astype(np.float32)
    return tri, gt, uv


def _samples32(tri, uv):
    """The sample placement of the operator in fp32 torch ops, operation by operation: (wa a + wb b) + wc c."""
    s, r1 = torch.sqrt(uv[0]), uv[1]
    wa, wb, wc = (1.0 - s)[..., None], (s * (1.0 - r1))[..., None], (s * r1)[..., None]
    smp = (wa * tri[:, :, None, 0] + wb * tri[:, :, None, 1]) + wc * tri[:, :, None, 2]
    return smp.reshape(tri.shape[0], -1, 3)


@pytest.mark.parametrize("K", [1, 7])
def test_chamfer_to_cloud_vs_fp64_across_shape_groups(cuda, K):
    """9 shapes: the nearest-neighbour search inside the loss runs a second group.  Value and gradient against the fp64
    expression on the operator's own indices, at the bounds the fp32 composition test asserts (value rtol 2e-6, atol 1e-6;
    gradient 2e-5 of its largest entry).  One sample sits on a cloud point (r0 = 0: corner a, which is in the cloud)."""
    from deftet_amd import hip_ops
    tri_np, gt_np, uv_np = _chamfer_inputs(K, CH_COUNTS, 60 + K)
    uv_np[0, 1, 3, 0] = 0.0                                          # shape 1, face 3, sample 0 = corner a ...
    gt_np[1, 700] = tri_np[1, 3, 0]                                  # ... which is cloud point 700
    tri = _dev(tri_np, cuda).requires_grad_(True)
    gt, uv = _dev(gt_np, cuda), _dev(uv_np, cuda)
    w = torch.linspace(0.5, 1.5, CH_B, device=cuda)
    out = hip_ops.chamfer_to_cloud(tri, gt, CH_COUNTS, K, uv=uv)
    (out * w).sum().backward()
    smp = _samples32(tri.detach(), uv)
    idx = hip_ops.nn_index_ragged(smp, gt, [c * K for c in CH_COUNTS])
    assert idx[1, 3 * K].item() == 700 and torch.equal(smp[1, 3 * K], gt[1, 700])
    t64 = tri.detach().double().requires_grad_(True)
    want = R.chamfer64(t64, gt, idx, uv, CH_COUNTS, K)
    (want * w.double()).sum().backward()
    assert torch.isfinite(out).all() and torch.isfinite(tri.grad).all()
    scale = want.abs().max().item()
    tol.check_close("chamfer_to_cloud value vs fp64, K=%d" % K, out, want, 2e-6 + 1e-6 / scale)
    assert torch.allclose(out.double(), want, rtol=2e-6, atol=1e-6), (out, want)
    assert out[2].item() == 0.0 and torch.equal(tri.grad[2], torch.zeros_like(tri.grad[2]))
    tol.check_close("chamfer_to_cloud grad vs fp64, K=%d" % K, tri.grad, t64.grad, 2e-5)
    for b, n in enumerate(CH_COUNTS):
        assert (tri.grad[b, n:] == 0).all(), b
    if K == 1:                                                        # the coinciding sample is face 3's only one
        assert torch.equal(tri.grad[1, 3], torch.zeros(3, 3, device=cuda))


def test_chamfer_to_cloud_sample_on_a_cloud_point_alone(cuda):
    """The ninth shape (a group of its own) has one face and one sample, placed on corner a, which is in the cloud:
    the shape's sum IS that sample's d = sqrt(0 + 1e-10) as fp32 rounds it, and its gradient is 0, not NaN."""
    from deftet_amd import hip_ops
    counts = [40] * 8 + [1]
    tri_np, gt_np, uv_np = _chamfer_inputs(1, counts, 70)
    uv_np[0, 8, 0, 0] = 0.0
    gt_np[8, 11] = tri_np[8, 0, 0]
    gt_np[8, 900] = tri_np[8, 0, 0]                                   # twice: the lower index is the nearest
    tri = _dev(tri_np, cuda).requires_grad_(True)
    gt, uv = _dev(gt_np, cuda), _dev(uv_np, cuda)
    out = hip_ops.chamfer_to_cloud(tri, gt, counts, 1, uv=uv)
    out.sum().backward()
    assert hip_ops.nn_index_ragged(_samples32(tri.detach(), uv), gt, counts)[8, 0].item() == 11
    assert out[8].item() == float(np.sqrt(np.float32(0.0) + np.float32(1e-10)))
    assert torch.isfinite(tri.grad).all() and (tri.grad[8] == 0).all()
    assert (out[:8] > 0.01).all() and (tri.grad[:8].abs().amax((1, 2, 3)) > 0).all()
