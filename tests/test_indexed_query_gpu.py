"""The indexed occupancy query (deftet_point_in_tet_indexed_*): vertices + an index list in, the same bits out as the dense
entry points on the tensor tet_gather makes from the same inputs — forward (every algo, traversal order, query box, the
two-call form), backward onto the vertices (records and lists, either forward's records), bad indices, autograd through
DefTet.occupancy_query(indexed=True), activation memory and graph capture."""
import numpy as np
import pytest
import torch

from deftet_amd import grids

pytestmark = pytest.mark.gpu

ALGOS = (0, 1, 2, 3, 4, 5)          # AUTO, BRUTE, EXACT, SLAB, WAVE, PAIR


def _same(a, b):
    """bit-equal, NaN masks included"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool((a[~na] == b[~nb]).all())


def _mesh(res, batch, cuda, per_shape=False, seed=3):
    verts, tets = grids.kuhn_grid(res)
    pos = torch.from_numpy(grids.jittered_positions(verts, res, batch, 0.1).astype(np.float32)).to(cuda)
    idx = torch.from_numpy(tets.astype(np.int64)).to(cuda)
    if per_shape:                                                   # a different tet numbering per shape
        rng = np.random.default_rng(seed)
        idx = torch.stack([idx[torch.from_numpy(rng.permutation(len(tets))).to(cuda)] for _ in range(batch)])
    return pos, idx


def _soup(tet_bxtx4x3, cuda):
    """a tet soup as a topology: V = 4T, idx = arange"""
    t = torch.from_numpy(np.ascontiguousarray(tet_bxtx4x3)).to(cuda)
    B, T = t.shape[0], t.shape[1]
    return t.reshape(B, 4 * T, 3).contiguous(), torch.arange(4 * T, device=cuda, dtype=torch.int64).reshape(T, 4)


def _both(pos, idx, pts, **kw):
    from deftet_amd import hip_ops
    a = hip_ops.point_in_tet(hip_ops.tet_gather(pos, idx), pts, **kw)
    b = hip_ops.point_in_tet_indexed(pos, idx, pts, **kw)
    return (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))


@pytest.mark.parametrize("res,batch,per_shape", [(8, 2, False), (10, 3, True), (40, 8, False)])
def test_forward_equals_dense_every_algo(cuda, res, batch, per_shape):
    from deftet_amd import hip_ops
    pos, idx = _mesh(res, batch, cuda, per_shape)
    T = idx.shape[-2]
    pts = torch.from_numpy(grids.random_queries(batch, 3000 if res < 40 else 50000)).to(cuda)
    pred = torch.rand(batch, T, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    for algo in ALGOS:
        a, b = _both(pos, idx, pts, want_bary=True, algo=algo, pred_bxt=pred)
        for name, x, y in zip(("cond", "bary", "occ"), a, b):
            assert _same(x, y), (algo, name)


@pytest.mark.parametrize("res,batch,per_shape", [(10, 2, False), (40, 8, True)])
def test_forward_equals_dense_with_hints(cuda, res, batch, per_shape):
    from deftet_amd import hip_ops
    pos, idx = _mesh(res, batch, cuda, per_shape)
    T = idx.shape[-2]
    pts = torch.from_numpy(grids.random_queries(batch, 4000)).to(cuda)
    pred = torch.rand(batch, T, device=cuda, generator=torch.Generator(device=cuda).manual_seed(2))
    tet = hip_ops.tet_gather(pos, idx)
    box = torch.tensor([[-0.4, -0.45, -0.5, 0.45, 0.4, 0.5]] * batch, device=cuda)
    orders = [None, hip_ops.tet_spatial_order(tet[0]), "auto"]
    for algo in (0, 3, 4, 5):
        for order in orders:
            for qb in (None, box, "track"):
                kw = dict(want_bary=True, algo=algo, pred_bxt=pred, want_hits=True, order=order, query_box=qb)
                a = hip_ops.point_in_tet(tet, pts, **kw)
                b = hip_ops.point_in_tet_indexed(pos, idx, pts, **kw)
                for name, x, y in zip(("cond", "bary", "occ"), a[:3], b[:3]):
                    assert _same(x, y), (algo, name, order if order is None or isinstance(order, str) else "perm", qb if qb is None or isinstance(qb, str) else "box")
    hip_ops.clear_query_box_cache()
    # the two-call form, the query side prepared on a second stream
    side = torch.cuda.Stream()
    for algo in (0, 2, 4):
        want = hip_ops.point_in_tet(tet, pts, want_bary=True, algo=algo, pred_bxt=pred)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pq = hip_ops.prepare_queries(pts, T, algo=algo)
        got = hip_ops.point_in_tet_indexed(pos, idx, pts, want_bary=True, algo=algo, pred_bxt=pred, prepared=pq)
        for x, y in zip(want, got):
            assert _same(x, y), algo


@pytest.mark.parametrize("case", ["adversarial", "scaled_small", "scaled_big"])
def test_forward_equals_dense_on_soups(cuda, case):
    from tests import cases
    tet, pts = {"adversarial": lambda: cases.adversarial(0), "scaled_small": lambda: cases.scaled(1e-3, (5.0, -3.0, 2.0)),
                "scaled_big": lambda: cases.scaled(3e4, (1e5, 0.0, -2e5))}[case]()
    pos, idx = _soup(tet, cuda)
    q = torch.from_numpy(np.ascontiguousarray(pts)).to(cuda)
    for algo in ALGOS:
        a, b = _both(pos, idx, q, want_bary=True, algo=algo)
        for name, x, y in zip(("cond", "bary"), a, b):
            assert _same(x, y), (case, algo, name)


@pytest.mark.parametrize("res,n_query", [(40, 50000), (70, 100000)])
def test_full_size_fwd_bwd_equal_dense(cuda, res, n_query):
    """configs[1] / configs[2], B = 8, AUTO with the autograd ops' hints: forward bit-equal, and the indexed backward from the
    indexed forward's records bit-equal to the dense backward from the dense forward's records."""
    from deftet_amd import hip_ops
    B = 8
    pos, idx = _mesh(res, B, cuda)
    T = idx.shape[0]
    pts = torch.from_numpy(grids.random_queries(B, n_query)).to(cuda)
    g = torch.Generator(device=cuda).manual_seed(7)
    pred = torch.rand(B, T, device=cuda, generator=g)
    gw = torch.randn(B, n_query, 4, device=cuda, generator=g)
    go = torch.randn(B, n_query, device=cuda, generator=g)
    csr = hip_ops.tet_vertex_csr(idx, pos.shape[1])
    kw = dict(want_bary=True, pred_bxt=pred, want_hits=True, order="auto", query_box="track")
    tet = hip_ops.tet_gather(pos, idx)
    a = hip_ops.point_in_tet(tet, pts, **kw)
    b = hip_ops.point_in_tet_indexed(pos, idx, pts, **kw)
    for name, x, y in zip(("cond", "bary", "occ"), a[:3], b[:3]):
        assert _same(x, y), name
    ga = hip_ops.point_in_tet_bwd_to_vertices(tet, pts, a[0], gw, csr, pos.shape[1], want_grad_pts=True, grad_occ=go, hits=a[3])
    gb = hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, idx, pts, b[0], gw, csr, want_grad_pts=True, grad_occ=go, hits=b[3])
    for name, x, y in zip(("grad_pos", "grad_pts", "grad_pred"), ga, gb):
        assert _same(x, y), name
    hip_ops.clear_query_box_cache()


@pytest.mark.parametrize("res,n_query,batch,per_shape", [(8, 500, 2, False), (10, 4000, 3, True), (6, 3000, 1, False)])
def test_backward_paths(cuda, res, n_query, batch, per_shape):
    """record path bit-equal (with / without grad_pts and grad_occ, out= accumulation), records of either forward fed to either
    backward; the list path (no records, or > 2 queries per tet) within the bound test_bwd_to_vertices_equals_two_call_form uses."""
    from deftet_amd import hip_ops
    pos, idx = _mesh(res, batch, cuda, per_shape)
    V, T = pos.shape[1], idx.shape[-2]
    csr = hip_ops.tet_vertex_csr(idx, V)
    q = torch.from_numpy(grids.random_queries(batch, n_query)).to(cuda)
    g = torch.Generator(device=cuda).manual_seed(11)
    pred = torch.rand(batch, T, device=cuda, generator=g)
    gw = torch.randn(batch, n_query, 4, device=cuda, generator=g)
    go = torch.randn(batch, n_query, device=cuda, generator=g)
    tet = hip_ops.tet_gather(pos, idx)
    fa = hip_ops.point_in_tet(tet, q, want_bary=True, pred_bxt=pred, want_hits=True)
    fb = hip_ops.point_in_tet_indexed(pos, idx, q, want_bary=True, pred_bxt=pred, want_hits=True)
    assert torch.equal(fa[0], fb[0])
    records = n_query <= 2 * T
    for want_pts in (False, True):
        for gocc in (None, go):
            for hits_a, hits_b in ((fa[3], fb[3]), (fb[3], fa[3]), (None, None)):
                ref = hip_ops.point_in_tet_bwd_to_vertices(tet, q, fa[0], gw, csr, V, want_grad_pts=want_pts, grad_occ=gocc, hits=hits_a)
                got = hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, idx, q, fb[0], gw, csr, want_grad_pts=want_pts, grad_occ=gocc,
                                                                   hits=hits_b)
                for k, (x, y) in enumerate(zip(ref, got)):
                    if x is None:
                        assert y is None
                    elif records and hits_a is not None:
                        assert _same(x, y), (want_pts, gocc is not None, k)
                    else:
                        assert torch.allclose(x, y, rtol=1e-5, atol=1e-5 * float(x.abs().max().clamp(min=1e-30))), (want_pts, k)
    if records:                                                      # out= accumulation
        base = torch.randn(batch, V, 3, device=cuda, generator=g)
        ra = hip_ops.point_in_tet_bwd_to_vertices(tet, q, fa[0], gw, csr, V, grad_occ=go, hits=fa[3], out=base.clone())
        rb = hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, idx, q, fb[0], gw, csr, grad_occ=go, hits=fb[3], out=base.clone())
        for x, y in zip(ra, rb):
            assert _same(x, y)


def test_empty_cases(cuda):
    from deftet_amd import hip_ops
    pos, idx = _mesh(4, 2, cuda)
    V = pos.shape[1]
    csr = hip_ops.tet_vertex_csr(idx, V)
    q0 = torch.zeros(2, 0, 3, device=cuda)
    c = hip_ops.point_in_tet_indexed(pos, idx, q0)
    assert c.shape == (2, 0, 1)
    z = hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, idx, q0, torch.zeros(2, 0, 1, device=cuda), torch.zeros(2, 0, 4, device=cuda), csr)
    assert z[0].shape == (2, V, 3) and bool((z[0] == 0).all())
    q = torch.from_numpy(grids.random_queries(2, 300)).to(cuda)
    e_idx = torch.zeros(0, 4, device=cuda, dtype=torch.int64)
    c, w = hip_ops.point_in_tet_indexed(pos, e_idx, q, want_bary=True)
    assert bool((c == -1).all()) and bool((w == 0).all())
    e_csr = hip_ops.tet_vertex_csr(e_idx, V)
    z = hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, e_idx, q, c, torch.randn(2, 300, 4, device=cuda), e_csr, want_grad_pts=True)
    assert bool((z[0] == 0).all()) and bool((z[1] == 0).all())
    # V == 0: every corner is out of range (NaN corners, as tet_gather writes them), pos is never read
    p0 = torch.zeros(2, 0, 3, device=cuda)
    small = torch.zeros(1, 4, device=cuda, dtype=torch.int64)
    c = hip_ops.point_in_tet_indexed(p0, small, q)
    assert torch.equal(c, hip_ops.point_in_tet(torch.full((2, 1, 4, 3), float("nan"), device=cuda), q))
    csr0 = (torch.zeros(1, device=cuda, dtype=torch.int32), torch.zeros(4, device=cuda, dtype=torch.int32), 1)
    z = hip_ops.point_in_tet_indexed_bwd_to_vertices(p0, small, q, c, torch.randn(2, 300, 4, device=cuda), csr0)
    assert z[0].shape == (2, 0, 3)


def test_bad_indices(cuda):
    """indices -1 and V: those corners read as NaN exactly as in tet_gather, every output equals the dense path on the
    NaN-carrying gathered tensor, the flag is raised and check=True raises."""
    from deftet_amd import hip_ops
    pos, idx = _mesh(8, 2, cuda)
    V = pos.shape[1]
    idx = idx.clone()
    idx[5, 2] = -1
    idx[100, 0] = V
    idx[101, 3] = V
    q = torch.from_numpy(grids.random_queries(2, 2000)).to(cuda)
    pred = torch.rand(2, idx.shape[0], device=cuda, generator=torch.Generator(device=cuda).manual_seed(4))
    tet = hip_ops.tet_gather(pos, idx)
    assert bool(torch.isnan(tet[:, 5, 2]).all())
    for algo in ALGOS:
        a = hip_ops.point_in_tet(tet, q, want_bary=True, algo=algo, pred_bxt=pred)
        b = hip_ops.point_in_tet_indexed(pos, idx, q, want_bary=True, algo=algo, pred_bxt=pred)
        for x, y in zip(a, b):
            assert _same(x, y), algo
    lib = __import__("deftet_amd._lib", fromlist=["load"]).load()
    from deftet_amd import _lib
    idx32 = idx.to(torch.int32).contiguous()
    cond = torch.empty(2, 2000, 1, device=cuda)
    bad = torch.zeros(1, device=cuda, dtype=torch.int32)
    ws = torch.empty(lib.deftet_point_in_tet_workspace_bytes(2, idx.shape[0], 2000, 0), device=cuda, dtype=torch.uint8)
    rc = lib.deftet_point_in_tet_indexed_f32(_lib.ptr(pos), _lib.ptr(idx32), 1, _lib.ptr(q), _lib.ptr(cond), None, None, None, None, 2, V,
                                             idx.shape[0], 2000, 0, None, None, None, None, _lib.ptr(bad), _lib.ptr(ws), ws.numel(),
                                             _lib.current_stream(cuda))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(bad.item()) == 1
    with pytest.raises(RuntimeError, match="out of range"):
        hip_ops.point_in_tet_indexed(pos, idx, q, check=True)
    hip_ops.point_in_tet_indexed(pos, idx.clamp(0, V - 1), q, check=True)          # (a good list passes the check)


def test_occupancy_query_indexed_autograd(cuda, oracle):
    """DefTet.occupancy_query(..., indexed=True) == the default path bit for bit (cond, w, occ, vertice_pos.grad, pred.grad), and
    the gradient matches fp64 autograd through torch.gather as test_occupancy_query_autograd_to_vertices checks it."""
    from deftet_amd.layers.DefTet.deftet import DefTet
    verts, tets = grids.kuhn_grid(8)
    pos = grids.jittered_positions(verts, 8, 2, 0.1).astype(np.float32)
    pts = grids.random_queries(2, 500)
    idx = torch.from_numpy(tets.astype(np.int64)).to(cuda)[None].expand(2, -1, -1).contiguous()
    q = torch.from_numpy(pts).to(cuda)
    gen = torch.Generator(device=cuda).manual_seed(5)
    pred0 = torch.rand(2, len(tets), device=cuda, generator=gen)
    m = DefTet(device=cuda)
    gw = torch.randn(2, 500, 4, device=cuda, generator=gen)
    go = torch.randn(2, 500, device=cuda, generator=gen)
    res = []
    for indexed in (False, True):
        p = torch.from_numpy(pos).to(cuda).requires_grad_(True)
        pred = pred0.clone().requires_grad_(True)
        cond, w, occ = m.occupancy_query(p, idx, q, pred, indexed=indexed)
        ((w * gw).sum() + (occ * go).sum()).backward()
        res.append((cond, w.detach(), occ.detach(), p.grad.clone(), pred.grad.clone()))
    for name, x, y in zip(("cond", "w", "occ", "grad_pos", "grad_pred"), res[0], res[1]):
        assert _same(x, y), name
    pc = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    tc = torch.gather(pc.unsqueeze(2).expand(-1, -1, 4, -1), 1, idx.cpu().unsqueeze(-1).expand(-1, -1, -1, 3))
    c = res[1][0].cpu()[..., 0]
    hit = c >= 0
    sel = torch.gather(tc, 1, c.clamp(min=0).long()[:, :, None, None].expand(-1, -1, 4, 3))
    pq = torch.tensor(pts, dtype=torch.float64)
    wc = torch.stack(oracle.bary_torch(sel[:, :, 0], sel[:, :, 1], sel[:, :, 2], sel[:, :, 3], pq), dim=-1) * hit[..., None]
    (wc * gw.cpu().double()).sum().backward()
    from tests.tol import check_close
    check_close("indexed occupancy_query grad_pos, res8 vs fp64 autograd", res[1][3], pc.grad, 5e-7, elem_rel=1e-4)


def test_occupancy_query_indexed_inplace_change_raises(cuda):
    from deftet_amd.layers.DefTet.deftet import DefTet
    pos, idx = _mesh(6, 2, cuda)
    q = torch.from_numpy(grids.random_queries(2, 300)).to(cuda)
    m = DefTet(device=cuda)
    leaf = pos.clone().requires_grad_(True)
    p = leaf * 1.0                                                   # a non-leaf that can be changed in place
    pred = torch.rand(2, idx.shape[0], device=cuda, requires_grad=True)
    _, w, occ = m.occupancy_query(p, idx, q, pred, indexed=True)
    with torch.no_grad():
        p.add_(0.01)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (w.sum() + occ.sum()).backward()


def test_occupancy_query_rejects_tets_of_another_shape(cuda):
    """tet_bxfx4x3 handed to occupancy_query must have the [B,T,4,3] shape of (vertice_pos, tetrahedron): its values are used and
    the gradient goes to vertice_pos, so a tensor of other tets would give wrong gradients silently."""
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    pos, idx = _mesh(6, 2, cuda)
    q = torch.from_numpy(grids.random_queries(2, 300)).to(cuda)
    pred = torch.rand(2, idx.shape[0], device=cuda)
    m = DefTet(device=cuda)
    tet = hip_ops.tet_gather(pos, idx)
    want = m.occupancy_query(pos, idx, q, pred)
    assert all(torch.equal(a, b) for a, b in zip(m.occupancy_query(pos, idx, q, pred, tet_bxfx4x3=tet), want))
    for bad in (tet[:1], tet[:, :-1], tet[..., :2].contiguous(), tet.reshape(-1, 4, 3)):
        with pytest.raises(RuntimeError, match="tet_bxfx4x3"):
            m.occupancy_query(pos, idx, q, pred, tet_bxfx4x3=bad)


def test_occupancy_query_indexed_keeps_no_gathered_tensor(cuda):
    """res 40, B = 8: across a forward with grad enabled the allocated memory rises by less than one [B,T,4,3] tensor (the
    default path keeps exactly that tensor for its backward)."""
    from deftet_amd.layers.DefTet.deftet import DefTet
    B = 8
    pos, idx = _mesh(40, B, cuda)
    T = idx.shape[0]
    q = torch.from_numpy(grids.random_queries(B, 50000)).to(cuda)
    m = DefTet(device=cuda)
    p = pos.clone().requires_grad_(True)
    pred = torch.rand(B, T, device=cuda, requires_grad=True)
    out = m.occupancy_query(p, idx, q, pred, indexed=True)            # warm-up: topology, workspaces, order decision, box tracker
    del out
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(cuda)
    out = m.occupancy_query(p, idx, q, pred, indexed=True)
    torch.cuda.synchronize()
    rise = torch.cuda.memory_allocated(cuda) - before
    assert rise < B * T * 48, (rise, B * T * 48)
    (out[1].sum() + out[2].sum()).backward()


def test_indexed_step_captured_in_a_hipgraph_replays_on_new_inputs(cuda):
    """the indexed fwd (order="auto", query_box="track") + bwd onto the vertices captured in one graph on one stream; replayed on
    other inputs copied into the captured tensors, it equals the eager operator every time."""
    from deftet_amd import hip_ops
    hip_ops.clear_query_box_cache()
    B, Q, res = 2, 2400, 12                                          # T = 1296: <= 2 queries per tet, the backward reads the records (bit-reproducible)
    verts, tets = grids.kuhn_grid(res)
    idx = torch.from_numpy(tets.astype(np.int32)).to(cuda)
    V, T = len(verts), len(tets)
    csr = hip_ops.tet_vertex_csr(idx, V)
    sets = []
    for s in range(3):
        g = torch.Generator(device=cuda).manual_seed(70 + s)
        pos = torch.from_numpy(grids.jittered_positions(verts, res, B, 0.1 + 0.05 * s, seed0=300 + 10 * s).astype(np.float32)).to(cuda)
        sets.append(dict(pos=pos, pts=torch.from_numpy(grids.random_queries(B, Q, seed0=900 + 10 * s)).to(cuda) * (1.0 + 0.1 * s),
                         pred=torch.rand(B, T, device=cuda, generator=g), gw=torch.randn(B, Q, 4, device=cuda, generator=g),
                         go=torch.randn(B, Q, device=cuda, generator=g)))
    st = {k: v.clone() for k, v in sets[0].items()}

    def step(d, **hints):
        cond, w, occ, hits = hip_ops.point_in_tet_indexed(d["pos"], idx, d["pts"], want_bary=True, pred_bxt=d["pred"], want_hits=True, **hints)
        gp, _, gr = hip_ops.point_in_tet_indexed_bwd_to_vertices(d["pos"], idx, d["pts"], cond, d["gw"], csr, grad_occ=d["go"], hits=hits)
        return cond, w, occ, gp, gr

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(st, order="auto", query_box="track")
    for i in (1, 2, 0, 2):
        for k in st:
            st[k].copy_(sets[i][k])
        graph.replay()
        torch.cuda.synchronize()
        want = step(sets[i])
        for name, a, b in zip(("cond", "w", "occ", "grad_pos", "grad_pred"), out, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (i, name)
    del graph
    hip_ops.clear_query_box_cache()
