"""The vertex Laplacian regulariser (hip_ops.VertexAdjacency, hip_ops.vertex_laplacian) in its two forms:
  training  DefTet.laplacian_sparse (layers/DefTet/deftet.py:340-343): D⁻¹A, Σ_{i,c} r² per shape — against fp64 and the torch
            sparse path;
  render    Deftet.get_featlap (diff_render/diftet_6_subdiv/3_model/deftet.py:221-241): the padded point table — bit-identical to
            an fp32 restatement that sums in table order and then divides, and close to the reference formula in torch.
Gradients against fp64 autograd of the reference formulas; duplicates, isolated vertices, empty adjacencies, channel counts,
bad indices, determinism and graph capture."""
import numpy as np
import pytest
import torch

from deftet_amd import grids

pytestmark = pytest.mark.gpu


def _grid(res):
    verts, tets = grids.kuhn_grid(res)
    return verts.shape[0], tets.astype(np.int32)


def _x(B, V, C, seed=3, scale=0.05):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal((B, V, C)) * scale).astype(np.float32))


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _torch_adj(V, tets, dev):
    from deftet_amd.utils.lib.tet_point_adj.interface import Tet_point_adj
    return Tet_point_adj().run(V, tets, normalize=True).to(dev)


def _train_ref64(x, adj, reduction):
    """fp64 restatement of the training form: nei = A x per shape (an index_add over the stored entries), r = nei - x"""
    a = adj.coalesce()
    rows, cols = a.indices()
    vals = a.values().double()
    x64 = x if x.dtype == torch.float64 else x.double()
    nei = torch.zeros_like(x64).index_add(1, rows, vals[None, :, None] * x64[:, cols])
    r2 = (nei - x64) ** 2
    return r2.sum(dim=(1, 2)) if reduction == "shape" else r2


def _render_table(V, tets, dev, extra=0):
    """hip_ops.point_adj_idx stored as the reference stores it (3_model/deftet.py:160-161): +1, weights + 1e-10"""
    from deftet_amd import hip_ops
    table, adjsum = hip_ops.point_adj_idx(V + extra, torch.from_numpy(tets).to(dev))
    return table + 1, adjsum + 1e-10


def _render_ref(x, table1, w, reduction="none"):
    """the reference formula (get_featlap) in torch, per shape; fp64 when x is"""
    P, m = table1.shape
    out = []
    for f in x:
        f1 = torch.nn.functional.pad(f, (0, 0, 1, 0))
        nei = f1[table1.view(-1), :].view(P, m, -1).sum(1) / w.to(f.dtype)
        out.append(torch.nn.functional.mse_loss(nei, f, reduction="none"))
    out = torch.stack(out)
    return out.sum(dim=(1, 2)) if reduction == "shape" else out


# ------------------------------------------------------------------------------------------------------------ 1. training form
@pytest.mark.parametrize("res,B", [(8, 2), (40, 8), (70, 8)])
def test_training_form(cuda, res, B):
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    V, tets = _grid(res)
    tadj = _torch_adj(V, tets, cuda)
    a_sp = hip_ops.VertexAdjacency.from_sparse(tadj)
    a_tt = hip_ops.VertexAdjacency.from_tets(torch.from_numpy(tets).to(cuda), V, normalize=True)
    for k in ("offsets", "cols", "vals", "t_offsets", "t_rows", "t_vals"):
        assert torch.equal(getattr(a_sp, k), getattr(a_tt, k)), k
    assert a_sp.nnz == tadj._nnz() and a_sp.weighting == hip_ops.VLAP_VALUES and a_sp.n_vertex == V
    x = _x(B, V, 3).to(cuda)
    loss = hip_ops.vertex_laplacian(x, a_sp, reduction="shape")
    assert loss.shape == (B,) and loss.dtype == torch.float32
    want = _train_ref64(x, tadj, "shape")
    assert ((loss.double() - want).abs() / want.abs()).max() <= 1e-5
    torch_path = DefTet(device=cuda).laplacian_sparse(x, tadj)
    torch.testing.assert_close(loss, torch_path, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------------------ 2. render form
@pytest.mark.parametrize("res,C", [(8, 7), (40, 7), (70, 3)])
def test_render_form_bit_identical_to_table_order_restatement(cuda, res, C):
    from deftet_amd import hip_ops
    from deftet_amd.render import get_featlap
    V, tets = _grid(res)
    table1, w = _render_table(V, tets, cuda)
    adj = hip_ops.VertexAdjacency.from_table(table1, w, index_base=1)
    assert adj.weighting == hip_ops.VLAP_ROW_DIVISOR
    feat = _x(1, V, C, seed=5, scale=1.0)[0].to(cuda)
    got = get_featlap(feat, adj)
    assert got.shape == (V, C)
    # fp32 restatement: an explicit loop over the table's columns (np.sum would sum pairwise), then one division
    t = table1.cpu().numpy()
    xp = np.concatenate([np.zeros((1, C), np.float32), feat.cpu().numpy()], 0)
    acc = np.zeros((V, C), np.float32)
    for k in range(t.shape[1]):
        acc = acc + xp[t[:, k]]
    r = acc / w.cpu().numpy() - xp[1:]
    want = r * r
    assert want.dtype == np.float32
    assert np.array_equal(got.cpu().numpy(), want)
    ref = _render_ref(feat[None], table1, w)[0]
    assert _rel(got, ref) <= 1e-6
    # this repository's own -1 padded table gives the same adjacency
    table0 = table1 - 1
    adj0 = hip_ops.VertexAdjacency.from_table(table0, w, index_base=0)
    assert torch.equal(get_featlap(feat, adj0), got)


# ------------------------------------------------------------------------------------------------------------ 3. gradients
def _adjacency(form, res, dev, extra=0):
    from deftet_amd import hip_ops
    V, tets = _grid(res)
    if form == "train":
        tadj = _torch_adj(V + extra, tets, dev)
        return V + extra, hip_ops.VertexAdjacency.from_sparse(tadj), lambda x, red: _train_ref64(x, tadj, red)
    table1, w = _render_table(V, tets, dev, extra)
    return V + extra, hip_ops.VertexAdjacency.from_table(table1, w, index_base=1), lambda x, red: _render_ref(x, table1, w, red)


@pytest.mark.parametrize("form", ["train", "render"])
@pytest.mark.parametrize("reduction", ["shape", "none"])
def test_gradients_against_fp64(cuda, form, reduction):
    from deftet_amd import hip_ops
    V, adj, ref = _adjacency(form, 12, cuda)
    B, C = 3, (3 if form == "train" else 7)
    x = _x(B, V, C, seed=9).to(cuda).requires_grad_(True)
    out = hip_ops.vertex_laplacian(x, adj, reduction=reduction)
    rng = np.random.default_rng(13)
    g = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).to(cuda)
    (gx,) = torch.autograd.grad(out, x, g)
    x64 = x.detach().double().requires_grad_(True)
    out64 = ref(x64, reduction)
    (gx64,) = torch.autograd.grad(out64, x64, g.double())
    assert _rel(out.detach(), out64.detach()) <= 1e-5
    assert _rel(gx, gx64) <= 1e-5
    # without requires_grad: the same values, no graph
    out_ng = hip_ops.vertex_laplacian(x.detach(), adj, reduction=reduction)
    assert out_ng.grad_fn is None and not out_ng.requires_grad
    assert torch.equal(out_ng, out.detach())


# ------------------------------------------------------------------------------------------------------------ 4. edge cases
def test_uncoalesced_duplicates_and_row_order(cuda):
    from deftet_amd import hip_ops
    V, tets = _grid(6)
    tadj = _torch_adj(V, tets, cuda).coalesce()
    idx, val = tadj.indices(), tadj.values()
    n = val.numel()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to(cuda)
    x = _x(2, V, 3).to(cuda).requires_grad_(True)
    a_ref = hip_ops.VertexAdjacency.from_sparse(tadj)
    # rows out of order, no duplicates: the same CSR, so the same bits
    shuffled = torch.sparse_coo_tensor(idx[:, perm], val[perm], tadj.shape)
    a_sh = hip_ops.VertexAdjacency.from_sparse(shuffled)
    for k in ("offsets", "cols", "vals", "t_offsets", "t_rows", "t_vals"):
        assert torch.equal(getattr(a_sh, k), getattr(a_ref, k)), k
    # every entry split into two duplicates (a quarter and three quarters), all shuffled: summed as torch.sparse.mm sums them
    idx2 = torch.cat([idx, idx], 1)[:, torch.cat([perm, perm + n])]
    val2 = torch.cat([val * 0.25, val * 0.75])[torch.cat([perm, perm + n])]
    dup = torch.sparse_coo_tensor(idx2, val2, tadj.shape)
    assert not dup.is_coalesced()
    a_dup = hip_ops.VertexAdjacency.from_sparse(dup)
    assert a_dup.nnz == 2 * n
    for red in ("shape", "none"):
        o_ref = hip_ops.vertex_laplacian(x, a_ref, reduction=red)
        o_dup = hip_ops.vertex_laplacian(x, a_dup, reduction=red)
        torch.testing.assert_close(o_dup, o_ref, rtol=1e-5, atol=1e-7)
        g = torch.ones_like(o_ref)
        torch.testing.assert_close(torch.autograd.grad(o_dup, x, g)[0], torch.autograd.grad(o_ref, x, g)[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(hip_ops.vertex_laplacian(x, a_dup), _train_ref64(x.detach(), dup, "shape").float(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("form", ["train", "render"])
def test_isolated_vertices(cuda, form):
    from deftet_amd import hip_ops
    extra = 5
    V, adj, ref = _adjacency(form, 6, cuda, extra=extra)
    x = _x(2, V, 3, seed=4).to(cuda).requires_grad_(True)
    out = hip_ops.vertex_laplacian(x, adj, reduction="none")
    iso = x.detach()[:, V - extra:]
    assert torch.equal(out.detach()[:, V - extra:], iso * iso)                       # r = -x
    g = torch.from_numpy(np.random.default_rng(2).standard_normal(tuple(out.shape)).astype(np.float32)).to(cuda)
    (gx,) = torch.autograd.grad(out, x, g)
    assert torch.equal(gx[:, V - extra:], (2.0 * g[:, V - extra:]) * iso)           # dx = -u = 2 g x, nobody's neighbour
    x64 = x.detach().double().requires_grad_(True)
    (gx64,) = torch.autograd.grad(ref(x64, "none"), x64, g.double())
    assert _rel(gx, gx64) <= 1e-5


def test_empty_adjacency(cuda):
    from deftet_amd import hip_ops
    V = 50
    empty = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (V, V)).to(cuda)
    tables = [hip_ops.VertexAdjacency.from_sparse(empty),
              hip_ops.VertexAdjacency.from_table(torch.zeros(V, 0, dtype=torch.int64, device=cuda), torch.ones(V, 1, device=cuda),
                                                 index_base=1)]
    x = _x(2, V, 4).to(cuda).requires_grad_(True)
    for adj in tables:
        assert adj.nnz == 0
        out = hip_ops.vertex_laplacian(x, adj)
        torch.testing.assert_close(out, (x.detach() ** 2).sum(dim=(1, 2)), rtol=1e-6, atol=0)
        (gx,) = torch.autograd.grad(out, x, torch.ones_like(out))
        assert torch.equal(gx, 2.0 * x.detach())


@pytest.mark.parametrize("C", [1, 3, 4, 7, 16])
def test_channel_counts(cuda, C):
    from deftet_amd import hip_ops
    for form in ("train", "render"):
        V, adj, ref = _adjacency(form, 8, cuda)
        x = _x(2, V, C, seed=C).to(cuda).requires_grad_(True)
        for red in ("shape", "none"):
            out = hip_ops.vertex_laplacian(x, adj, reduction=red)
            g = torch.rand(out.shape, device=cuda)
            (gx,) = torch.autograd.grad(out, x, g)
            x64 = x.detach().double().requires_grad_(True)
            out64 = ref(x64, red)
            (gx64,) = torch.autograd.grad(out64, x64, g.double())
            assert _rel(out.detach(), out64.detach()) <= 1e-5, (form, red)
            assert _rel(gx, gx64) <= 1e-5, (form, red)


def test_non_contiguous_x(cuda):
    from deftet_amd import hip_ops
    V, adj, _ = _adjacency("train", 8, cuda)
    base = _x(2, 3, V).to(cuda)                                    # [B,C,V]
    xn = base.transpose(1, 2).requires_grad_(True)                 # [B,V,C], not contiguous
    assert not xn.is_contiguous()
    xc = xn.detach().contiguous().requires_grad_(True)
    for red in ("shape", "none"):
        on, oc = hip_ops.vertex_laplacian(xn, adj, reduction=red), hip_ops.vertex_laplacian(xc, adj, reduction=red)
        assert torch.equal(on, oc)
        g = torch.rand(on.shape, device=cuda)
        (gn,), (gc,) = torch.autograd.grad(on, xn, g), torch.autograd.grad(oc, xc, g)
        assert torch.equal(gn, gc)


def test_bad_indices_and_channels_are_refused(cuda):
    from deftet_amd import hip_ops
    V, tets = _grid(6)
    table1, w = _render_table(V, tets, cuda)
    for bad in (V + 3, -5):
        t = table1.clone() - 1
        t[V // 2, 0] = bad
        with pytest.raises(RuntimeError):
            hip_ops.VertexAdjacency.from_table(t, w, index_base=0)
    adj = hip_ops.VertexAdjacency.from_table(table1, w, index_base=1)
    for C in (17, 0):
        with pytest.raises(RuntimeError):
            hip_ops.vertex_laplacian(torch.zeros(1, V, C, device=cuda), adj)
    with pytest.raises(RuntimeError):
        hip_ops.vertex_laplacian(torch.zeros(1, V + 1, 3, device=cuda), adj)
    with pytest.raises(ValueError):
        hip_ops.vertex_laplacian(torch.zeros(1, V, 3, device=cuda), adj, reduction="mean")


# ------------------------------------------------------------------------------------------------------------ 5. determinism, capture
def _fwd_bwd(hip_ops, x, adj, red, g):
    xx = x.detach().clone().requires_grad_(True)
    out = hip_ops.vertex_laplacian(xx, adj, reduction=red)
    (gx,) = torch.autograd.grad(out, xx, g)
    return out.detach(), gx


@pytest.mark.parametrize("form,red", [("train", "shape"), ("render", "none")])
def test_deterministic(cuda, form, red):
    from deftet_amd import hip_ops
    V, adj, _ = _adjacency(form, 40, cuda)
    x = _x(8, V, 3).to(cuda)
    g = torch.rand((8,) if red == "shape" else (8, V, 3), device=cuda)
    runs = [_fwd_bwd(hip_ops, x, adj, red, g) for _ in range(3)]
    for o, gx in runs[1:]:
        assert torch.equal(o, runs[0][0]) and torch.equal(gx, runs[0][1])


@pytest.mark.parametrize("form,red", [("train", "shape"), ("render", "none")])
def test_graph_capture_replay_equals_eager(cuda, form, red):
    from deftet_amd import hip_ops
    V, adj, _ = _adjacency(form, 20, cuda)
    B = 4
    x = _x(B, V, 3).to(cuda).requires_grad_(True)
    g = torch.rand((B,) if red == "shape" else (B, V, 3), device=cuda)
    eager = _fwd_bwd(hip_ops, x, adj, red, g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            out = hip_ops.vertex_laplacian(x, adj, reduction=red)
            torch.autograd.grad(out, x, g)
        del out                                                        # (nothing of the warm-up graph stays alive)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = hip_ops.vertex_laplacian(x, adj, reduction=red)
        (gx_s,) = torch.autograd.grad(out_s, x, g)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_s.detach(), eager[0]) and torch.equal(gx_s, eager[1])
    with torch.no_grad():
        x.mul_(2.0)                                                    # replay on new values of the same input
    graph.replay()
    torch.cuda.synchronize()
    again = _fwd_bwd(hip_ops, x, adj, red, g)
    assert torch.equal(out_s.detach(), again[0]) and torch.equal(gx_s, again[1])


# ------------------------------------------------------------------------------------------------------------ 6. DefTet layer
def test_laplacian_sparse_with_a_vertex_adjacency(cuda):
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet, TetTopology
    V, tets = _grid(20)
    tet_t = torch.from_numpy(tets).to(cuda)
    topo = TetTopology(tet_t.long(), V)
    adj = topo.vertex_adjacency()
    assert topo.vertex_adjacency() is adj                              # built once
    ref = hip_ops.VertexAdjacency.from_tets(tet_t, V, normalize=True)
    for k in ("offsets", "cols", "vals", "t_offsets", "t_rows", "t_vals"):
        assert torch.equal(getattr(adj, k), getattr(ref, k)), k
    plain = topo.vertex_adjacency(normalize=False)
    assert torch.equal(plain.vals, torch.ones_like(plain.vals))
    layer = DefTet(device=cuda)
    off = _x(4, V, 3).to(cuda).requires_grad_(True)
    got = layer.laplacian_sparse(off, adj)
    want = hip_ops.vertex_laplacian(off, adj, reduction="shape")
    assert torch.equal(got, want)
    (g1,), (g2,) = torch.autograd.grad(got.sum(), off), torch.autograd.grad(want.sum(), off)
    assert torch.equal(g1, g2)
    # a torch sparse adjacency keeps the torch path, and the two agree
    torch.testing.assert_close(layer.laplacian_sparse(off, _torch_adj(V, tets, cuda)), got, rtol=1e-5, atol=0)
