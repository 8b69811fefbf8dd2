"""The wide-channel vertex aggregation on the GPU (hip_ops.vertex_aggregate, deftet_amd.utils.matrix_utils.sparse_batch_matmul,
DESIGN.md section 6j).

Accuracy bound, derived and not measured: a row of n stored entries is summed as acc = 0, then acc = fmaf(a_k, x_k, acc) in CSR
order — n operations with one rounding each, so with u = 2^-24
    |out - ref64| <= gamma_n · Σ_k |a_k|·|x_k|,  gamma_n = n·u / (1 - n·u) <= (n + 1)·u   (n < 4000),
where ref64 is the fp64 product of the fp32 inputs (an index_add over the stored entries, duplicates included).  It is asserted
elementwise for the forward, and on the transposed rows for the gradient from backward() with a random upstream gradient.
Any fp32 summation of the same n products — multiply, then add, in any order — stays within (n + 1)·u·Σ|a_k|·|x_k| as well,
which is why the torch sparse path is compared within TWICE the bound.
"""
import gc
import os

import numpy as np
import pytest
import torch

from deftet_amd import grids

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
CHANNELS = [1, 3, 4, 5, 64, 128, 132, 256, 260, 512]


# ------------------------------------------------------------------------------------------------------------ adjacencies
def _kuhn(res, dev):
    from deftet_amd.utils.lib.tet_point_adj.interface import Tet_point_adj
    verts, tets = grids.kuhn_grid(res)
    V = verts.shape[0]
    return Tet_point_adj().run(V, tets.astype(np.int32), normalize=True).to(dev)


HAND_V, HAND_ISOLATED, HAND_SINGLE, HAND_HUBS = 203, (0, 17, 101, 202), (1, 64, 201), {5: 70, 130: 130}


def _hand_made(dev, duplicates=False):
    """V = 203 (no workgroup of 4, 8 or 16 rows is filled evenly): isolated vertices (no entry in their row or column, the
    first and the last vertex among them), rows of one entry, a hub row of 70 entries and one of 130 (more than one broadcast
    window at every group width), the rest 2..20 entries; signed values.  `duplicates`: every entry split into a quarter and
    three quarters, all shuffled."""
    rng = np.random.default_rng(31)
    V = HAND_V
    allowed = np.array([v for v in range(V) if v not in HAND_ISOLATED])
    rows, cols = [], []
    for i in range(V):
        if i in HAND_ISOLATED:
            continue
        n = HAND_HUBS.get(i, 1 if i in HAND_SINGLE else int(rng.integers(2, 21)))
        c = np.sort(rng.choice(allowed, size=n, replace=False))
        rows.append(np.full(n, i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.standard_normal(rows.shape[0]).astype(np.float32)
    if duplicates:
        perm = rng.permutation(2 * rows.shape[0])
        rows, cols = np.concatenate([rows, rows])[perm], np.concatenate([cols, cols])[perm]
        vals = np.concatenate([vals * np.float32(0.25), vals * np.float32(0.75)])[perm]
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (V, V)).to(dev)
    assert duplicates == (not adj.is_coalesced() and adj._nnz() > adj.coalesce()._nnz())
    return adj


def _one_vertex(dev):
    return torch.sparse_coo_tensor(torch.tensor([[0], [0]]), torch.tensor([-1.5]), (1, 1)).to(dev)


_ADJ = {}


def _case(name, dev):
    """(torch sparse tensor, VertexAdjacency) of a named case, built once per session"""
    from deftet_amd import hip_ops
    if name not in _ADJ:
        t = {"one": _one_vertex, "kuhn8": lambda d: _kuhn(8, d), "hand": _hand_made,
             "hand_dup": lambda d: _hand_made(d, duplicates=True), "kuhn40": lambda d: _kuhn(40, d),
             "kuhn70": lambda d: _kuhn(70, d)}[name](dev)
        _ADJ[name] = (t, hip_ops.VertexAdjacency.from_sparse(t))
    return _ADJ[name]


def _rand(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, device=dev, generator=g)


# ------------------------------------------------------------------------------------------------------------ fp64 reference
def _ref64(tadj, x, transpose=False, only_rows=None):
    """(ref64, bound) of M·x (Mᵀ·x with `transpose`) from the STORED entries of the torch sparse tensor, fp64 [B,V,C] each —
    or [B,len(only_rows),C] for the given rows only.  One shape and 64 channels at a time, to bound the memory."""
    idx, vals = tadj._indices(), tadj._values().double()
    rows, cols = (idx[1], idx[0]) if transpose else (idx[0], idx[1])
    V = tadj.shape[0]
    n = torch.bincount(rows, minlength=V)
    n_out = V
    if only_rows is not None:
        slot = torch.full((V,), -1, dtype=torch.int64, device=rows.device)
        slot[only_rows] = torch.arange(only_rows.numel(), device=rows.device)
        keep = slot[rows] >= 0
        rows, cols, vals = slot[rows[keep]], cols[keep], vals[keep]
        n, n_out = n[only_rows], only_rows.numel()
    B, _, C = x.shape
    ref = torch.zeros(B, n_out, C, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for b in range(B):
        for c0 in range(0, C, 64):
            terms = vals[:, None] * x[b, :, c0:c0 + 64].double()[cols]
            ref[b, :, c0:c0 + 64].index_add_(0, rows, terms)
            mag[b, :, c0:c0 + 64].index_add_(0, rows, terms.abs())
    return ref, (n + 1).double()[None, :, None] * U * mag


def _assert_within(got, ref, bound, what, factor=1.0):
    err = (got.double() - ref).abs()
    worst = (err - factor * bound).max().item()
    assert worst <= 0.0, "%s: |got - ref64| exceeds %g x bound by %.3e (largest error %.3e)" % (what, factor, worst, err.max().item())


def _fwd_bwd(x, adj, g):
    from deftet_amd import hip_ops
    xx = x.detach().clone().requires_grad_(True)
    out = hip_ops.vertex_aggregate(xx, adj)
    out.backward(g)
    return out.detach(), xx.grad


# ------------------------------------------------------------------------------------------------------------ 1. the bound
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("name", ["one", "kuhn8", "hand", "hand_dup"])
def test_forward_and_gradient_within_the_fp64_bound(cuda, name, C):
    tadj, adj = _case(name, cuda)
    V = tadj.shape[0]
    assert adj.nnz == tadj._nnz() and adj.n_vertex == V
    for B in (1, 3):
        x, g = _rand((B, V, C), cuda, 100 + C), _rand((B, V, C), cuda, 200 + C)
        out, gx = _fwd_bwd(x, adj, g)
        assert out.shape == (B, V, C) and out.dtype == torch.float32 and out.is_contiguous()
        assert gx.shape == (B, V, C) and gx.is_contiguous()
        _assert_within(out, *_ref64(tadj, x), "forward B=%d" % B)
        _assert_within(gx, *_ref64(tadj, g, transpose=True), "gradient B=%d" % B)
        if name.startswith("hand"):
            iso = list(HAND_ISOLATED)
            assert torch.equal(out[:, iso], torch.zeros_like(out[:, iso]))
            assert torch.equal(gx[:, iso], torch.zeros_like(gx[:, iso]))


def test_hand_made_rows_are_what_the_test_says(cuda):
    _, adj = _case("hand", cuda)
    n = (adj.offsets[1:] - adj.offsets[:-1]).cpu().numpy()
    tn = (adj.t_offsets[1:] - adj.t_offsets[:-1]).cpu().numpy()
    assert all(n[i] == 0 and tn[i] == 0 for i in HAND_ISOLATED)
    assert all(n[i] == 1 for i in HAND_SINGLE)
    assert all(n[i] == k for i, k in HAND_HUBS.items())
    _, dup = _case("hand_dup", cuda)
    assert dup.nnz == 2 * adj.nnz


def test_duplicates_sum_as_the_coalesced_matrix(cuda):
    (t1, a1), (t2, a2) = _case("hand", cuda), _case("hand_dup", cuda)
    x = _rand((2, HAND_V, 132), cuda, 5)
    from deftet_amd import hip_ops
    o1, o2 = hip_ops.vertex_aggregate(x, a1), hip_ops.vertex_aggregate(x, a2)
    r1, b1 = _ref64(t1, x)
    r2, b2 = _ref64(t2, x)
    # the two references differ by the rounding of 0.75·v alone: u per entry
    assert ((r1 - r2).abs() <= b1).all()
    _assert_within(o2, r1, b1 + b2, "duplicates against the plain matrix")
    _assert_within(o1, r1, b1, "plain")


# ------------------------------------------------------------------------------------------------------------ 2. edge cases
def test_empty_adjacency_and_empty_shapes(cuda):
    from deftet_amd import hip_ops
    V = 50
    empty = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (V, V)).to(cuda)
    adj = hip_ops.VertexAdjacency.from_sparse(empty)
    assert adj.nnz == 0
    for C in (3, 256):
        x = _rand((2, V, C), cuda, 1).requires_grad_(True)
        out = hip_ops.vertex_aggregate(x, adj)
        assert torch.equal(out, torch.zeros(2, V, C, device=cuda))
        (gx,) = torch.autograd.grad(out, x, torch.ones_like(out))
        assert torch.equal(gx, torch.zeros_like(gx))
    out = hip_ops.vertex_aggregate(torch.zeros(0, V, 8, device=cuda), adj)
    assert out.shape == (0, V, 8)
    _, hand = _case("hand", cuda)
    assert hip_ops.vertex_aggregate(torch.zeros(0, HAND_V, 256, device=cuda), hand).shape == (0, HAND_V, 256)
    none = hip_ops.VertexAdjacency.from_sparse(torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (0, 0)).to(cuda))
    x0 = torch.zeros(3, 0, 4, device=cuda, requires_grad=True)
    out = hip_ops.vertex_aggregate(x0, none)
    assert out.shape == (3, 0, 4)
    out.sum().backward()
    assert x0.grad.shape == (3, 0, 4)


def test_argument_checks(cuda):
    from deftet_amd import hip_ops
    tadj, adj = _case("kuhn8", cuda)
    V = adj.n_vertex
    x = torch.zeros(1, V, 4, device=cuda)
    with pytest.raises(TypeError):
        hip_ops.vertex_aggregate(x, tadj)
    with pytest.raises(RuntimeError):
        hip_ops.vertex_aggregate(torch.zeros(1, V + 1, 4, device=cuda), adj)
    with pytest.raises(RuntimeError):
        hip_ops.vertex_aggregate(torch.zeros(V, 4, device=cuda), adj)
    with pytest.raises(RuntimeError):
        hip_ops.vertex_aggregate(torch.zeros(1, V, 0, device=cuda), adj)
    table = torch.zeros(V, 2, dtype=torch.int64, device=cuda)
    rowdiv = hip_ops.VertexAdjacency.from_table(table, torch.ones(V, 1, device=cuda), index_base=0)
    with pytest.raises(ValueError, match="VLAP_ROW_DIVISOR"):
        hip_ops.vertex_aggregate(x, rowdiv)


def test_non_contiguous_input_and_no_grad(cuda):
    from deftet_amd import hip_ops
    _, adj = _case("kuhn8", cuda)
    base = _rand((2, 128, adj.n_vertex), cuda, 8)
    xn = base.transpose(1, 2)                                      # [B,V,C], not contiguous: what the decoder's first layer hands on
    assert not xn.is_contiguous()
    out = hip_ops.vertex_aggregate(xn, adj)
    assert out.grad_fn is None and out.is_contiguous()
    assert torch.equal(out, hip_ops.vertex_aggregate(xn.contiguous(), adj))
    g = _rand(tuple(out.shape), cuda, 9).transpose(1, 2).contiguous().transpose(1, 2)      # a strided upstream gradient
    xr = xn.detach().requires_grad_(True)
    (gx,) = torch.autograd.grad(hip_ops.vertex_aggregate(xr, adj), xr, g)
    assert torch.equal(gx, _fwd_bwd(xn.contiguous(), adj, g.contiguous())[1])


# ------------------------------------------------------------------------------------------------------------ 3. path independence
def test_a_channel_does_not_depend_on_the_path(cuda):
    """the scalar path (5 channels), the vector path with four, two and one rows per wave (64, 128, 256 channels) and the chunked
    vector path (260, 512 channels) give the same bits for the same channel, forward and backward"""
    for name in ("hand", "kuhn8"):
        _, adj = _case(name, cuda)
        V = adj.n_vertex
        x, g = _rand((3, V, 512), cuda, 41), _rand((3, V, 512), cuda, 42)
        wide = _fwd_bwd(x, adj, g)
        for lo, hi in [(0, 260), (0, 5), (4, 260), (8, 72), (100, 228), (511, 512), (0, 3), (1, 133)]:
            part = _fwd_bwd(x[..., lo:hi].contiguous(), adj, g[..., lo:hi].contiguous())
            assert torch.equal(part[0], wide[0][..., lo:hi]), (name, lo, hi)
            assert torch.equal(part[1], wide[1][..., lo:hi]), (name, lo, hi)
    # as the issue states them, on the 260-wide call
    _, adj = _case("hand", cuda)
    from deftet_amd import hip_ops
    x = _rand((3, HAND_V, 260), cuda, 43)
    full = hip_ops.vertex_aggregate(x, adj)
    assert torch.equal(full[..., :5], hip_ops.vertex_aggregate(x[..., :5].contiguous(), adj))
    assert torch.equal(full[..., 4:260], hip_ops.vertex_aggregate(x[..., 4:260].contiguous(), adj))


@pytest.mark.parametrize("name,C", [("hand", 260), ("kuhn40", 256), ("kuhn8", 5)])
def test_two_runs_are_bit_identical(cuda, name, C):
    _, adj = _case(name, cuda)
    x, g = _rand((3, adj.n_vertex, C), cuda, 51), _rand((3, adj.n_vertex, C), cuda, 52)
    first, second = _fwd_bwd(x, adj, g), _fwd_bwd(x, adj, g)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ------------------------------------------------------------------------------------------------------------ 4. against torch
def _torch_path(sparse_matrix, dense_matrix_batch):
    """the reference-shaped path: transpose to [n, b·p], torch.sparse.mm, transpose back"""
    b, n, p = dense_matrix_batch.shape
    flat = dense_matrix_batch.transpose(0, 1).reshape(n, b * p)
    return torch.sparse.mm(sparse_matrix, flat).reshape(n, b, p).transpose(0, 1)


@pytest.mark.parametrize("name", ["kuhn8", "kuhn40"])
def test_sparse_batch_matmul_against_the_torch_path(cuda, name):
    from deftet_amd.utils.matrix_utils import sparse_batch_matmul
    tadj, adj = _case(name, cuda)
    V = tadj.shape[0]
    x, g = _rand((2, V, 256), cuda, 61), _rand((2, V, 256), cuda, 62)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ours, theirs = sparse_batch_matmul(tadj, xa), _torch_path(tadj, xb)
    assert ours.is_contiguous() and ours.shape == theirs.shape
    ours.backward(g)
    theirs.backward(g)
    _, bound = _ref64(tadj, x)
    _, gbound = _ref64(tadj, g, transpose=True)
    assert ((ours.detach().double() - theirs.detach().double()).abs() <= 2.0 * bound).all()
    assert ((xa.grad.double() - xb.grad.double()).abs() <= 2.0 * gbound).all()
    # a VertexAdjacency is taken as it is
    assert torch.equal(sparse_batch_matmul(adj, x), ours.detach())


def test_conversion_is_cached_per_tensor_object(cuda, monkeypatch):
    from deftet_amd import hip_ops
    from deftet_amd.utils import matrix_utils
    builds = []
    real = hip_ops.VertexAdjacency._build.__func__

    def counting(cls, *args, **kwargs):
        builds.append(1)
        return real(cls, *args, **kwargs)

    base, _ = _case("kuhn8", cuda)                                  # (built before the counter is in place)
    monkeypatch.setattr(hip_ops.VertexAdjacency, "_build", classmethod(counting))
    x = _rand((2, base.shape[0], 8), cuda, 71)

    def fresh():
        return torch.sparse_coo_tensor(base._indices().clone(), base._values().clone(), base.shape)

    t1 = fresh()
    first = matrix_utils.sparse_batch_matmul(t1, x)
    for _ in range(3):
        assert torch.equal(matrix_utils.sparse_batch_matmul(t1, x), first)
    assert len(builds) == 1
    t2 = fresh()
    assert torch.equal(matrix_utils.sparse_batch_matmul(t2, x), first)
    assert len(builds) == 2
    matrix_utils.sparse_batch_matmul(t1, x)
    assert len(builds) == 2                                         # both stay cached
    key = id(t1)
    del t1
    gc.collect()
    assert key not in matrix_utils._adjacencies                     # the entry died with its tensor
    t3 = fresh()                                                    # (may or may not reuse the id: either way it is a new tensor)
    assert torch.equal(matrix_utils.sparse_batch_matmul(t3, x), first)
    assert len(builds) == 3


# ------------------------------------------------------------------------------------------------------------ 5. the reference block
def test_graph_conv_block_against_the_reference_fixture(cuda):
    """GraphConvBlock(size_in=12, size_out=8) of layers/gcn_decoder.py:90-129 rebuilt from the stored weights with F.linear and
    this repository's sparse_batch_matmul; tests/golden/gen_graph_conv.py ran the reference's own block on the host."""
    import torch.nn.functional as F
    from deftet_amd.utils.matrix_utils import sparse_batch_matmul
    d = np.load(os.path.join(HERE, "golden", "graph_conv.npz"))
    V = int(d["n_vertex"])
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([d["rows"], d["cols"]])), torch.from_numpy(d["vals"]), (V, V)).to(cuda)
    w = {k[2:]: torch.from_numpy(d[k]).to(cuda) for k in d.files if k.startswith("w.")}

    def layer(x, name):                                             # GraphConvLayer without its batch norm, then GraphConv
        a = F.relu(x)
        return (F.linear(a, w[name + ".conv.self_filter.weight"], w[name + ".conv.self_filter.bias"]) +
                F.linear(sparse_batch_matmul(adj, a), w[name + ".conv.filter.weight"], w[name + ".conv.filter.bias"]))

    x = torch.from_numpy(d["x"]).to(cuda).requires_grad_(True)
    y = F.linear(x, w["shortcut.weight"], w["shortcut.bias"]) + layer(layer(x, "layer_0"), "layer_1")
    (gx,) = torch.autograd.grad(y, x, torch.from_numpy(d["gy"]).to(cuda))
    for got, want in ((y.detach().cpu().numpy(), d["y"]), (gx.cpu().numpy(), d["gx"])):
        assert got.shape == want.shape
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------------------ 6. full size
def test_full_size_on_sampled_rows(cuda):
    """res 70, B = 8, C = 256 (V = 46,656): forward and gradient within the bound on 4,096 rows of every shape — the first, the
    last and the longest row among them"""
    tadj, adj = _case("kuhn70", cuda)
    V, B, C = tadj.shape[0], 8, 256
    assert V == 46656
    x, g = _rand((B, V, C), cuda, 81), _rand((B, V, C), cuda, 82)
    out, gx = _fwd_bwd(x, adj, g)
    perm = np.random.default_rng(83).permutation(V)
    for got, src, transpose, offsets in ((out, x, False, adj.offsets), (gx, g, True, adj.t_offsets)):
        longest = int((offsets[1:] - offsets[:-1]).argmax())
        must = sorted({0, V - 1, longest})
        rest = perm[~np.isin(perm, must)][:4096 - len(must)]
        rows = torch.from_numpy(np.sort(np.concatenate([must, rest]))).to(cuda)
        assert rows.numel() == 4096 and rows.unique().numel() == 4096
        ref, bound = _ref64(tadj, src, transpose=transpose, only_rows=rows)
        _assert_within(got[:, rows], ref, bound, "gradient" if transpose else "forward")
