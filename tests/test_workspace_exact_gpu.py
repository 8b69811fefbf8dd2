"""Every operator whose workspace size comes from a layout function ("Workspaces"), run on a workspace of EXACTLY the
declared size: the shared allocator is replaced by one that hands out the 256-byte-aligned middle of `guard + n + guard` bytes,
both guards 64 KiB of 0xA5, so `ws.numel()` is the declared size to the byte (the real allocator never gives less than 1 MiB or
1.25 x the request, which hides an under-declared size at every shape a test can afford).  The three operators that allocate
their workspace privately (surface_extract, marching_tets, voxel_surface_mesh) run their count and fill entries through the C ABI on such a buffer.  Each test asserts that the
allocator was asked, that both guards are intact after a synchronise, and that every output equals, bit for bit, the same call
made the normal way.

This catches a write within 64 KiB past either end of a workspace.  It cannot catch a read outside it, nor a write further off.
Every byte the operators may touch belongs to the test's own allocation.

Shapes: the smallest that cross one scan tile (2,048 elements), one 256-thread workgroup and one launch group of shapes."""
import numpy as np
import pytest
import torch

from deftet_amd import grids

pytestmark = pytest.mark.gpu
GUARD = 64 << 10


class Guarded:
    """the allocator: a fresh guarded buffer per request, so nothing is shared between the calls of one operator either"""

    def __init__(self):
        self.blocks = []

    def __call__(self, device, nbytes):
        n = int(nbytes)
        raw = torch.full((GUARD + n + GUARD + 256,), 0xA5, dtype=torch.uint8, device=device)
        start = GUARD + (-(raw.data_ptr() + GUARD)) % 256
        self.blocks.append((raw, start, n))
        return raw[start:start + n]

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((raw[:start] == 0xA5).all()) and bool((raw[start + n:] == 0xA5).all()) for raw, start, n in self.blocks)


def flat(x):
    """the tensors (and plain values) of an operator's result, in order"""
    from deftet_amd import hip_ops
    if isinstance(x, hip_ops.VertexAdjacency):
        return flat((x.offsets, x.cols, x.vals, x.t_offsets, x.t_rows, x.t_vals))
    if isinstance(x, hip_ops.TetEdges):
        return flat((x.edges, x.tet_edge, x.offsets, x.slots))
    if isinstance(x, hip_ops.FaceTopology):
        return flat((x.offsets, x.slots))
    if isinstance(x, (tuple, list)):
        return [y for e in x for y in flat(e)]
    return [x]


def same_bits(a, b):
    if torch.is_tensor(a) and torch.is_tensor(b):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().flatten().view(torch.uint8),
                                                                           b.contiguous().flatten().view(torch.uint8))
    return not torch.is_tensor(a) and not torch.is_tensor(b) and a == b


def check_exact(monkeypatch, call):
    from deftet_amd import _lib
    want = flat(call())
    torch.cuda.synchronize()
    g = Guarded()
    with monkeypatch.context() as m:
        m.setattr(_lib, "workspace", g)
        got = flat(call())
    assert g.blocks, "the operator did not ask for a workspace"
    assert g.intact(), "a guard was written"
    assert len(want) == len(got) and len(want) > 0
    for i, (a, b) in enumerate(zip(want, got)):
        assert same_bits(a, b), "output %d differs" % i


def rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32))


def rnd_idx(seed, hi, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, hi, shape, dtype=np.int64))


@pytest.fixture(scope="module", params=[2, 8], ids=["res2", "res8"])
def grid(request, cuda):
    verts, tets = grids.kuhn_grid(request.param)
    return torch.from_numpy(verts).float().to(cuda), torch.from_numpy(tets).to(cuda), verts.shape[0]


@pytest.fixture(scope="module")
def grid8(cuda):
    verts, tets = grids.kuhn_grid(8)
    pos = torch.from_numpy(grids.jittered_positions(verts, 8, 2)).to(cuda)
    return verts, tets, pos, torch.from_numpy(tets).to(cuda)


# ------------------------------------------------------------------------------------------------ surface operators
@pytest.mark.parametrize("B,N,M", [(9, 65, 300), (1, 1, 1)])
def test_nn_index(cuda, monkeypatch, B, N, M):
    from deftet_amd import hip_ops
    q, p = rnd(1, B, N, 3).to(cuda), rnd(2, B, M, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.nn_index(q, p))


def test_nn_index_ragged_with_an_empty_shape(cuda, monkeypatch):
    from deftet_amd import hip_ops
    q, p = rnd(3, 9, 65, 3).to(cuda), rnd(4, 9, 300, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.nn_index_ragged(q, p, [65, 0, 30, 1, 64, 65, 7, 0, 65]))


def test_tri_dist_fwd(cuda, monkeypatch):
    from deftet_amd import hip_ops
    pts, face = rnd(5, 9, 65, 3).to(cuda), rnd(6, 9, 70, 3, 3).to(cuda)
    nfb = torch.tensor([70, 1, 33, 70, 64, 65, 2, 70, 17], dtype=torch.float32, device=cuda)

    def call():                                                        # the order inside a grid cell is whatever the atomics gave
        d, f, order = hip_ops.tri_dist_fwd(pts, face, nfb, want_order=True)      # (k_tri_point_keys): compared as a permutation
        return d, f, order.sort(1).values
    check_exact(monkeypatch, call)


def test_face_edge_adj_ragged(cuda, monkeypatch):
    """33 shapes (launch groups of 32): a 5 x 7 sheet of quads, two triangles each, so that faces share edges"""
    from deftet_amd import hip_ops
    ix, iy = np.meshgrid(np.arange(5), np.arange(7), indexing="ij")
    a = (ix * 8 + iy).reshape(-1)
    tri = np.concatenate([np.stack([a, a + 8, a + 9], 1), np.stack([a, a + 9, a + 1], 1)], 0)             # [70,3] over a 6 x 8 lattice
    gx, gy = np.meshgrid(np.arange(6), np.arange(8), indexing="ij")
    pts = np.stack([gx, gy, gx * 0], -1).reshape(-1, 3).astype(np.float32)
    face = torch.from_numpy(pts[tri])[None].repeat(33, 1, 1, 1).to(cuda) + torch.arange(33, device=cuda).float().view(33, 1, 1, 1)
    counts = [70, 0] + [int(c) for c in np.random.default_rng(7).integers(0, 71, 30)] + [70]
    check_exact(monkeypatch, lambda: hip_ops.face_edge_adj_ragged(face, counts))
    check_exact(monkeypatch, lambda: hip_ops.face_edge_adj(face[0]))


# ------------------------------------------------------------------------------------------------ builders
def test_tet_adj_share(grid, monkeypatch):
    from deftet_amd import hip_ops
    _, tets, V = grid
    check_exact(monkeypatch, lambda: hip_ops.tet_adj_share(tets, V, tets.device))


def test_tet_to_face(grid, monkeypatch):
    from deftet_amd import hip_ops
    _, tets, V = grid
    check_exact(monkeypatch, lambda: hip_ops.tet_to_face(tets, V, tets.device, with_boundary=True))


@pytest.mark.parametrize("wrap32", [True, False])
def test_tet_face_adj(grid, monkeypatch, wrap32):
    from deftet_amd import hip_ops
    _, tets, V = grid
    check_exact(monkeypatch, lambda: hip_ops.tet_face_adj(tets, V, tets.device, wrap32=wrap32))


def test_tet_point_adj(grid, monkeypatch):
    from deftet_amd import hip_ops
    _, tets, V = grid
    check_exact(monkeypatch, lambda: hip_ops.tet_point_adj(tets, V, tets.device))


def test_colaps_v(grid, monkeypatch):
    from deftet_amd import hip_ops
    verts, _, _ = grid
    pts = torch.cat([verts, verts.flip(0), verts[::2]], 0)                 # every point two or three times
    check_exact(monkeypatch, lambda: hip_ops.colaps_v(pts))


def test_tet_edges(grid, monkeypatch):
    from deftet_amd import hip_ops
    _, tets, V = grid
    check_exact(monkeypatch, lambda: hip_ops.tet_edges(tets.long(), V))


def test_subdivide(grid, monkeypatch):
    from deftet_amd import hip_ops
    verts, tets, V = grid
    T = tets.shape[0]
    feat = rnd(8, V, 2).to(verts.device)
    sig = (rnd(9, T) > 0.5).to(verts.device)
    check_exact(monkeypatch, lambda: hip_ops.subdivide(tets.long(), verts, feat, sig))


def test_delete_tet(grid, monkeypatch):
    from deftet_amd import hip_ops
    _, tets, _ = grid
    w = rnd(10, tets.shape[0], 2).to(tets.device)
    check_exact(monkeypatch, lambda: hip_ops.delete_tet(tets.long(), w, thres=0.5))


def test_tet_neighbours(grid, monkeypatch):
    from deftet_amd import hip_ops
    _, tets, V = grid
    check_exact(monkeypatch, lambda: hip_ops.tet_neighbours(tets, V, tets.device, want_face_owners=True))


# ------------------------------------------------------------------------------------------------ tet operators
@pytest.mark.parametrize("mode", [1, 2])
def test_boundary_index(grid8, cuda, monkeypatch, mode):
    from deftet_amd import hip_ops
    _, tets, _, tets_d = grid8
    f3, t2, _, _, _ = hip_ops.tet_to_face(tets_d, 125, cuda, with_boundary=True)
    occ = (rnd(11, 2, tets.shape[0]) > 0.5).float().to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.boundary_index(f3, t2, occ, mode=mode))


@pytest.mark.parametrize("pow_", [4, 2])
def test_tet_energies(grid8, cuda, monkeypatch, pow_):
    from deftet_amd import hip_ops
    _, tets, pos, _ = grid8
    tet_p = torch.from_numpy(grids.gather_tets(pos.cpu().numpy(), tets)).to(cuda)
    inv = rnd(12, tets.shape[0], 3, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.tet_energies(tet_p, inv, pow_v=pow_, pow_e=pow_))


def test_tet_order_coherence(cuda, monkeypatch):
    from deftet_amd import hip_ops
    tet = rnd(13, 300, 4, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.tet_order_coherence(tet))


# ------------------------------------------------------------------------------------------------ incidence lists
def test_vertex_adjacency_build(cuda, monkeypatch):
    from deftet_amd import hip_ops
    adj = torch.sparse_coo_tensor(rnd_idx(14, 300, 2, 3000), rnd(15, 3000), (300, 300)).to(cuda)       # duplicates stay as stored
    check_exact(monkeypatch, lambda: hip_ops.VertexAdjacency.from_sparse(adj))


def test_tet_vertex_csr(cuda, monkeypatch):
    from deftet_amd import hip_ops
    idx = rnd_idx(16, 125, 600, 4).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.tet_vertex_csr(idx, 125))


def test_face_vertex_csr(cuda, monkeypatch):
    from deftet_amd import hip_ops
    faces = rnd_idx(17, 125, 600, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.FaceTopology(faces, 125))


def test_tet_edges_topology(cuda, monkeypatch):
    from deftet_amd import hip_ops
    tets = torch.from_numpy(np.argsort(np.random.default_rng(18).random((600, 125)), 1)[:, :4].copy()).to(cuda)   # four distinct corners
    check_exact(monkeypatch, lambda: hip_ops.TetEdges(tets, 125))


# ------------------------------------------------------------------------------------------------ meshes
def test_surface_weld(cuda, monkeypatch):
    from deftet_amd import hip_ops
    verts, attrs, faces = rnd(19, 2100, 3).to(cuda), rnd(20, 2100, 3).to(cuda), rnd_idx(21, 2100, 500, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.surface_weld(verts, faces, attrs))


def test_mesh_voxelize(cuda, monkeypatch):
    from deftet_amd import hip_ops
    verts, faces = rnd(22, 2, 200, 3).to(cuda), rnd_idx(23, 200, 300, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.mesh_voxelize(verts, faces, 33))


def test_face_edges(cuda, monkeypatch):
    from deftet_amd import hip_ops
    faces = rnd_idx(24, 250, 400, 3).to(cuda)
    check_exact(monkeypatch, lambda: hip_ops.face_edges(faces, 250))


def test_sample_points(cuda, monkeypatch):
    from deftet_amd import metrics
    fv, u = rnd(25, 2, 1100, 3, 3).to(cuda), rnd(26, 2, 64, 3).to(cuda)
    check_exact(monkeypatch, lambda: metrics.sample_faces(fv, [1100, 700], u))


# ------------------------------------------------------------------------------------------------ grid samplers (cell_gather.hpp)
def test_avg_voxelize(cuda, monkeypatch):
    from deftet_amd import hip_ops
    feat, coords = rnd(32, 2, 3, 2100).to(cuda), rnd_idx(33, 7, 2, 3, 2100).int().to(cuda) - 1          # -1 and 5: outside R = 5
    check_exact(monkeypatch, lambda: hip_ops.avg_voxelize_fwd(feat, coords, 5))


def test_voxel_sample_forward_and_backward(cuda, monkeypatch):
    """the sort of the points by cell and the corner partials of the volume backward, two resolutions"""
    from deftet_amd import hip_ops
    vols0, pos0, gout = [rnd(34, 2, 3, 5, 5, 5).to(cuda), rnd(35, 2, 2, 8, 8, 8).to(cuda)], (1.1 * (rnd(36, 2, 2100, 3) - 0.5)).to(cuda), rnd(37, 2, 5, 2100).to(cuda)

    def call():
        vols, pos = [v.clone().requires_grad_(True) for v in vols0], pos0.clone().requires_grad_(True)
        out = hip_ops.voxel_sample(vols, pos)
        out.backward(gout)
        return out.detach(), pos.grad, [v.grad for v in vols]
    check_exact(monkeypatch, call)


def test_image_sample_forward_and_backward(cuda, monkeypatch):
    from deftet_amd import hip_ops
    maps0, uv0, gout = [rnd(38, 2, 3, 5, 4).to(cuda), rnd(39, 2, 2, 8, 8).to(cuda)], (2.6 * (rnd(40, 2, 2100, 2) - 0.5)).to(cuda), rnd(41, 2, 7, 2100).to(cuda)
    glob0 = rnd(42, 2, 2).to(cuda)

    def call():
        maps, uv, glob = [m.clone().requires_grad_(True) for m in maps0], uv0.clone().requires_grad_(True), glob0.clone().requires_grad_(True)
        out = hip_ops.image_sample(maps, uv, global_features=glob)
        out.backward(gout)
        return out.detach(), uv.grad, glob.grad, [m.grad for m in maps]
    check_exact(monkeypatch, call)


# ------------------------------------------------------------------------------------------------ private workspaces, by the C ABI
@pytest.mark.parametrize("weights", [False, True], ids=["occ", "vertex_weights"])
def test_surface_extract(grid8, cuda, weights):
    from deftet_amd import _lib, hip_ops
    _, tets, pos, _ = grid8
    B, T, V = 2, 257, 125
    tets = tets[:T]
    nbr = hip_ops.tet_face_neighbours(tets, V, cuda)
    tet_p = torch.from_numpy(grids.gather_tets(pos.cpu().numpy(), tets)).to(cuda)
    idx32 = torch.from_numpy(tets).int().to(cuda)
    occ = None if weights else rnd(27, B, T).to(cuda)
    w = rnd(28, B, V).to(cuda) if weights else None
    want = hip_ops.surface_extract(tet_p, occ, nbr, "threshold", thres=0.25, vertex_weights=w, tet_idx=idx32, return_index=True, return_faces=True)
    lib, st, g = _lib.load(), _lib.current_stream(cuda), Guarded()
    wsb = lib.deftet_surface_extract_workspace_bytes(B, T, int(weights))
    ws = g(cuda, wsb)
    offs = torch.empty(B + 1, dtype=torch.int32, device=cuda)
    _lib.check(lib.deftet_surface_extract_count_f32(_lib.ptr(occ), _lib.ptr(w), idx32.data_ptr(), V if weights else 0, nbr.table32.data_ptr(), B,
                                                    T, 1, 0.25, offs.data_ptr(), ws.data_ptr(), wsb, st), "count")
    o = offs.tolist()
    F = o[B]
    assert F > 0 and o == [0] + list(np.cumsum([x.shape[0] for x in want.face]))
    face = torch.empty(F, 3, 3, device=cuda)
    index, faces = (torch.empty(F, k, dtype=torch.int64, device=cuda) for k in (2, 3))
    _lib.check(lib.deftet_surface_extract_fill_f32(tet_p.data_ptr(), None, 0, _lib.ptr(occ), idx32.data_ptr(), nbr.table32.data_ptr(), B, T, 1,
                                                   0.25, F, face.data_ptr(), None, index.data_ptr(), faces.data_ptr(), ws.data_ptr(), wsb, st),
               "fill")
    assert g.blocks and g.intact()
    for got, ref in ((face, want.face), (index, want.index), (faces, want.faces)):
        assert same_bits(got, torch.cat(ref))


@pytest.mark.parametrize("C", [0, 3])
def test_marching_tets(grid8, cuda, C):
    from deftet_amd import _lib, hip_ops
    _, tets, pos, tets_d = grid8
    B, V, T = 2, 125, tets.shape[0]
    top = hip_ops.TetEdges(tets_d, V)
    E = top.n_edge
    field = (rnd(29, B, V) - 0.5).to(cuda)
    attr = rnd(30, B, V, C).to(cuda) if C else None
    want = hip_ops.marching_tets(pos, field, top, iso=0.0, attr=attr, return_index=True)
    lib, st, g = _lib.load(), _lib.current_stream(cuda), Guarded()
    wsb = lib.deftet_marching_tets_workspace_bytes(B, T, E)
    ws = g(cuda, wsb)
    ev = torch.empty(B, E, dtype=torch.int32, device=cuda)
    offs = torch.empty(2, B + 1, dtype=torch.int32, device=cuda)
    _lib.check(lib.deftet_marching_tets_count_f32(field.data_ptr(), top.edges.data_ptr(), top.tets.data_ptr(), B, V, T, E, 0.0, ev.data_ptr(),
                                                  offs.data_ptr(), ws.data_ptr(), wsb, st), "count")
    o = offs.tolist()
    Nv, Nf = o[0][B], o[1][B]
    assert Nv > 0 and Nf > 0
    verts, t = torch.empty(Nv, 3, device=cuda), torch.empty(Nv, device=cuda)
    vattr = torch.empty(Nv, C, device=cuda) if C else None
    faces, edge_id, tet_id = (torch.empty(*s, dtype=torch.int64, device=cuda) for s in ((Nf, 3), (Nv,), (Nf,)))
    _lib.check(lib.deftet_marching_tets_fill_f32(pos.data_ptr(), field.data_ptr(), _lib.ptr(attr), C, top.edges.data_ptr(), top.tets.data_ptr(),
                                                 top.tet_edge.data_ptr(), ev.data_ptr(), B, V, T, E, 0.0, Nv, Nf, verts.data_ptr(), _lib.ptr(vattr),
                                                 faces.data_ptr(), edge_id.data_ptr(), t.data_ptr(), tet_id.data_ptr(), ws.data_ptr(), wsb, st),
               "fill")
    assert g.blocks and g.intact()
    pairs = [(verts, want.verts), (faces, want.faces), (edge_id, want.edge_id), (t, want.t), (tet_id, want.tet_id)]
    if C:
        pairs.append((vattr, want.vert_attr))
    for got, ref in pairs:
        assert same_bits(got, torch.cat(ref))


def test_voxel_surface_mesh(cuda):
    """B = 2, R = 33: (R + 1)^2 rows of two words per shape, so the face and the corner tables both pass one scan tile"""
    from deftet_amd import _lib, hip_ops
    B, R = 2, 33
    ax = torch.arange(R, device=cuda).float() - 16.0
    r2 = ax.view(R, 1, 1) ** 2 + ax.view(1, R, 1) ** 2 + ax.view(1, 1, R) ** 2
    vox = torch.stack([r2 < 14.5 ** 2, (r2 < 9.5 ** 2) | (rnd(31, R, R, R).to(cuda) > 0.97)]).to(torch.uint8)    # a ball; a ball and specks
    bits = hip_ops.voxel_pack(vox)
    want_v, want_f = hip_ops.voxel_surface_mesh(bits)
    lib, st, g = _lib.load(), _lib.current_stream(cuda), Guarded()
    wsb = lib.deftet_voxel_surface_workspace_bytes(B, R)
    ws = g(cuda, wsb)
    offs = torch.empty(2 * (B + 1), dtype=torch.int32, device=cuda)
    _lib.check(lib.deftet_voxel_surface_count_b32(bits.words.data_ptr(), B, R, offs.data_ptr(), ws.data_ptr(), wsb, st), "count")
    o = offs.tolist()
    fo, vo = o[:B + 1], o[B + 1:]
    assert fo[B] > 0 and vo[B] > 0
    assert fo == [0] + list(np.cumsum([x.shape[0] for x in want_f])) and vo == [0] + list(np.cumsum([x.shape[0] for x in want_v]))
    faces = torch.empty(fo[B], 3, dtype=torch.int64, device=cuda)
    verts = torch.empty(vo[B], 3, device=cuda)
    _lib.check(lib.deftet_voxel_surface_fill_b32(bits.words.data_ptr(), B, R, fo[B], vo[B], verts.data_ptr(), faces.data_ptr(), ws.data_ptr(),
                                                 wsb, st), "fill")
    assert g.blocks and g.intact()
    assert same_bits(verts, torch.cat(want_v)) and same_bits(faces, torch.cat(want_f))
