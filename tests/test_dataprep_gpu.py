"""Ground-truth preparation on the GPU against the numpy restatement tests/dataprep_ref.py: bit equality wherever
the rule is exact, the fp64 margin where it is not, and closedness / volume / occupancy properties of the surface.  PARITY
UNPINNED against Kaolin: the semantics are this library's own.

Two readings of the issue text are fixed here, with their reasons:
  * check_sign is asked at the voxel centres moved by (0, 1/8, 1/16): check_sign's ray runs along +i and its Möller-Trumbore
    test is closed (oracle/deftet_oracle_sign.c: u >= 0, v >= 0, u + v <= 1), and the centre of a voxel projects onto the centre
    of every -i / +i quad, which lies on the diagonal both of its triangles share — there both triangles count and the parity is
    that of twice the crossings.  The moved points are inside the same voxels and off every diagonal and lattice line.
  * the end-to-end input is the welded surface of a sphere occupancy (r = 0.3) on kuhn_grid(8): four cells a side, 48 tets,
    48 faces — the 2 x 2 x 2 block of cells about the centre, a cube.  It cannot carry a bound against |p| - r that is tighter
    than its own cell (0.45 in the output's units), so on it the remesh is closed, has the input's box, and is held against the
    cube's own signed distance (a formula) within delta = 3 voxels of the remesh grid: the conservative voxelization grows the
    surface by at most a voxel diagonal (1.74), three rounds of neighbour means over unit edges move a vertex by less than
    one voxel, and the rescaling to the input's box takes the growth back; 1.74 + 1 rounded up.  The issue's bounds against
    |p| - r are asserted on a sphere that is one: the icosahedron subdivided four times."""
import sys

import numpy as np
import pytest
import torch

from deftet_amd import grids
from tests import dataprep_ref as ref
from tests import tol

pytestmark = pytest.mark.gpu
_cache = {}


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------- voxelization, exact fixtures
def exact_mesh():
    """B = 2 shapes sharing one face list; vertices are multiples of 2^-6 (the second shape: the first mirrored in x and moved by 2^-6 in y)"""
    tris = [[(0.25, 0.25, 0.5), (0.75, 0.25, 0.5), (0.25, 0.75, 0.5)],                 # in the lattice plane k = R / 2 (even R)
            [(0.0, 0.0, 1.0), (0.5, 0.0, 1.0), (0.0, 0.5, 1.0)],                       # in the last lattice plane of the grid
            [(0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (0.0, 1.0, 1.0)],                       # spans the whole grid
            [(0.25, 0.25, 0.25), (0.75, 0.75, 0.75), (0.5, 0.5, 0.5)],                 # zero area
            [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, -0.5, 0.75)],                     # partly outside
            [(0.125, 0.125, 0.125), (float("nan"), 0.25, 0.125), (0.125, 0.25, 0.25)],  # a NaN corner
            [(2.0, 2.0, 2.0), (3.0, 2.0, 2.0), (2.0, 3.0, 2.5)],                       # outside
            [(0.015625, 0.984375, 0.328125), (0.515625, 0.0625, 0.921875), (0.890625, 0.671875, 0.046875)]]
    v0 = np.asarray(tris, np.float32).reshape(-1, 3)
    v1 = v0.copy()
    v1[:, 0] = 1.0 - v1[:, 0]
    v1[:, 1] = v1[:, 1] + 0.015625
    return np.stack([v0, v1]), np.arange(v0.shape[0]).reshape(-1, 3)


@pytest.mark.parametrize("R", [1, 8, 31, 32, 33, 64])
def test_voxelize_is_bit_equal_on_exact_fixtures(cuda, R):
    from deftet_amd import hip_ops
    v, f = exact_mesh()
    origin, scale = np.zeros((2, 3), np.float32), np.ones(2, np.float32)
    want = ref.mesh_voxelize_f32(v, f, R, origin, scale)
    tv, tf = torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda)
    to, ts = torch.from_numpy(origin).to(cuda), torch.from_numpy(scale).to(cuda)
    got = hip_ops.mesh_voxelize(tv, tf, R, origin=to, scale=ts)
    assert got.dtype == torch.uint8 and same(got, want)
    assert want[0].sum() > 0 and want[1].sum() > 0 and (R == 1 or not np.array_equal(want[0], want[1]))
    bits = hip_ops.mesh_voxelize(tv, tf, R, origin=to, scale=ts, return_bits=True)
    assert same(bits.unpack(), want) and same(hip_ops.voxel_pack(got).words, bits.words.cpu().numpy())
    n_task, n_split, bad, _ = bits.stats.tolist()
    # the spanning triangle has R * R * ceil(R / 32) word columns: beyond the budget it must have been cut into several tasks
    spans = R * R * ((R + 31) // 32) > hip_ops.VOXELIZE_UNIT_BUDGET
    assert bad == 0 and (n_split >= 2 if spans else n_split == 0) and n_task >= 12 + (2 if spans else 0)
    assert spans == (R >= 31)
    again = hip_ops.mesh_voxelize(tv, tf, R, origin=to, scale=ts)
    assert torch.equal(got, again)
    # F = 0, and a face index out of range
    none = hip_ops.mesh_voxelize(tv, tf[:0], R, origin=to, scale=ts)
    assert none.shape == (2, R, R, R) and int(none.sum()) == 0
    oob = hip_ops.mesh_voxelize(tv, torch.tensor([[0, 1, 99]], device=cuda), R, origin=to, scale=ts, return_bits=True)
    assert oob.stats.tolist()[2] == 1 and int(oob.words.ne(0).sum()) == 0


def test_kaolin_named_voxelizer_returns_float_and_uses_the_default_frame(cuda):
    from deftet_amd import dataprep
    v, f = exact_mesh()
    v = np.nan_to_num(v[:1], nan=0.25)
    got = dataprep.trianglemeshes_to_voxelgrids(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda), 8)
    assert got.dtype == torch.float32 and same(got.to(torch.uint8), ref.mesh_voxelize_f32(v, f, 8))


# ---------------------------------------------------------------------------- voxelization, general floats
def sphere_surface(cuda, res=8, r=0.3):
    """the welded surface_extract of a sphere occupancy on kuhn_grid(res): (verts f32 [V,3], faces int64 [F,3]) on the GPU"""
    from deftet_amd import hip_ops
    key = ("sphere", res, r)
    if key not in _cache:
        verts, tets = grids.kuhn_grid(res)
        nbr = hip_ops.tet_face_neighbours(tets, verts.shape[0], cuda)
        pos = np.ascontiguousarray(verts[None], np.float32)
        tet_p = torch.from_numpy(grids.gather_tets(pos, tets)).to(cuda)
        occ = ((tet_p.mean(dim=2) - 0.5).norm(dim=-1) < r).float()
        soup = hip_ops.surface_extract(tet_p, occ, nbr, "binary", tet_idx=torch.from_numpy(tets.astype(np.int64)), return_faces=True)
        v, _a, f, _old = hip_ops.surface_weld(torch.from_numpy(pos[0]).to(cuda), soup.faces[0])
        assert f.shape[0] == 48                                         # four cells a side: 48 tets inside, 48 boundary faces
        _cache[key] = (v, f)
    return _cache[key]


def general_inputs(cuda, name):
    if name == "icosphere":
        return ref.icosphere(2, seed=5)
    v, f = sphere_surface(cuda)
    rng = np.random.default_rng(11)                                     # off the lattice: general floats
    return (v.cpu().numpy() * np.float32(0.83) + rng.uniform(-0.004, 0.004, tuple(v.shape)).astype(np.float32)), f.cpu().numpy()


@pytest.mark.parametrize("R", [33, 100])
@pytest.mark.parametrize("name", ["icosphere", "sphere_surface"])
def test_voxelize_general_floats_differs_only_inside_the_fp64_margin(cuda, name, R):
    from deftet_amd import hip_ops
    v, f = general_inputs(cuda, name)
    want = ref.mesh_voxelize_f32(v[None], f, R)
    v64, near = ref.mesh_voxelize_f64(v[None], f, R, margin=1e-4)
    n_set = int(want.sum())
    # the references themselves first: fp32 against fp64 inside the margin, and the margin voxels under the cap
    assert not ((want != v64) & ~near).any()
    assert near.sum() <= 0.005 * n_set, (int(near.sum()), n_set)
    got = hip_ops.mesh_voxelize(torch.from_numpy(v[None]).to(cuda), torch.from_numpy(f).to(cuda), R).cpu().numpy()
    diff = got != want
    print("voxelize %s R=%d: set %d, margin voxels %d, differing %d" % (name, R, n_set, int(near.sum()), int(diff.sum())))
    assert not (diff & ~near).any()
    # conservative: the voxel of every triangle vertex and of every centroid is set
    o, s = ref.default_frame(v[None])
    q = ((v - o[0][None, :]) / s[0]) * np.float32(R)
    cent = q[f].astype(np.float64).mean(axis=1)
    for pts in (q[np.unique(f)], cent):
        ijk = np.clip(np.floor(pts).astype(np.int64), 0, R - 1)
        assert got[0, ijk[:, 0], ijk[:, 1], ijk[:, 2]].all()


# ---------------------------------------------------------------------------- depth maps, projection, fill
def grids_for(R):
    rng = np.random.default_rng(100 + R)
    out = {"random": (rng.uniform(size=(2, R, R, R)) < 0.3).astype(np.uint8), "empty": np.zeros((1, R, R, R), np.uint8),
           "full": np.ones((1, R, R, R), np.uint8)}
    if R >= 5:
        shell = np.zeros((1, R, R, R), np.uint8)
        shell[0, 1:R - 1, 1:R - 2, 2:R - 1] = 1
        shell[0, 2:R - 2, 2:R - 3, 3:R - 2] = 0
        out["shell"] = shell
    return out


@pytest.mark.parametrize("R", [1, 31, 32, 33])
def test_odms_projection_and_fill_are_bit_equal(cuda, R):
    from deftet_amd import dataprep, hip_ops
    for name, g in grids_for(R).items():
        t = torch.from_numpy(g).to(cuda)
        want_o = ref.extract_odms(g)
        odms = hip_ops.extract_odms(t)
        assert odms.dtype == torch.int32 and same(odms, want_o), name
        assert same(dataprep.extract_odms(t.float()), want_o), name
        for votes in (1, 3, 6):
            assert same(hip_ops.project_odms(odms, votes=votes), ref.project_odms(want_o, votes=votes)), (name, votes)
        base = np.roll(g, 1, axis=2) | g
        assert same(hip_ops.project_odms(odms, voxelgrids=torch.from_numpy(base).to(cuda), votes=2), ref.project_odms(want_o, base, 2)), name
        want_fill = ref.project_odms(want_o)
        bits = hip_ops.voxel_pack(t)
        assert same(bits.unpack(), g), name
        filled = hip_ops.voxel_fill(bits)
        assert isinstance(filled, hip_ops.VoxelBits) and same(filled.unpack(), want_fill), name
        assert same(hip_ops.voxel_fill(t), want_fill) and same(hip_ops.project_odms(hip_ops.extract_odms(t)), want_fill), name
        if name == "shell":
            assert want_fill.sum() > g.sum()
        pad = R % 32
        if pad:                                                         # the pad bits of the last word stay zero
            assert int((filled.words[..., -1].cpu().numpy().view(np.uint32) >> pad).max()) == 0


# ---------------------------------------------------------------------------- surface
def contact(kind, R=4):
    v = np.zeros((1, R, R, R), np.uint8)
    v[0, 1, 1, 1] = v[0][(2, 2, 1) if kind == "edge" else (2, 2, 2)] = 1
    return v


def moved_centres(R):
    i = np.arange(R, dtype=np.float32)
    c = np.stack(np.meshgrid(i, i, i, indexing="ij"), axis=-1).reshape(-1, 3)
    return c + np.array([0.5, 0.625, 0.5625], np.float32)


def check_surface(cuda, g, iso=0.5):
    from deftet_amd import hip_ops
    wv, wf = ref.voxel_surface_mesh(g, iso)
    gv, gf = hip_ops.voxel_surface_mesh(torch.from_numpy(g).to(cuda), iso_value=iso)
    B, R = g.shape[0], g.shape[1]
    assert len(gv) == len(gf) == B
    for b in range(B):
        assert gv[b].dtype == torch.float32 and gf[b].dtype == torch.int64
        assert same(gv[b], wv[b]) and same(gf[b], wf[b]), b
        v, f = gv[b].cpu().numpy(), gf[b].cpu().numpy()
        n_occ = int((g[b] > iso).sum())
        assert ref.signed_volume(v, f) == float(n_occ)
        assert ref.directed_edge_imbalance(f) == 0
        if n_occ and R <= 33:
            pts = torch.from_numpy(moved_centres(R)).to(cuda)[None]
            inside = hip_ops.check_sign(gv[b][None], gf[b], pts)
            assert same(inside[0].view(torch.uint8).cpu().numpy().reshape(R, R, R), (g[b] > iso).astype(np.uint8)), b
    return gv, gf


@pytest.mark.parametrize("R", [1, 31, 32, 33])
def test_surface_mesh_is_bit_equal_closed_and_encloses_the_voxels(cuda, R):
    for name, g in grids_for(R).items():
        check_surface(cuda, g)


def test_surface_mesh_contacts_batch_with_an_empty_shape_and_iso_value(cuda):
    from deftet_amd import dataprep, hip_ops
    check_surface(cuda, contact("edge"))
    check_surface(cuda, contact("corner"))
    rng = np.random.default_rng(3)
    g = (rng.uniform(size=(3, 9, 9, 9)) < 0.3).astype(np.uint8)
    g[1] = 0
    gv, gf = check_surface(cuda, g)
    assert gv[1].shape == (0, 3) and gf[1].shape == (0, 3)
    fl = rng.uniform(size=(1, 6, 6, 6)).astype(np.float32)
    check_surface(cuda, fl, iso=0.7)
    kv, kf = dataprep.voxelgrids_to_trianglemeshes(torch.from_numpy(fl).to(cuda))
    wv, wf = ref.voxel_surface_mesh(fl, 0.5)
    assert same(kv[0], wv[0]) and same(kf[0], wf[0])
    bits = hip_ops.voxel_pack(torch.from_numpy(g).to(cuda))
    bv, bf = hip_ops.voxel_surface_mesh(bits)
    assert all(torch.equal(a, b) for a, b in zip(bv + bf, gv + gf))


# ---------------------------------------------------------------------------- adjacency and smoothing
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def test_from_faces_csr_and_smoothing(cuda):
    from deftet_amd import dataprep, hip_ops
    g = grids_for(9)["random"][:1]
    cv, cf = ref.voxel_surface_mesh(g)
    for faces, V in ((TET, 5), (cf[0], cv[0].shape[0]), (np.array([[0, 0, 1], [1, 2, 2]]), 3)):
        adj = hip_ops.VertexAdjacency.from_faces(torch.from_numpy(faces).to(cuda), V, normalize=True)
        offs, cols = ref.edge_csr(faces, V)
        assert same(adj.offsets, offs.astype(np.int32)) and same(adj.cols, cols.astype(np.int32))
        deg = np.diff(offs)
        assert same(adj.vals, (1.0 / deg[ref.face_edges(faces, V)[:, 0]]).astype(np.float32))
        ones = hip_ops.VertexAdjacency.from_faces(torch.from_numpy(faces).to(cuda), V, normalize=False)
        assert same(ones.cols, cols.astype(np.int32)) and bool((ones.vals == 1).all())
        dense = dataprep.adjacency_matrix(V, torch.from_numpy(faces).to(cuda)).to_dense().cpu().numpy()
        want = np.zeros((V, V), np.float32)
        p = ref.face_edges(faces, V)
        want[p[:, 0], p[:, 1]] = 1
        assert np.array_equal(dense, want)
    with pytest.raises(RuntimeError, match="outside"):
        hip_ops.face_edges(torch.tensor([[0, 1, 7]], device=cuda), 3)
    assert hip_ops.face_edges(torch.zeros(0, 3, dtype=torch.long, device=cuda), 3).shape == (0, 2)
    # the neighbour mean against float64, three rounds
    V = cv[0].shape[0]
    adj = hip_ops.VertexAdjacency.from_faces(torch.from_numpy(cf[0]).to(cuda), V)
    got = dataprep.smooth_vertices(torch.from_numpy(cv[0]).to(cuda), adj, 3)
    tol.check_close("smooth_vertices, 3 rounds", got, ref.smooth(cv[0], cf[0], 3), maxnorm=1e-5)
    # every degree a power of two (an octahedron: 4; no triangulated cube has that, its degrees sum to 36 over 8 corners): exact
    adj = hip_ops.VertexAdjacency.from_faces(torch.from_numpy(OCTA_F).to(cuda), 6)
    got = dataprep.smooth_vertices(torch.from_numpy(OCTA_V * np.float32(3) + np.float32(0.25) * OCTA_V[::-1]).to(cuda), adj, 3)
    assert same(got, ref.smooth(OCTA_V * np.float32(3) + np.float32(0.25) * OCTA_V[::-1], OCTA_F, 3).astype(np.float32))
    cube_v, cube_f = ref.voxel_surface_mesh(np.ones((1, 1, 1, 1), np.uint8))
    adj = hip_ops.VertexAdjacency.from_faces(torch.from_numpy(cube_f[0]).to(cuda), 8)
    assert sorted(np.diff(adj.offsets.cpu().numpy()).tolist()) == [4, 4, 4, 4, 4, 4, 6, 6]
    tol.check_close("smooth_vertices, cube", dataprep.smooth_vertices(torch.from_numpy(cube_v[0]).to(cuda), adj, 3),
                    ref.smooth(cube_v[0], cube_f[0], 3), maxnorm=1e-5)


# ---------------------------------------------------------------------------- end to end
def centred_input(v):
    v = v.double()
    v = v / (v.amax(0) - v.amin(0)).amax() * 0.9
    return v - (v.amax(0) + v.amin(0)) / 2


def held_against(what, got, d0, delta, sign_beyond, min_far, min_far_inside):
    """got: mesh_to_sdf of a remesh; d0: the signed distance it is compared with, > 0 outside, from a formula that does not go
    through the library.  The sign is asserted wherever |d0| > sign_beyond, the magnitude everywhere against d0 SQUARED (the
    reference's quirk): a surface within delta of the one d0 belongs to moves the distance by e, |e| <= delta, and
    |(d0 - e)^2 - d0^2| <= delta (2 |d0| + delta)."""
    far = np.abs(d0) > sign_beyond
    err, bound = np.abs(np.abs(got) - d0 ** 2), delta * (2 * np.abs(d0) + delta)
    print("mesh_to_sdf against %s: %d far points (%d inside), sign errors %d, worst error over its bound %.3f, bound at the worst %.3g" %
          (what, int(far.sum()), int((d0[far] < 0).sum()), int(((got[far] > 0) != (d0[far] < 0)).sum()), float((err / bound).max()),
           float(bound[np.argmax(err / bound)])))
    # the statement must not be empty, and the squared distance must be told from the plain one: |d0| - d0^2 beyond the bound
    assert far.sum() >= min_far and (d0[far] < 0).sum() >= min_far_inside
    assert ((np.abs(d0) - d0 ** 2) > 2 * bound).sum() >= min_far // 2
    assert np.array_equal(got[far] > 0, d0[far] < 0)                    # positive inside (2 check_sign - 1)
    assert (err <= bound).all()


def sample_points(cuda, seed):
    return (1.05 * (torch.rand(1, 4096, 3, generator=torch.Generator().manual_seed(seed)) - 0.5)).to(cuda)


@pytest.mark.parametrize("R", [33, 100])
def test_make_surface_mesh_and_sdf_end_to_end(cuda, R):
    """the res-8 input is the 2 x 2 x 2 block of cells about the centre: a CUBE, of side 0.9 about the origin once centred.  Its
    signed distance is a formula, and the remesh is held against it in voxels of the remesh grid (delta = 3 voxels, the module
    text); the bounds of the issue against |p| - r are asserted on a real sphere in the test below, where they say something
    (here a cell is 0.45 and no sample point is 1.5 cells from the sphere)."""
    from deftet_amd import dataprep
    v_in, f_in = sphere_surface(cuda)
    nv, nf = dataprep.make_surface_mesh(v_in, f_in, resolution=R)
    assert nv.is_cuda and nf.is_cuda and nv.dtype == torch.float32 and nf.dtype == torch.int64 and nf.shape[0] > 6 * R
    assert ref.directed_edge_imbalance(nf.cpu().numpy()) == 0           # closed, by edge parity
    c = centred_input(v_in)
    assert float((nv.double().amin(0) - c.amin(0)).abs().max()) <= 1e-6 and float((nv.double().amax(0) - c.amax(0)).abs().max()) <= 1e-6
    # every input vertex lies on the cube |x|_inf = 0.45, and the 48 faces are its 6 sides of 4 cell faces of 2 triangles
    assert float((c.abs().amax(dim=1) - 0.45).abs().max()) <= 1e-12
    pts = sample_points(cuda, R)
    sdf = dataprep.mesh_to_sdf(nv[None], nf, pts)
    assert sdf.shape == (1, 4096) and sdf.dtype == torch.float32
    q = np.abs(pts[0].cpu().numpy().astype(np.float64)) - 0.45
    d_cube = np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)
    voxel = 0.9 / R
    held_against("the cube it was made from, R=%d" % R, sdf[0].cpu().numpy().astype(np.float64), d_cube, 3.0 * voxel, 2.25 * voxel, 2000, 50)


@pytest.mark.parametrize("R", [33, 100])
def test_remeshed_sphere_has_the_sign_and_squared_distance_of_the_sphere(cuda, R):
    """A real sphere (the icosahedron subdivided four times, every vertex ON the sphere, turned by a random rotation: 5,120 faces
    whose planes stay within r (1 - cos 2.3 deg) < 0.05 voxels of it at R = 100) through make_surface_mesh, then mesh_to_sdf on
    4,096 points 1.05 (U - 0.5): the sign of |p| - r beyond 1.5 voxels and | |sdf| - (|p| - r)^2 | within
    (2 / R) (2 | |p| - r | + 2 / R), the voxel being that of the remesh grid in the output's units (0.9 / R; 2 / R is 2.2 of them).
    Centre and radius go through the same rescaling and centring as the mesh, in float64."""
    from deftet_amd import dataprep
    key = "true sphere"
    if key not in _cache:
        v, f = ref.icosphere(4, seed=2, radius=0.37, jitter=0.0)
        assert f.shape[0] == 5120 and float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.37).max()) < 2e-7
        _cache[key] = (torch.from_numpy(v + np.float32(0.5)).to(cuda), torch.from_numpy(f).to(cuda))
    v_in, f_in = _cache[key]
    nv, nf = dataprep.make_surface_mesh(v_in, f_in, resolution=R)
    assert ref.directed_edge_imbalance(nf.cpu().numpy()) == 0
    c = centred_input(v_in)
    assert float((nv.double().amin(0) - c.amin(0)).abs().max()) <= 1e-6 and float((nv.double().amax(0) - c.amax(0)).abs().max()) <= 1e-6
    s = 0.9 / float((v_in.double().amax(0) - v_in.double().amin(0)).amax())
    mid = (v_in.double().amax(0) + v_in.double().amin(0)) * s / 2
    centre, r = (0.5 * s - mid).cpu().numpy(), 0.37 * s
    pts = sample_points(cuda, 1000 + R)
    got = dataprep.mesh_to_sdf(nv[None], nf, pts)[0].cpu().numpy().astype(np.float64)
    d_sphere = np.linalg.norm(pts[0].cpu().numpy().astype(np.float64) - centre[None, :], axis=1) - r
    held_against("the sphere, R=%d (r = %.4f)" % (R, r), got, d_sphere, 2.0 / R, 1.5 * 0.9 / R, 3000, 500)


def test_dataloader_shaped_caller_runs_through_the_overlay(cuda):
    from deftet_amd import dataprep, overlay
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "kaolin" or k.startswith("kaolin.")}
    names = overlay.install(kaolin=True)
    try:
        from tests import dataprep_callers
        v_in, f_in = sphere_surface(cuda)
        nv, nf = dataprep_callers.make_surface_mesh(v_in, f_in, resolution=33)
        ov, of = dataprep.make_surface_mesh(v_in, f_in, resolution=33)
        assert torch.equal(nf, of)                                      # the same voxels, fill and surface
        tol.check_close("caller against make_surface_mesh", nv, ov, maxnorm=1e-5)
        n = dataprep_callers.unit_normals(nv[None], nf)
        assert n.shape == (1, nf.shape[0], 3) and float((n.norm(dim=-1) - 1).abs().max()) < 1e-5
        pts = sample_points(cuda, 7)
        assert torch.equal(dataprep_callers.kaolin_mesh_to_sdf(ov[None], of, pts), dataprep.mesh_to_sdf(ov[None], of, pts))
    finally:
        overlay.uninstall(names)
        sys.modules.update(saved)
