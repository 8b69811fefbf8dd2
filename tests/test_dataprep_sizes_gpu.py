"""Ground-truth preparation (dataprep.hip) past its size switches and word widths, against the numpy restatement
tests/dataprep_ref.py on the shared inputs of tests/dataprep_cases.py (whose conditions tests/test_dataprep_cases_cpu.py holds).
No tolerance is new: integers are exact, the voxelization differs from the fp32 restatement only inside the fp64 margin (1e-4
voxel units, at most 0.5 % of the set voxels), the smoothing is within 1e-5 (max-norm) of fp64 — test_dataprep_gpu.py's own.

Per test, the switch it crosses and the lines of dataprep.hip it is there for:
  * test_voxelize_two_large_shapes — B F + 1 = 40,991 > prims::kScanSmall: the task table is scanned by three launches (:624).
    B F >= 32,768: k_vx_raster's grid is at its cap of 8,192 blocks (:630-631) and 41,210 tasks are more than its 32,768
    waves, so `task += nwave` (:177) is taken.  The binary search over the scanned table (:179-183) crosses the shape boundary
    between two runs of faces without a task, lands on entry 0 with 50 tasks, and finds three split triangles per list.
    Each shape alone: 4,096 < F < 32,768, the grid follows the face count (:630).  R = 65: W = 3 words per row (:194-198, :210).
    One reading of the issue is fixed here: "a spanning triangle at face 0" and "a run without a task at the very start" are
    both kept, by the vertices: face 0 spans the grid in shape 0 and lies outside the frame in shape 1, whose list starts
    with the run, straight after the run that ends shape 0; shape 1 alone starts the whole table with it.
  * test_voxelize_the_same_mesh_on_the_narrow_grid — the same 20,495 faces at R = 33, W = 2, B = 1.
  * test_bit_grid_stages — R in {64, 65, 95, 96, 97}: (W, Wc) = (2,3), (3,3), (3,3) with a full last corner word, (3,4), (4,4).
    k_fill_span_k's whole-word branch (:292-295: z == 31 with a == 0, an interior word), the cross-word carries of face_masks
    (:344-345) and k_sf_count_verts (:380) at w >= 2, Wc > W (:382-383) at R = 64 and 96, corner_id's word (:401-402), and B = 2:
    the face and corner tables (:733-737) cross a shape boundary.
  * test_production_chain_at_100 — make_surface_mesh's default resolution, stage by stage: W = 4; 5,120 faces put the raster
    grid between its floor and its cap (:630-631); 40,001 surface words and 577,656 edge keys.
  * test_face_edges_with_wide_keys — V in {65,535, 65,536, 65,537, 2,097,152}: bit_length(V^2) = 32, 33, 33, 43 (:784-785), four,
    five, five and six passes of the radix sort (:787), the largest key V^2 - 2 next to the sentinel V^2 (:471-473, :478).

Measured on an MI355X — the counts the tests print (set / margin / differing voxels; tasks, split triangles):
  2 x 20,495 faces at R = 65: shape 0 41,630 / 74 / 0, shape 1 36,820 / 58 / 0; 41,210 tasks, 5 split; 163,845 corners and
  centroids inside the grid.  The same mesh at R = 33: 9,755 / 23 / 0; 20,507 tasks, 3 split.
  The chain at R = 100: 46,942 / 38 / 0; 546,160 voxels after the fill, 48,140 vertices, 96,276 faces, 577,656 edge keys,
  288,828 directed edges.  face_edges: 24,000 keys, 22,646 unique edges at every V (32, 33, 33, 43 key bits)."""
import numpy as np
import pytest
import torch

from tests import dataprep_cases as C
from tests import dataprep_ref as ref
from tests import tol
from tests.test_dataprep_gpu import check_surface, same

pytestmark = pytest.mark.gpu
_cache = {}


def _t(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def u32(words):
    return words.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------- A
def voxelize(cuda, R, shapes):
    from deftet_amd import hip_ops
    c = C.voxel_batch()
    return hip_ops.mesh_voxelize(_t(c["verts"][shapes], cuda), _t(c["faces"], cuda), R, origin=_t(c["origin"][shapes], cuda),
                                 scale=_t(c["scale"][shapes], cuda), return_bits=True)


def held_to_the_margin(what, got, want, near):
    """got differs from the fp32 restatement only where the fp64 one has a decision inside the margin"""
    for b in range(want.shape[0]):
        diff = got[b] != want[b]
        print("voxelize %s, shape %d: set %d, margin voxels %d, differing %d" % (what, b, int(want[b].sum()), int(near[b].sum()), int(diff.sum())))
        assert near[b].sum() <= 0.005 * want[b].sum()
        assert not (diff & ~near[b]).any()


def corners_and_centroids_are_set(got, R, shapes):
    """conservative: the voxel of every triangle corner and of every centroid inside the grid is set"""
    c = C.voxel_batch()
    n = 0
    for at, b in enumerate(shapes):
        with np.errstate(all="ignore"):
            q = ((c["verts"][b] - c["origin"][b][None, :]) / c["scale"][b]) * np.float32(R)
        tri = q[c["faces"]]                                             # [F,3,3]
        tri = tri[np.isfinite(tri).all(axis=(1, 2))]
        for pts in (tri.reshape(-1, 3).astype(np.float64), tri.astype(np.float64).mean(axis=1)):
            pts = pts[((pts >= 0) & (pts <= R)).all(axis=1)]
            ijk = np.minimum(np.floor(pts).astype(np.int64), R - 1)
            assert got[at, ijk[:, 0], ijk[:, 1], ijk[:, 2]].all()
            n += pts.shape[0]
    return n


def test_voxelize_two_large_shapes(cuda):
    R = C.VOX_R
    want, v64, near, tasks = C.voxel_refs(R)
    assert not ((want != v64) & ~near).any()
    bits = voxelize(cuda, R, [0, 1])
    got = bits.unpack().cpu().numpy()
    assert bits.words.shape == (2, R, R, 3)
    held_to_the_margin("2 x %d faces at R=%d" % (tasks.shape[1], R), got, want, near)
    n = corners_and_centroids_are_set(got, R, [0, 1])
    stats = bits.stats.tolist()
    print("tasks %d, split %d, corners and centroids inside the grid %d" % (stats[0], stats[1], n))
    assert n > 2 * 4 * 20480
    assert stats == [int(tasks.sum()), int((tasks > 1).sum()), 0, 0]
    again = voxelize(cuda, R, [0, 1])
    assert torch.equal(again.words, bits.words) and again.stats.tolist() == stats
    # each shape alone: the grid follows the face count, the table ends (shape 0) or starts (shape 1) with a run without a task
    for b in range(2):
        alone = voxelize(cuda, R, [b])
        assert torch.equal(alone.words, bits.words[b:b + 1]), b
        assert alone.stats.tolist() == [int(tasks[b].sum()), int((tasks[b] > 1).sum()), 0, 0]
    assert int((u32(bits.words)[..., -1] >> (R % 32)).max()) == 0        # the pad bits of the last word


def test_voxelize_the_same_mesh_on_the_narrow_grid(cuda):
    R = C.VOX_R_NARROW
    want, v64, near, tasks = C.voxel_refs(R)
    assert not ((want != v64) & ~near).any()
    bits = voxelize(cuda, R, [0])
    got = bits.unpack().cpu().numpy()
    held_to_the_margin("%d faces at R=%d" % (tasks.shape[1], R), got, want, near)
    corners_and_centroids_are_set(got, R, [0])
    print("tasks %d, split %d" % tuple(bits.stats.tolist()[:2]))
    assert bits.stats.tolist() == [int(tasks.sum()), int((tasks > 1).sum()), 0, 0]


# ---------------------------------------------------------------------------- B
@pytest.mark.parametrize("R", C.BIT_RS)
def test_bit_grid_stages(cuda, R):
    from deftet_amd import hip_ops
    for name, g in C.bit_batches(R):
        t = _t(g, cuda)
        want_o = ref.extract_odms(g)
        odms = hip_ops.extract_odms(t)
        assert odms.dtype == torch.int32 and same(odms, want_o), name
        for votes in (1, 3, 6):
            assert same(hip_ops.project_odms(odms, votes=votes), ref.project_odms(want_o, votes=votes)), (name, votes)
        base = np.roll(g, 1, axis=2) | g
        assert same(hip_ops.project_odms(odms, voxelgrids=_t(base, cuda), votes=2), ref.project_odms(want_o, base, 2)), name
        want_fill = ref.project_odms(want_o)
        bits = hip_ops.voxel_pack(t)
        assert same(u32(bits.words), C.words_of(g)) and same(bits.unpack(), g), name
        filled = hip_ops.voxel_fill(bits)
        assert isinstance(filled, hip_ops.VoxelBits) and same(filled.unpack(), want_fill), name
        assert same(u32(filled.words), C.words_of(want_fill)), name
        assert same(hip_ops.voxel_fill(t), want_fill) and same(hip_ops.project_odms(hip_ops.extract_odms(t)), want_fill), name
        if "planted" in name:
            assert want_fill.sum() > g.sum()
        if R % 32:                                                      # the pad bits of the last word stay zero
            assert int((u32(filled.words)[..., -1] >> (R % 32)).max()) == 0 and int((u32(bits.words)[..., -1] >> (R % 32)).max()) == 0
        gv, gf = check_surface(cuda, g)                                 # from bytes: vertices, faces, volume, edge balance
        bv, bf = hip_ops.voxel_surface_mesh(bits)
        assert all(torch.equal(a, b) for a, b in zip(bv + bf, gv + gf)), name


# ---------------------------------------------------------------------------- C
def test_production_chain_at_100(cuda):
    from deftet_amd import dataprep, hip_ops
    R = C.CHAIN_R
    v_np, f_np = C.chain_sphere()
    v_in, f_in = _t(v_np, cuda), _t(f_np, cuda)
    with torch.no_grad():                                               # make_surface_mesh's own first lines
        v = v_in.float()
        vmin, vmax = v.amin(dim=0), v.amax(dim=0)
        v = (v / (vmax - vmin).amax()) * 0.9
        vmin, vmax = v.amin(dim=0), v.amax(dim=0)
        v = v - ((vmax + vmin) / 2).unsqueeze(0)
    host = v.cpu().numpy()
    # 1: voxelization of the GPU-normalised vertices
    want = ref.mesh_voxelize_f32(host[None], f_np, R, flat=True)
    v64, near = ref.mesh_voxelize_f64(host[None], f_np, R, margin=1e-4, flat=True)
    assert not ((want != v64) & ~near).any()
    bits = hip_ops.mesh_voxelize(v.unsqueeze(0), f_in, R, return_bits=True)
    grid = bits.unpack().cpu().numpy()
    assert bits.words.shape == (1, R, R, 4)
    held_to_the_margin("the chain's sphere at R=%d" % R, grid, want, near)
    # 2: the fill of the GPU's own grid
    filled = hip_ops.voxel_fill(bits)
    filled_np = ref.project_odms(ref.extract_odms(grid))
    assert same(filled.unpack(), filled_np)
    # 3: the surface of the filled bits
    gv, gf = hip_ops.voxel_surface_mesh(filled)
    wv, wf = ref.voxel_surface_mesh(filled_np)
    assert same(gv[0], wv[0]) and same(gf[0], wf[0])
    V = wv[0].shape[0]
    # 4: the adjacency
    adj = hip_ops.VertexAdjacency.from_faces(gf[0], V, normalize=True)
    offs, cols = ref.edge_csr(wf[0], V)
    print("filled %d, surface %d vertices, %d faces, %d edge keys, %d edges" % (int(filled_np.sum()), V, wf[0].shape[0], 6 * wf[0].shape[0], cols.shape[0]))
    assert same(adj.offsets, offs.astype(np.int32)) and same(adj.cols, cols.astype(np.int32))
    deg = np.diff(offs)
    assert deg.min() >= 3 and same(adj.vals, (1.0 / np.repeat(deg, deg)).astype(np.float32))
    # 5: three rounds of the neighbour mean
    sm = dataprep.smooth_vertices(gv[0], adj, 3)
    tol.check_close("smooth_vertices at R=100, 3 rounds", sm, ref.smooth(wv[0], wf[0], 3), maxnorm=1e-5)
    # 6: the whole function is the chain above and the final rescale
    nv, nf = dataprep.make_surface_mesh(v_in, f_in, resolution=R)
    assert torch.equal(nf, gf[0])
    with torch.no_grad():
        omin, omax = v.amin(dim=0), v.amax(dim=0)
        nmin, nmax = sm.amin(dim=0), sm.amax(dim=0)
        chained = ((sm - nmin) / (nmax - nmin)) * (omax - omin) + omin
    assert torch.equal(nv, chained)


# ---------------------------------------------------------------------------- D
@pytest.mark.parametrize("V", C.EDGE_VS)
def test_face_edges_with_wide_keys(cuda, V):
    from deftet_amd import hip_ops
    f = C.edge_faces(V)
    tf = _t(f, cuda)
    want = ref.face_edges(f, V)
    got = hip_ops.face_edges(tf, V)
    print("face_edges V=%d: %d key bits, %d keys, %d unique edges" % (V, (V * V).bit_length(), 6 * f.shape[0], want.shape[0]))
    assert got.dtype == torch.int32 and same(got, want.astype(np.int32))
    offs, cols = ref.edge_csr(f, V)
    deg = np.diff(offs)
    for normalize in (True, False):
        adj = hip_ops.VertexAdjacency.from_faces(tf, V, normalize=normalize)
        assert same(adj.offsets, offs.astype(np.int32)) and same(adj.cols, cols.astype(np.int32)), normalize
        assert same(adj.vals, (1.0 / np.repeat(deg, deg)).astype(np.float32) if normalize else np.ones(cols.shape[0], np.float32)), normalize
    with pytest.raises(RuntimeError, match="outside"):
        hip_ops.face_edges(torch.tensor([[0, 1, V]], device=cuda), V)
