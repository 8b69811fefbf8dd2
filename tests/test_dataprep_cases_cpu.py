"""CPU half of tests/test_dataprep_sizes_gpu.py: the inputs of tests/dataprep_cases.py reach the switches they are there for
(a test there means nothing once they stop), the references alone stay inside the voxelization margin's cap, and the new
restatement code (the vectorised voxelizer, the task counts) agrees with the loop and with the rule text of
include/deftet_hip.h."""
import numpy as np
import pytest

from tests import dataprep_cases as C
from tests import dataprep_ref as ref
from tests.test_dataprep_gpu import exact_mesh

SCAN_SMALL = 8192                                                       # prims::kScanSmall
RASTER_BLOCK_CAP, WAVES_PER_BLOCK = 8192, 4                             # k_vx_raster's grid rule
BUDGET = 256                                                            # DEFTET_VOXELIZE_UNIT_BUDGET


def same_pair(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------- the vectorised evaluator is the loop
@pytest.mark.parametrize("name", ["exact_mesh", "icosphere", "shape0_head"])
def test_flat_evaluator_equals_the_loop_bit_for_bit(name):
    if name == "exact_mesh":
        v, f = exact_mesh()
        cases = [(v, f, R, np.zeros((2, 3), np.float32), np.ones(2, np.float32)) for R in (1, 8, 33, 64)]
    elif name == "icosphere":
        v, f = ref.icosphere(2, seed=5)
        cases = [(v[None], f, R, None, None) for R in (33, 100)]
    else:                                                               # with the spanning triangle, the NaN corner and the outside ones
        c = C.voxel_batch()
        cases = [(c["verts"][:1], c["faces"][:2000], C.VOX_R, c["origin"][:1], c["scale"][:1])]
    for v, f, R, o, s in cases:
        assert same_pair([ref.mesh_voxelize_f32(v, f, R, o, s, flat=True)], [ref.mesh_voxelize_f32(v, f, R, o, s)]), R
        assert same_pair(ref.mesh_voxelize_f64(v, f, R, o, s, flat=True), ref.mesh_voxelize_f64(v, f, R, o, s)), R
        # a small chunk cuts the pair list inside the run of a mesh's triangles: the same grid
        if R <= 33:
            assert same_pair(ref.mesh_voxelize_f64(v, f, R, o, s, flat=True), ref._voxelize_flat(v, f, R, o, s, np.float64, 1e-4, chunk=97)), R


def test_task_counts_follow_the_candidate_rule_of_the_header():
    # one triangle, q = 4 x its coordinates at R = 4: x in [1, 3] -> i + 1 >= 1 and i <= 3 -> i in 0..3 (i = 0 touches at x = 1),
    # y likewise, z = 2 -> k in 1..2 -> one word: 4 * 4 * 1 units, one task at any budget >= 16, 16 tasks at budget 1
    v = np.array([[[0.25, 0.25, 0.5], [0.75, 0.25, 0.5], [0.25, 0.75, 0.5]]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 0, 0]])
    zero, one = np.zeros((1, 3), np.float32), np.ones(1, np.float32)
    assert ref.voxelize_tasks(v, f, 4, zero, one).tolist() == [[1, 0, 1]]             # a bad index: none; a point: its box
    assert ref.voxelize_tasks(v, f, 4, zero, one, budget=1).tolist() == [[16, 0, 4]]   # the point (1,1,2): i, j in 0..1, k in 1..2
    # the whole grid: R R ceil(R / 32) word columns (the bound test_dataprep_gpu.py's exact fixtures state)
    span = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]], np.float32)
    for R in (8, 31, 33, 64, 65, 100):
        assert ref.voxelize_tasks(span, f[:1], R, zero, one).tolist() == [[-(-R * R * ((R + 31) // 32) // BUDGET)]]
    # k in 31..32 touches two words; outside, NaN and inf: none
    two = np.array([[[0.1, 0.1, 31.5 / 64], [0.11, 0.1, 32.5 / 64], [0.1, 0.11, 32.0 / 64]]], np.float32)
    assert ref.voxelize_tasks(two, f[:1], 64, zero, one, budget=1).tolist() == [[2 * 2 * 2]]
    for bad in (np.nan, np.inf):
        w = span.copy()
        w[0, 1, 1] = bad
        assert ref.voxelize_tasks(w, f[:1], 8, zero, one).tolist() == [[0]]
    assert ref.voxelize_tasks(span + 2.5, f[:1], 8, zero, one).tolist() == [[0]]
    assert ref.voxelize_tasks(span - 2.5, f[:1], 8, zero, one).tolist() == [[0]]
    # a triangle with tasks is one with candidates: the fp32 loop sets nothing for a triangle without
    v8, f8 = exact_mesh()
    t = ref.voxelize_tasks(v8, f8, 8, np.zeros((2, 3), np.float32), np.ones(2, np.float32))
    for b in range(2):
        for i in range(f8.shape[0]):
            if t[b, i] == 0:
                assert ref.mesh_voxelize_f32(v8[b:b + 1], f8[i:i + 1], 8, np.zeros((1, 3), np.float32), np.ones(1, np.float32)).sum() == 0


# ---------------------------------------------------------------------------- A
def test_voxel_batch_reaches_the_scan_and_grid_switches():
    c = C.voxel_batch()
    B, F = c["verts"].shape[0], c["faces"].shape[0]
    assert B == 2 and 20400 <= F < 20500
    assert B * F + 1 > SCAN_SMALL                                       # the three-launch scan
    assert B * F >= 4 * RASTER_BLOCK_CAP                                # the grid at its cap: the waves stride over the tasks
    assert 4096 < F < 4 * RASTER_BLOCK_CAP                              # one shape alone: the grid follows the face count
    o, s = ref.default_frame(c["verts"][:, :10242])
    assert np.array_equal(o, c["origin"]) and np.array_equal(s, c["scale"])
    _, _, _, tasks = C.voxel_refs(C.VOX_R)
    print("tasks %d, split %d of %d faces" % (int(tasks.sum()), int((tasks > 1).sum()), B * F))
    assert tasks.sum() > RASTER_BLOCK_CAP * WAVES_PER_BLOCK             # more tasks than waves: task += nwave is taken
    assert (tasks > 1).sum() >= 3
    whole = -(-C.VOX_R * C.VOX_R * 3 // BUDGET)
    assert whole == 50
    a, m, z = c["span"]
    assert a == 0 and abs(m - F // 2) < 16 and F - 16 < z < c["trail"][0]
    assert tasks[0, [a, m, z]].tolist() == [whole] * 3 and tasks[1, [a, m, z]].tolist() == [0, whole, whole]
    # the zero runs: after face 0 and at the very end of shape 0, at the very start and the very end of shape 1
    (l0, l1), (t0, t1) = c["lead"], c["trail"]
    assert l0 == 1 and t1 == F and l1 - l0 >= 6 and t1 - t0 >= 6
    for b in range(2):
        assert not tasks[b, l0:l1].any() and not tasks[b, t0:].any()
        assert tasks[b, l1] > 0 and tasks[b, t0 - 1] > 0                # ... and no longer than intended
    flat = tasks.reshape(-1)
    assert not flat[t0:F + l1].any() and flat[t0 - 1] > 0 and flat[F + l1] > 0       # across the shape boundary of the table
    assert np.isnan(c["verts"][0, c["faces"][l1 - 1]]).any() and np.isnan(c["verts"][1, c["faces"][t0]]).any()
    # every other face is a face of the sphere with one task
    rest = np.ones(F, bool)
    rest[[a, m, z]] = False
    rest[l0:l1] = rest[t0:] = False
    assert rest.sum() == 20480 and (tasks[:, rest] == 1).all()
    # at the narrow grid the spanning triangles are still split: 33 * 33 * 2 word columns
    t33 = C.voxel_refs(C.VOX_R_NARROW)[3]
    assert t33.shape == (1, F) and t33[0, [a, m, z]].tolist() == [-(-33 * 33 * 2 // BUDGET)] * 3


@pytest.mark.parametrize("R", [C.VOX_R, C.VOX_R_NARROW])
def test_voxel_batch_references_stay_inside_the_margin_cap(R):
    v32, v64, near, _ = C.voxel_refs(R)
    for b in range(v32.shape[0]):
        n_set, n_near = int(v32[b].sum()), int(near[b].sum())
        print("shape %d at R=%d: set %d, margin voxels %d (%.2f %%), fp32 != fp64 at %d" %
              (b, R, n_set, n_near, 100.0 * n_near / n_set, int((v32[b] != v64[b]).sum())))
        assert not ((v32[b] != v64[b]) & ~near[b]).any()
        assert n_near <= 0.005 * n_set
        assert n_set > 20000 or R == C.VOX_R_NARROW


# ---------------------------------------------------------------------------- B
@pytest.mark.parametrize("R", C.BIT_RS)
def test_planted_grid_has_what_the_fill_is_tested_on(R):
    g = C.planted_grid(R)
    W, Wc = (R + 31) // 32, (R + 32) // 32
    assert (W, Wc) == {64: (2, 3), 65: (3, 3), 95: (3, 3), 96: (3, 4), 97: (4, 4)}[R]
    singles, pairs = C.planted_positions(R)
    assert set(singles) == {k for k in (0, 31, 32, 63, 64, 95, 96, R - 1) if k < R}
    assert (len(pairs) >= 2) == (R >= 65)
    words = C.words_of(g)                                               # [R,R,W]
    for n, k in enumerate(singles):                                     # the single-bit rows, on all three axes
        line = 2 * n + 1
        assert g[line, 0].sum() == 1 and g[line, 0, k] == 1
        assert g[:, R - 1, line].sum() == 1 and g[k, R - 1, line] == 1
        assert g[R - 1, :, line].sum() == 1 and g[R - 1, k, line] == 1
    for n, (a, b) in enumerate(pairs):                                  # first and last bit with an empty word between them
        line = 2 * (len(singles) + n) + 1
        row = words[line, 0]
        assert g[line, 0].sum() == 2 and row[a >> 5] and row[b >> 5] and not row[(a >> 5) + 1:(b >> 5)].any() and (b >> 5) - (a >> 5) >= 2
        assert np.flatnonzero(g[:, R - 1, line]).tolist() == [a, b] and np.flatnonzero(g[R - 1, :, line]).tolist() == [a, b]
    # a row through the cavity has its first bit in the first word and its last in the last one, every word between is empty:
    # the cavity crosses every word boundary, and the restated fill turns the row into all ones, whole words where R >= 65
    mid = words[R // 2, R // 2]
    assert not g[2:R - 2, 2:R - 2, 1:R - 1].any() and g[R // 2, R // 2, [0, R - 1]].all()
    assert mid[0] == 1 and mid[W - 1] == np.uint32(1) << np.uint32((R - 1) & 31) and not mid[1:W - 1].any()
    filled = ref.project_odms(ref.extract_odms(g[None]))[0]
    assert filled[1:R - 1, 1:R - 1, :].all()
    fw = C.words_of(filled)
    assert (fw[R // 2, R // 2, :W - 1] == 0xFFFFFFFF).all() and fw[R // 2, R // 2, W - 1] == (0xFFFFFFFF >> (31 - ((R - 1) & 31)))
    assert (W >= 3) == (R >= 65)
    if R >= 65:                                                         # an INTERIOR whole word, which the input has nowhere
        assert (fw[2:R - 2, 2:R - 2, 1:W - 1] == 0xFFFFFFFF).all() and not (words[:, :, 1:W - 1] == 0xFFFFFFFF)[2:R - 2, 2:R - 2].any()
    for name, batch in C.bit_batches(R):
        assert batch.shape == (2, R, R, R) and batch.dtype == np.uint8
    sparse = C.bit_batches(R)[0][1][1]
    assert 0.02 < sparse.mean() < 0.04


def test_words_of_packs_as_the_bit_grid_is_defined():
    g = np.zeros((1, 1, 70), np.uint8)
    g[0, 0, [0, 31, 32, 69]] = 1
    assert C.words_of(g).tolist() == [[[0x80000001, 1, 1 << 5]]]


# ---------------------------------------------------------------------------- C
def test_chain_sphere_references_stay_inside_the_margin_cap_at_100():
    v, f = C.chain_sphere()
    n = C.normalise(v)
    assert abs(float((n.max(axis=0) - n.min(axis=0)).max()) - 0.9) < 1e-6 and float(np.abs(n.max(axis=0) + n.min(axis=0)).max()) < 1e-6
    v32 = ref.mesh_voxelize_f32(n[None], f, C.CHAIN_R, flat=True)
    v64, near = ref.mesh_voxelize_f64(n[None], f, C.CHAIN_R, margin=1e-4, flat=True)
    n_set, n_near = int(v32.sum()), int(near.sum())
    print("chain sphere at R=100: set %d, margin voxels %d (%.2f %%), fp32 != fp64 at %d" % (n_set, n_near, 100.0 * n_near / n_set, int((v32 != v64).sum())))
    assert not ((v32 != v64) & ~near).any() and n_near <= 0.005 * n_set and n_set > 40000
    # what the later stages of the chain will see: W = 4, and a surface short of the 65,536-vertex line that D covers
    filled = ref.project_odms(ref.extract_odms(v32))
    sv, sf = ref.voxel_surface_mesh(filled)
    print("filled %d, surface %d vertices, %d faces" % (int(filled.sum()), sv[0].shape[0], sf[0].shape[0]))
    assert filled.sum() > 500000 and 40000 < sv[0].shape[0] < 65536 and 6 * sf[0].shape[0] > 500000


# ---------------------------------------------------------------------------- D
def test_edge_faces_have_the_key_widths_and_the_planted_faces():
    assert len(C.EDGE_VS) == len(C.EDGE_KEY_BITS) == 4
    for V, bits in zip(C.EDGE_VS, C.EDGE_KEY_BITS):
        assert (V * V).bit_length() == bits and (bits + 7) // 8 == {32: 4, 33: 5, 43: 6}[bits]
        f = C.edge_faces(V)
        assert f.shape == (C.EDGE_F, 3) and f.dtype == np.int64 and f.min() == 0 and f.max() == V - 1
        assert f[-1].tolist() == [V - 1, V - 2, V - 1]
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = e[:, 0] * V + e[:, 1]
        proper = e[:, 0] != e[:, 1]
        assert key[proper].max() == (V - 1) * V + (V - 2) == V * V - 2  # just below the sentinel V^2
        assert (~proper).sum() >= 20 + 3 * 10                           # self edges
        assert (f[:, 0] == f[:, 1]).sum() >= 30 and ((f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2])).sum() >= 10
        assert np.unique(f, axis=0).shape[0] <= C.EDGE_F - 100          # duplicate faces
        fwd = set(map(tuple, e[proper].tolist()))
        assert sum((b, a) in fwd for a, b in fwd) >= 200                # both windings of an edge
        p = ref.face_edges(f, V)
        assert p.shape[0] < 6 * C.EDGE_F - 600 and p[0, 0] == 0 and p[-1].tolist() == [V - 1, V - 2]
