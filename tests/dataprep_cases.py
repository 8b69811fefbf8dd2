"""The shared inputs of tests/test_dataprep_sizes_gpu.py and tests/test_dataprep_cases_cpu.py: the ground-truth preparation
 past its size switches and word widths.  Every input and every reference is made once per process; nobody
writes into what these functions return."""
import functools

import numpy as np

from tests import dataprep_ref as ref

# ---------------------------------------------------------------------------- A: voxelization at 2 x 20,495 faces
VOX_R, VOX_R_NARROW = 65, 33
ZERO_RUN = 6                                                            # faces without a task at either end of the list
# corners in frame units (0..1 is the grid), general floats: every axis starts below 0 and ends above 1, so the candidate box is
# the whole grid: R R W word columns
SPANNING = [[(-0.031, -0.047, 0.213), (1.043, 0.389, -0.029), (0.467, 1.061, 1.037)],
            [(1.029, -0.053, -0.037), (-0.041, 0.611, 1.049), (0.733, 1.057, 0.271)],
            [(-0.059, 1.033, -0.043), (0.317, -0.039, 1.051), (1.047, 0.571, 0.419)]]
OUTSIDE = [(2.13, 2.31, 2.07), (3.19, 2.11, 2.43), (2.37, 3.23, 2.61), (2.71, 2.53, 3.17),      # beyond the far corner
           (-1.31, -2.17, -1.93), (-2.23, -1.19, -1.57), (-1.77, -1.41, -2.39)]                 # before the near one


@functools.lru_cache(maxsize=None)
def voxel_batch():
    """B = 2 spheres of 20,480 faces on one face list, with 15 more faces on 17 more vertices per shape:
      * three triangles across the whole grid (50 tasks each at R = 65) at face 0, mid-list and near the end.  Face 0 is one of
        them in shape 0 only: its corners lie outside the frame in shape 1, whose list therefore STARTS with a run of faces
        without a task, straight after the run that ends shape 0 — both sides of the shape boundary of the task table are zero
        runs, and entry 0 of the table is a split triangle;
      * ZERO_RUN faces without a task after face 0 and ZERO_RUN at the very end: triangles wholly outside the frame (beyond
        either corner of it) and one with a NaN corner between two vertices of the sphere.
    origin / scale are the default frame of each sphere alone.  Returns a dict: verts f32 [2,V,3], faces int64 [F,3], origin,
    scale, span (the three face indices), lead / trail (the index ranges of the zero runs of shape 0)."""
    v0, f = ref.icosphere(5, seed=5)
    v1, f1 = ref.icosphere(5, seed=6, radius=0.3)
    assert f.shape == (20480, 3) and np.array_equal(f, f1)
    sph = np.stack([v0, v1])
    origin, scale = ref.default_frame(sph)
    n0 = sph.shape[1]
    extra = np.asarray([c for t in SPANNING for c in t] + OUTSIDE + [(np.nan, 0.5, 0.5)], np.float64)     # [17,3] in frame units
    ev = np.stack([(origin[b].astype(np.float64)[None, :] + float(scale[b]) * extra).astype(np.float32) for b in range(2)])
    ev[1, 0:3] = (origin[1].astype(np.float64)[None, :] + float(scale[1]) * (extra[0:3] + 3.0)).astype(np.float32)
    verts = np.concatenate([sph, ev], axis=1)
    span = [[n0 + 3 * s, n0 + 3 * s + 1, n0 + 3 * s + 2] for s in range(3)]
    o, nan = n0 + 9, n0 + 16
    far = [[o, o + 1, o + 2], [o + 4, o + 5, o + 6], [o + 1, o + 2, o + 3], [o + 3, o, o + 2], [o + 6, o + 4, o + 5]]
    lead = far + [[5, nan, 77]]
    trail = [[9000, 31, nan]] + far[::-1]
    assert len(lead) == len(trail) == ZERO_RUN
    half, tail = 10240, 20475
    faces = np.concatenate([[span[0]], lead, f[:half], [span[1]], f[half:tail], [span[2]], f[tail:], trail]).astype(np.int64)
    F = faces.shape[0]
    return {"verts": verts, "faces": faces, "origin": origin, "scale": scale, "span": (0, 1 + ZERO_RUN + half, 2 + ZERO_RUN + tail),
            "lead": (1, 1 + ZERO_RUN), "trail": (F - ZERO_RUN, F)}


@functools.lru_cache(maxsize=None)
def voxel_refs(R):
    """(fp32 grid, fp64 grid, margin voxels, tasks [B,F]) of voxel_batch() at R: both shapes at VOX_R, shape 0 alone at
    VOX_R_NARROW, by the vectorised evaluator"""
    c = voxel_batch()
    n = 2 if R == VOX_R else 1
    args = (c["verts"][:n], c["faces"], R, c["origin"][:n], c["scale"][:n])
    v64, near = ref.mesh_voxelize_f64(*args, margin=1e-4, flat=True)
    return ref.mesh_voxelize_f32(*args, flat=True), v64, near, ref.voxelize_tasks(*args)


# ---------------------------------------------------------------------------- B: bit grids at R = 64 .. 97
BIT_RS = (64, 65, 95, 96, 97)                                           # (W, Wc) = (2,3), (3,3), (3,3) full corner word, (3,4), (4,4)
WORD_EDGES = (0, 31, 32, 63, 64, 95, 96)


def planted_positions(R):
    """(single positions, (first, last) pairs with at least one whole word between their words) along an axis of length R"""
    singles = sorted({k for k in WORD_EDGES + (R - 1,) if 0 <= k < R})
    pairs = [(a, b) for a, b in ((0, R - 1), (31, 64), (5, R - 2), (30, 70), (31, 96)) if b < R and (b >> 5) - (a >> 5) >= 2]
    return singles, pairs


@functools.lru_cache(maxsize=None)
def planted_grid(R):
    """uint8 [R,R,R]: a hollow box over 1 .. R-2 along i and j and 0 .. R-1 along k with walls one voxel thick (a row through
    its cavity has bit 0 and bit R-1 only: the cavity crosses every word boundary, and the fill turns every word between into
    0xFFFFFFFF), and on three outer planes of the grid, outside the box, rows along k (in the plane j = 0), along i (j = R-1)
    and along j (i = R-1): one row per single position and one per (first, last) pair of planted_positions, in every second
    line of the plane."""
    g = np.zeros((R, R, R), np.uint8)
    g[1:R - 1, 1:R - 1, :] = 1
    g[2:R - 2, 2:R - 2, 1:R - 1] = 0
    singles, pairs = planted_positions(R)
    rows = [(k,) for k in singles] + pairs
    for n, pos in enumerate(rows):
        line = 2 * n + 1
        assert line < R
        for p in pos:
            g[line, 0, p] = 1                                           # along k
            g[p, R - 1, line] = 1                                       # along i
            g[R - 1, p, line] = 1                                       # along j
    return g


@functools.lru_cache(maxsize=None)
def bit_batches(R):
    """((name, uint8 [2,R,R,R]), ...): B = 2 per call, so that the scanned tables cross a shape boundary"""
    rng = np.random.default_rng(300 + R)
    sparse = (rng.uniform(size=(R, R, R)) < 0.03).astype(np.uint8)
    empty, full, planted = np.zeros((R, R, R), np.uint8), np.ones((R, R, R), np.uint8), planted_grid(R)
    return (("planted+sparse", np.stack([planted, sparse])), ("full+empty", np.stack([full, empty])),
            ("empty+planted", np.stack([empty, planted])))


def words_of(vox):
    """uint32 [..., ceil(R / 32)]: the bit grid of a byte grid, bit k % 32 of word k // 32"""
    v = np.asarray(vox) != 0
    R = v.shape[-1]
    W = (R + 31) // 32
    p = np.zeros(v.shape[:-1] + (W * 32,), np.uint64)
    p[..., :R] = v
    return (p.reshape(v.shape[:-1] + (W, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


# ---------------------------------------------------------------------------- C: the production chain at R = 100
CHAIN_R = 100


@functools.lru_cache(maxsize=None)
def chain_sphere():
    """the true sphere of test_dataprep_gpu.py: (verts f32 [2562,3], faces int64 [5120,3])"""
    v, f = ref.icosphere(4, seed=2, radius=0.37, jitter=0.0)
    assert f.shape == (5120, 3)
    return v + np.float32(0.5), f


def normalise(v, max_length=0.9):
    """dataprep.make_surface_mesh's first lines in numpy, fp32: rescale by the largest extent, centre"""
    v = np.asarray(v, np.float32)
    v = (v / (v.max(axis=0) - v.min(axis=0)).max()) * np.float32(max_length)
    return v - ((v.max(axis=0) + v.min(axis=0)) / np.float32(2))[None, :]


# ---------------------------------------------------------------------------- D: face_edges with wide keys
EDGE_VS = (65535, 65536, 65537, 2097152)
EDGE_KEY_BITS = (32, 33, 33, 43)                                        # bit_length(V^2): four, five, five and six 8-bit passes
EDGE_F = 4000


@functools.lru_cache(maxsize=None)
def edge_faces(V):
    """int64 [4000,3] random faces on V vertices with duplicates, both windings of an edge, self edges, the vertices 0 and V-1
    and the face (V-1, V-2, V-1), whose edge (V-1, V-2) has the largest key a V + b there is"""
    rng = np.random.default_rng(V % 9973)
    f = rng.integers(0, V, size=(EDGE_F, 3), dtype=np.int64)
    f[100:200] = f[0:100]                                               # duplicates
    f[200:300] = f[0:100][:, [1, 0, 2]]                                 # the other winding
    f[300:320, 1] = f[300:320, 0]                                       # (a, a, b)
    f[320:330] = f[320:330, :1]                                         # (a, a, a)
    f[330] = (0, V - 1, 1)
    f[331] = (V - 1, 0, V - 2)
    f[332] = (0, 0, V - 1)
    f[EDGE_F - 1] = (V - 1, V - 2, V - 1)
    return f
