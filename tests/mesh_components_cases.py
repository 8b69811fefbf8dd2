"""The meshes of the mesh-component tests (tests/test_mesh_components_cpu.py, tests/test_mesh_components_gpu.py): the smallest
shapes where each stage can go wrong.  A case is (verts float32 [V,3], faces int64 [F,3]); V may exceed the vertices in use."""
import functools

import numpy as np

from tests import loop_subdiv_cases as LK

_mesh = LK._mesh

FROM_LOOP = ("tetrahedron", "book", "bowtie", "flat_patch", "big_index", "two_copies", "sphere20")
HOLLOW_ROWS = ((72, 2.5e-4), (5960, 0.1935), (1716, -0.0324), (288, 1.7e-3), (204, 1.1e-3))    # (faces, volume) in label order


def empty():
    return _mesh(np.zeros((4, 3)), np.zeros((0, 3), np.int64))


def single():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def same_way():
    """two faces on the edge (0,1), both running 0 -> 1: one misoriented edge"""
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0.5]], [[0, 1, 2], [0, 1, 3]])


def closed_strip(n):
    """one piece of n faces.  n = 2: a two-sided triangle; n even: a bipyramid over n/2 rim vertices, closed and oriented; an
    odd n cannot close (3 n = 2 E), so an odd piece is an open fan of n faces around a hub"""
    if n == 1:
        return single()
    if n == 2:
        v = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
        return _mesh(v, [[0, 1, 2], [0, 2, 1]])
    if n % 2:
        return LK.fan(n + 1, False)
    m = n // 2
    t = 2 * np.pi * np.arange(m) / m
    v = np.concatenate([[[0, 0, 0.7], [0, 0, -0.6]], np.stack([np.cos(t), np.sin(t), 0.05 * np.cos(2 * t)], 1)])
    up = [[0, 2 + k, 2 + (k + 1) % m] for k in range(m)]
    down = [[1, 2 + (k + 1) % m, 2 + k] for k in range(m)]
    return _mesh(v, up + down)


CHUNK_SIZES = (1, 2, 255, 256, 257, 513, 70_000)


@functools.lru_cache(maxsize=None)
def chunks():
    """disjoint pieces of 1, 2, 255, 256, 257, 513 and 70,000 faces in one list — closed bipyramids where the count is even, open
    fans where it is odd — with the FACE numbering a seeded random permutation: chunk boundaries and the many-chunk sum of the
    measures, deep union-find chains and workgroup boundaries in one mesh.  Pieces are shifted apart and scaled differently."""
    vs, fs, off = [], [], 0
    for k, n in enumerate(CHUNK_SIZES):
        v, f = closed_strip(n)
        vs.append(v * np.float32(0.5 + 0.25 * k) + np.float32(3.0 * k))
        fs.append(f + off)
        off += v.shape[0]
    f = np.concatenate(fs)
    return _mesh(np.concatenate(vs), f[np.random.default_rng(11).permutation(f.shape[0])])


@functools.lru_cache(maxsize=None)
def singles():
    """5,000 disjoint single triangles"""
    n = 5000
    rng = np.random.default_rng(12)
    v = rng.normal(size=(3 * n, 3)) + np.repeat(np.arange(n), 3)[:, None] * 0.01
    return _mesh(v, np.arange(3 * n).reshape(n, 3))


def hollow_field(pos_vx3):
    """max(min(0.36 - r, r - 0.20), ball((0,0,0), 0.08), ball((.4,.4,.4), 0.07), ball((-.41,.4,-.4), 0.05)) in float32,
    ball(c, rho) = rho - |x - c|: a hollow ball, a floater in its void and two floaters in the corners"""
    p = np.asarray(pos_vx3, np.float32)

    def dist(c):
        return np.sqrt(((p - np.asarray(c, np.float32)) ** 2).sum(-1, dtype=np.float32)).astype(np.float32)
    r = dist((0, 0, 0))
    shell = np.minimum(np.float32(0.36) - r, r - np.float32(0.20))
    balls = [np.float32(rho) - dist(c) for c, rho in (((0, 0, 0), 0.08), ((.4, .4, .4), 0.07), ((-.41, .4, -.4), 0.05))]
    return np.maximum.reduce([shell] + balls).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hollow_grid(res=40):
    """(pos [1,V,3], tets, edges, tet_edge, field [V]) of the hollow scene on marching_tets_cases.grid(res, 1)"""
    from tests import marching_tets_cases as MK
    pos, tets, edges, tet_edge = MK.grid(res, 1)
    field = hollow_field(pos[0])
    field.setflags(write=False)
    return pos, tets, edges, tet_edge, field


@functools.lru_cache(maxsize=None)
def hollow():
    """the marching-tetrahedra surface of hollow_field on grid(40, 1): V = 4,130, F = 8,240, five closed oriented components"""
    from tests import marching_tets_ref as R
    pos, tets, edges, tet_edge, field = hollow_grid(40)
    m = R.marching_tets(pos[0], field, tets, 0.0, edges=edges, tet_edge=tet_edge)
    return _mesh(m.verts, m.faces)


CASES = dict({name: LK.CASES[name] for name in FROM_LOOP}, empty=empty, single=single, same_way=same_way, chunks=chunks, singles=singles,
             hollow=hollow)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, connectivity="edge"):
    """the Components of a case, computed once and shared"""
    from tests import mesh_components_ref as ref
    v, f = case(name)
    return ref.components(f, v.shape[0], v, connectivity)
