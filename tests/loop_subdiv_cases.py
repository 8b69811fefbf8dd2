"""The meshes of the Loop subdivision tests (tests/test_loop_subdiv_cpu.py, tests/test_loop_subdiv_gpu.py): all tiny, each
for one branch of the rules.  A case is (verts float32 [V,3], faces int64 [F,3]); V may exceed the vertices in use."""
import functools

import numpy as np


def _mesh(verts, faces):
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def tetrahedron():
    """every vertex at valence 3: the beta = 3/16 branch"""
    v = [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
    return _mesh(v, [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def octahedron():
    """valence 4"""
    v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return _mesh(v, f)


def icosahedron():
    """valence 5"""
    p = (1 + 5 ** 0.5) / 2
    v = [[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1],
         [-p, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4],
         [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return _mesh(v, f)


def flat_patch(n=5):
    """n x n vertices of a regular triangular lattice in the plane (the square grid sheared and split along one diagonal: every
    interior vertex has valence 6 and sits at the centroid of its ring; row height 7/8 in place of sqrt(3)/2, an affine image
    whose coordinates are exact in float32), open: its boundary is a crease, two of its corners have valence 2"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i + 0.5 * j, j * 0.875, np.zeros_like(i, float)], -1).reshape(-1, 3)
    idx = lambda a, b: a * n + b
    f = []
    for a in range(n - 1):
        for b in range(n - 1):
            f.append([idx(a, b), idx(a + 1, b), idx(a, b + 1)])
            f.append([idx(a + 1, b), idx(a + 1, b + 1), idx(a, b + 1)])
    return _mesh(v, f)


def patch_interior(n=5):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return ((i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)).reshape(-1)


def fan(n, closed):
    """a hub (vertex 0, lifted off the plane) and n rim vertices; closed: n triangles, the hub smooth of valence n; open: n - 1
    triangles, the hub on the boundary"""
    t = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0, 0, 0.5]], np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3 * t)], 1)])
    f = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n if closed else n - 1)]
    return _mesh(v, f)


def open_fan200():
    """an open fan of valence 200: the hub has more neighbours than a wave has lanes and lies on the boundary (a crease vertex)"""
    return fan(200, False)


def smooth_fan200():
    """the same hub made SMOOTH: a second hub (201) below the rim 1..200, one triangle of the lower fan left out so the mesh
    stays open — a smooth vertex of valence 200 whose sum runs over 200 neighbours"""
    n = 200
    v, f = fan(n, True)
    v = np.concatenate([v, [[0, 0, -0.5]]])
    lower = [[n + 1, 1 + (k + 1) % n, 1 + k] for k in range(n - 1)]
    return _mesh(v, np.concatenate([f, lower]))


def closed_fan70():
    return fan(70, True)


def book():
    """three triangles on the edge (0,1): a non-manifold crease; 0 and 1 have 4 crease edges (corners), 2, 3, 4 have two"""
    v = [[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 0.9, 0.5], [-0.5, -0.9, 0.5]]
    return _mesh(v, [[0, 1, 2], [0, 1, 3], [0, 1, 4]])


def bowtie():
    """two triangles sharing vertex 0 only: its 4 boundary edges make it a corner"""
    v = [[0, 0, 0], [1, 0.5, 0], [1, -0.5, 0.2], [-1, 0.5, 0.1], [-1, -0.5, 0]]
    return _mesh(v, [[0, 1, 2], [0, 3, 4]])


def big_index():
    """eight faces (an octahedron) on the top indices of V = 100,000 otherwise isolated vertices: the key min V + max passes 32
    bits, and the smooth n = 0 branch runs"""
    V = 100_000
    ov, of = octahedron()
    rng = np.random.default_rng(5)
    v = rng.normal(size=(V, 3))
    top = np.array([V - 10, V - 9, V - 7, V - 5, V - 2, V - 1])
    v[top] = ov
    return _mesh(v, top[of])


def two_copies():
    """two disjoint icosahedra, the second with reversed faces"""
    v, f = icosahedron()
    return _mesh(np.concatenate([v, v * 0.5 + 3.0]), np.concatenate([f, f[:, ::-1] + v.shape[0]]))


@functools.lru_cache(maxsize=None)
def sphere20():
    """the marching-tetrahedra mesh of shape 0 of marching_tets_cases.spheres20() (radius 0.3 at res 20): irregular valences"""
    from tests import marching_tets_cases as K
    from tests import marching_tets_ref as R
    pos, field = K.spheres20()
    _p, tets, edges, tet_edge = K.grid(20, 1)
    m = R.marching_tets(pos[0], field[0], tets, 0.0, edges=edges, tet_edge=tet_edge)
    return _mesh(m.verts, m.faces)


CASES = {"tetrahedron": tetrahedron, "octahedron": octahedron, "icosahedron": icosahedron, "flat_patch": flat_patch, "open_fan200": open_fan200, "smooth_fan200": smooth_fan200,
         "closed_fan70": closed_fan70, "book": book, "bowtie": bowtie, "big_index": big_index, "two_copies": two_copies, "sphere20": sphere20}
CLOSED = ("tetrahedron", "octahedron", "icosahedron", "two_copies", "sphere20")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(topology, S, L) of a case, computed once and shared"""
    from tests import loop_subdiv_ref as ref
    v, f = case(name)
    top = ref.topology(f, v.shape[0])
    return top, ref.subdivision_matrix(top), ref.limit_matrix(top)
