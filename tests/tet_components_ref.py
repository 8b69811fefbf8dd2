"""numpy restatement of the connected tet components and the occupancy clean-up (deftet_amd/csrc/tet_components.hip, DESIGN.md
§6o), for the tests, and the masks both test files use.

Tets t and u of one shape are connected when both are inside and u stands in row t of the neighbour table or t in row u (entries
outside [0, T) are never followed).  components: labels = the smallest tet index of the component (scipy's connected_components,
relabelled), -1 outside; sizes and the open flag at the label's index; the count.  cleanup: fill the enclosed outside components,
label, drop the components below min_size, keep the largest (the smaller label among equal sizes)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from deftet_amd import grids

CORNER = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]])      # local face i -> corners (i, i^1, i^2)


def nbr_table(tets):
    """int32 [T,4]: the tet across local face i of t, -1 where no other tet owns the face (sorted face keys, no Python loop)"""
    tets = np.asarray(tets, np.int64)
    T, V = tets.shape[0], int(tets.max()) + 1
    f = np.sort(tets[:, CORNER], axis=2).reshape(-1, 3)
    key = (f[:, 0] * V + f[:, 1]) * V + f[:, 2]
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    if (same[1:] & same[:-1]).any():
        raise ValueError("a face has more than two owners")
    a, b = order[:-1][same], order[1:][same]
    nbr = -np.ones(4 * T, np.int64)
    nbr[a], nbr[b] = b // 4, a // 4
    return nbr.reshape(T, 4).astype(np.int32)


def grid(res):
    """(tets int32 [T,4], n_vertex, neighbour table int32 [T,4], centroid - 0.5 float64 [T,3]) of the Kuhn grid"""
    verts, tets = grids.kuhn_grid(res)
    return tets, verts.shape[0], nbr_table(tets), verts[tets.astype(np.int64)].mean(axis=1) - 0.5


def components(inside, nbr):
    """one shape: dict(labels int32 [T], sizes int32 [T], open uint8 [T], count int)"""
    inside = np.asarray(inside).reshape(-1) != 0
    nbr = np.asarray(nbr, np.int64)
    T = inside.shape[0]
    valid = (nbr >= 0) & (nbr < T)
    rows = np.repeat(np.arange(T), 4).reshape(T, 4)
    link = valid & inside[:, None] & inside[np.where(valid, nbr, 0)]
    g = coo_matrix((np.ones(int(link.sum()), np.int8), (rows[link], nbr[link])), shape=(T, T))
    n, comp = connected_components(g, directed=False)
    first = np.full(n, T, np.int64)
    np.minimum.at(first, comp, np.arange(T))                          # (ascending arange: the first hit is the smallest)
    labels = np.where(inside, first[comp], -1).astype(np.int32)
    sizes = np.bincount(labels[inside], minlength=T).astype(np.int32)
    opn = np.zeros(T, np.uint8)
    opn[labels[inside & (nbr == -1).any(axis=1)]] = 1
    return dict(labels=labels, sizes=sizes, open=opn, count=int((labels == np.arange(T)).sum()))


def cleanup(inside, nbr, keep_largest=False, min_size=0, fill_voids=False):
    """one shape: keep bool [T], in the fixed order of the operator"""
    inside = np.asarray(inside).reshape(-1) != 0
    if fill_voids:
        out = components(~inside, nbr)
        enclosed = (out["labels"] >= 0) & (out["open"][np.maximum(out["labels"], 0)] == 0)
        inside = inside | enclosed
    c = components(inside, nbr)
    labels, sizes = c["labels"], c["sizes"]
    keep = labels >= 0
    if min_size > 0:
        keep &= sizes[np.maximum(labels, 0)] >= min_size
    if keep_largest:
        alive = np.nonzero((sizes > 0) & (sizes >= min_size))[0]      # labels of the components left, ascending
        if alive.size == 0:
            return np.zeros_like(keep)
        keep &= labels == alive[np.argmax(sizes[alive])]              # (argmax: the first, so the smaller label among equals)
    return keep


def bfs_components(inside, nbr):
    """plain-Python breadth-first search over the undirected table: (labels, sizes, open, count) as lists"""
    inside = [bool(x) for x in np.asarray(inside).reshape(-1)]
    T = len(inside)
    adj = [set() for _ in range(T)]
    for t in range(T):
        for u in (int(x) for x in nbr[t]):
            if 0 <= u < T and u != t:
                adj[t].add(u)
                adj[u].add(t)
    labels, sizes, opn, count = [-1] * T, [0] * T, [0] * T, 0
    for s in range(T):                                                # ascending: a new component starts at its smallest index
        if not inside[s] or labels[s] >= 0:
            continue
        count += 1
        labels[s] = s
        todo = [s]
        while todo:
            nxt = []
            for t in todo:
                sizes[s] += 1
                if any(int(x) == -1 for x in nbr[t]):
                    opn[s] = 1
                for u in adj[t]:
                    if inside[u] and labels[u] < 0:
                        labels[u] = s
                        nxt.append(u)
            todo = nxt
    return labels, sizes, opn, count


def eccentricity(inside, nbr, start):
    """breadth-first steps from `start` to the farthest inside tet it reaches"""
    inside = np.asarray(inside).reshape(-1) != 0
    T = inside.shape[0]
    seen = np.zeros(T, bool)
    seen[start] = True
    todo, steps = np.array([start]), 0
    und = [[] for _ in range(T)]
    for t in range(T):
        for u in nbr[t]:
            if 0 <= u < T:
                und[t].append(int(u))
                und[int(u)].append(t)
    while True:
        nxt = {u for t in todo for u in und[t] if inside[u] and not seen[u]}
        if not nxt:
            return steps
        todo = np.fromiter(nxt, np.int64)
        seen[todo] = True
        steps += 1


# ---------------------------------------------------------------------------- masks (cen = tet centroid - 0.5)
def shell(cen, r0=0.2, r1=0.4):
    r = np.linalg.norm(cen, axis=1)
    return (r > r0) & (r < r1)


def balls(cen, centres, radius):
    m = np.zeros(cen.shape[0], bool)
    for c in centres:
        m |= np.linalg.norm(cen - np.asarray(c, np.float64), axis=1) < radius
    return m


def two_balls(cen):
    return balls(cen, [(-0.25, 0, 0), (0.25, 0, 0)], 0.15)


def snake(res):
    """a corridor of whole cubes (six tets each, cube-major) that winds through the grid: one component with the longest chain"""
    n = res // 2
    ix, iy, iz = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    cube = (ix % 2 == 0) & ((iy % 2 == 0) | ((iy % 4 == 1) & (iz == n - 1)) | ((iy % 4 == 3) & (iz == 0)))
    cube |= ((ix % 4 == 1) & (iy == n - 2) & (iz == 0)) | ((ix % 4 == 3) & (iy == 0) & (iz == 0))
    return np.repeat(cube.reshape(-1), 6)


def every_sixth(T, k):
    return np.arange(T) % 6 == k


def random_mask(T, density, seed=0):
    return np.random.default_rng(seed).random(T) < density


def sphere_with_floaters(cen):
    return balls(cen, [(0, 0, 0)], 0.3) | balls(cen, [(0.4, 0.4, 0.4), (-0.4, 0.4, -0.4), (0.4, -0.4, -0.4)], 0.05)


def permuted(tets, mask, seed):
    """(tet list in a random order, its neighbour table, the mask in that order, perm) with new tet j = old tet perm[j]"""
    perm = np.random.default_rng(seed).permutation(tets.shape[0])
    return tets[perm], nbr_table(tets[perm]), np.asarray(mask)[..., perm], perm


def labels_through(labels, perm):
    """the labelling `labels` of the unpermuted shape carried to the permuted numbering: the same partition, every component
    named by its smallest NEW index"""
    old = np.asarray(labels)[perm]                                    # old label of new tet j
    T = old.shape[0]
    first = np.full(T, T, np.int64)
    ins = old >= 0
    np.minimum.at(first, old[ins], np.nonzero(ins)[0])
    return np.where(ins, first[np.maximum(old, 0)], -1).astype(np.int32)
