"""Inputs of the fp64 pin of the point-in-tet weights and backward (tests/test_bary_ref_cpu.py, tests/test_bary_backward_gpu.py):
tets of known conditioning with queries whose tet is known by construction.

lattice      one tet per cell of an n x n x n lattice (cell edge `size`, first corner `origin`), so the tets are DISJOINT: four
             uniform points of the unit box, kept if the draw is well shaped (kappa0 <= 60, kappa of the draw about its own
             centroid) and still inside the box after the squash; squashed about the centroid along a random unit direction by
             `flat`; the box scaled by 0.9 * size and centred in the cell, so that no tet reaches the outer 5 % of its cell.
kappa        L^3 / |6V| * max(1, max|coordinate| / L), L the longest edge, in fp64 from the fp32 tet: the factor by which a
             relative error 2^-24 of the coordinates grows on the way to a weight.  A tet is ASSERTED iff kappa <= KAPPA_CAP.
queries      own[q] is chosen, p = sum w_i v_i in fp64 with Dirichlet(2,2,2,2) weights (the centroid where min w < 0.05), rounded
             to fp32; per-tet hit counts come from a list the case names.  Every cell holds a tet, so the misses (about 10 %, own
             = -1) go where no tet can be: the outer 4 % of a cell, next to one of its walls.  The order is shuffled.
"""
import numpy as np

U = 2.0 ** -24
K = 8                       # DESIGN.md section 4, "What is pinned": from the fp32 restatement (test_bary_ref_cpu.py), not from a GPU
KAPPA_CAP = 5e4
KAPPA0_MAX = 60.0
MIN_ASSERTED_SHARE = 0.90
MIN_WEIGHT = 0.05

BAND_GEOMETRY = {"unit": (0.0, 1.0), "small": (-0.5, 1.0 / 16), "far": (100.0, 1.0)}                 # origin, size
BANDS = [("unit", 1.0), ("unit", 0.1), ("unit", 0.01), ("small", 1.0), ("small", 0.1), ("small", 0.01), ("far", 1.0), ("far", 0.1)]
BAND_IDS = ["%s-%g" % b for b in BANDS]

# per-tet hit counts (a tet draws one of them)
COUNTS_SPARSE = [0, 0, 0, 0, 1, 1, 1, 2, 3, 6]           # records (<= 2 hits) and spill records (3 to 6); 1.4 per tet
COUNTS_DENSE = [1, 2, 6, 13, 40]                         # 12.4 per tet: the per-tet lists


def kappa(tet):
    """[T] fp64 from tet [T,4,3] (any float type; the fp32 values are what the kernels see)"""
    t = np.asarray(tet, np.float64)
    e = t[:, [1, 2, 3, 2, 3, 3]] - t[:, [0, 0, 0, 1, 1, 2]]
    L = np.sqrt((e ** 2).sum(-1)).max(1)
    v6 = np.abs(np.einsum("ti,ti->t", e[:, 0], np.cross(e[:, 1], e[:, 2])))
    with np.errstate(divide="ignore", invalid="ignore"):
        return L ** 3 / v6 * np.maximum(1.0, np.abs(t).max((1, 2)) / L)


def cell_corners(band, n):
    """[n^3,3] fp64: the low corner of every cell, x fastest"""
    origin, size = BAND_GEOMETRY[band]
    k = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)[:, ::-1]
    return origin + size * k.astype(np.float64)


def lattice(band, flat, n=8, seed=0):
    """tet f32 [n^3,4,3]"""
    origin, size = BAND_GEOMETRY[band]
    T = n ** 3
    rng = np.random.default_rng([seed, n, sorted(BAND_GEOMETRY).index(band), int(round(1000 * flat))])
    kept = []
    while sum(x.shape[0] for x in kept) < T:
        v = rng.random((4 * T, 4, 3))
        c = v.mean(1, keepdims=True)
        d = rng.standard_normal((4 * T, 1, 3))
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        ok = kappa(v - c) <= KAPPA0_MAX
        r = v - c
        v = c + r - (1.0 - flat) * (r * d).sum(2, keepdims=True) * d
        ok &= (v.min((1, 2)) >= 0.0) & (v.max((1, 2)) <= 1.0)
        kept.append(v[ok])
    v = np.concatenate(kept, 0)[:T]
    centre = cell_corners(band, n) + 0.5 * size
    tet = (centre[:, None, :] + (v - 0.5) * (0.9 * size)).astype(np.float32)
    lo = cell_corners(band, n)[:, None, :]
    assert ((tet > lo + 0.04 * size) & (tet < lo + 0.96 * size)).all()          # after the rounding to fp32 too
    return tet


def queries(band, tet, counts, n, seed=0, miss_share=0.1):
    """-> pts f32 [Q,3], own i64 [Q] (-1: placed where no tet is), for counts i64 [T] hits per tet"""
    origin, size = BAND_GEOMETRY[band]
    T = tet.shape[0]
    rng = np.random.default_rng([seed, T, int(np.sum(counts)), 77])
    own = np.repeat(np.arange(T), counts)
    w = rng.dirichlet([2, 2, 2, 2], own.shape[0])
    w[w.min(1) < MIN_WEIGHT] = 0.25
    p = (w[:, :, None] * tet[own].astype(np.float64)).sum(1)
    n_miss = int(round(miss_share * own.shape[0]))
    cell = cell_corners(band, n)[rng.integers(0, T, n_miss)]
    f = 0.02 + 0.96 * rng.random((n_miss, 3))
    axis = rng.integers(0, 3, n_miss)
    f[np.arange(n_miss), axis] = np.where(rng.random(n_miss) < 0.5, 0.0, 0.96) + 0.005 + 0.03 * rng.random(n_miss)
    pts = np.concatenate([p, cell + f * size], 0)
    own = np.concatenate([own, np.full(n_miss, -1)])
    order = rng.permutation(own.shape[0])
    return pts[order].astype(np.float32), own[order].astype(np.int64)


def draw_counts(T, choices, seed=0, extra=(), allowed=None):
    """i64 [T]: every tet draws one of `choices`; extra = ((count, how many tets), ...) then gives `count` hits to that many tets
    among `allowed` (bool [T]: the asserted ones, so that the long sums are checked and not merely run)"""
    rng = np.random.default_rng([seed, T, len(choices), 5])
    counts = rng.choice(np.asarray(choices, np.int64), T)
    if extra:
        where = rng.permutation(np.nonzero(allowed)[0] if allowed is not None else np.arange(T))
        k = 0
        for count, how_many in extra:
            counts[where[k: k + how_many]] = count
            k += how_many
    return counts


def shape(band, flat, counts=COUNTS_SPARSE, n=8, seed=0, extra=(), miss_share=0.1, perm_seed=None):
    """One shape of the pin: dict(tet f32 [T,4,3], pts f32 [Q,3], own i64 [Q], kappa [T], asserted bool [T], counts i64 [T]).
    perm_seed: the multiset of counts of seed 0, handed to other tets (the shapes of one batch must agree on Q)."""
    tet = lattice(band, flat, n, seed)
    k = kappa(tet)
    c = draw_counts(tet.shape[0], counts, 0 if perm_seed is not None else seed, extra, k <= KAPPA_CAP)
    if perm_seed is not None:
        c = c[np.random.default_rng([perm_seed, 3]).permutation(c.shape[0])]
    pts, own = queries(band, tet, c, n, seed, miss_share)
    return {"band": band, "flat": flat, "n": n, "tet": tet, "pts": pts, "own": own, "kappa": k, "asserted": k <= KAPPA_CAP, "counts": c}


# the shapes the GPU tests run and the CPU test holds the restatement to, by name
OVERFLOW_EXTRA = ((9, 8), (40, 2))                       # more than a record and its spill record hold: the ordered list scan
BUTTERFLY_N, BUTTERFLY_HITS = 12, 2048                   # 2,048 hits x 2,048 / 64 list steps > 16,384: the butterfly
MIXED_BANDS = [("unit", 0.01), ("small", 1.0), ("far", 0.1)]


def records_shape(band, seed=0, perm_seed=None):
    return shape(band[0], band[1], COUNTS_SPARSE, seed=seed, perm_seed=perm_seed)


def overflow_shape(band):
    return shape(band[0], band[1], COUNTS_SPARSE, extra=OVERFLOW_EXTRA)


def lists_shape(band):
    return shape(band[0], band[1], COUNTS_DENSE)


def butterfly_shape():
    return shape("unit", 0.1, [0, 0, 0, 1], n=BUTTERFLY_N, extra=((BUTTERFLY_HITS, 1),))


def mixed_batch():
    return [records_shape(b, seed=i, perm_seed=i) for i, b in enumerate(MIXED_BANDS)]


def pair_batch(band):
    """two shapes of one band with the same number of queries"""
    return [records_shape(band, seed=i, perm_seed=i) for i in range(2)]


def asserted_share(s):
    """the share of the tets that receive a hit which are asserted"""
    hit = s["counts"] > 0
    return float(s["asserted"][hit].mean())


def incoming(s, seed=0):
    """seeded incoming gradients: grad_w f32 [Q,4], grad_occ f32 [Q]"""
    rng = np.random.default_rng([seed, s["pts"].shape[0], 11])
    return rng.standard_normal((s["pts"].shape[0], 4)).astype(np.float32), rng.standard_normal(s["pts"].shape[0]).astype(np.float32)


def soup_topology(T, seed=0):
    """The 4T vertices of T disjoint tets as a mesh: idx i64 [T,4] a seeded permutation of arange(4T) (no vertex is shared, but
    vertex v is not corner v % 4 of tet v // 4 either: the incidence CSR is not the identity), and pos = scatter of the corners.
    -> idx; pos_from(tet) builds the positions"""
    return np.random.default_rng([seed, T, 13]).permutation(4 * T).reshape(T, 4).astype(np.int64)


def soup_positions(tet, idx):
    """pos [4T,3] with pos[idx[t,k]] = tet[t,k]"""
    pos = np.empty((idx.size, 3), tet.dtype)
    pos[idx.reshape(-1)] = tet.reshape(-1, 3)
    return pos
