"""Seeded inputs shared by the marching-tetrahedra tests (CPU and GPU): jittered Kuhn grids as tests/cases.py makes them, and the
fields the tests put on them."""
import functools

import numpy as np

from deftet_amd import grids
from tests import marching_tets_ref as R

# the condition of the max-norm tests ONLY (check_close against float64): |f_max - f_min| on crossing edges, as a share of the
# field's range.  The per-entry tests (thin, spheres20, ...) carry no such condition: real inputs sit far below it.
GAP = 0.01
ISOS = (0.0, 0.1, -0.37)                                     # the levels of the per-entry tests; 0.1 and -0.37 are not fp32 numbers
WIDTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8)                         # attribute widths: none, <4> partial and full, <8> partial and full


@functools.lru_cache(maxsize=None)
def grid(res, batch):
    """(pos f32 [B,V,3] centred on the origin and jittered, tets int64 [T,4], edges int64 [E,2], tet_edge int64 [T,6])"""
    verts, tets = grids.kuhn_grid(res)
    pos = grids.jittered_positions(verts, res, batch, 0.1)
    tets = tets.astype(np.int64)
    edges, tet_edge = R.tet_edges(tets)
    for a in (pos, tets, edges, tet_edge):
        a.setflags(write=False)
    return pos, tets, edges, tet_edge


def sphere(pos_vx3, radius):
    return (np.float32(radius) - np.sqrt((pos_vx3.astype(np.float32) ** 2).sum(-1, dtype=np.float32))).astype(np.float32)


def banded(n, seed, gap=0.1):
    """random values from [-1,-gap] and [gap,1]: every sign change spans at least 2 gap = 10 % of the range"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(gap, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def crossing_gap(field, edges, iso=0.0):
    """the smallest |f_max - f_min| over the crossing edges, as a share of the field's range (inf without a crossing)"""
    inside = field > np.float32(iso)
    c = inside[edges[:, 0]] != inside[edges[:, 1]]
    if not c.any():
        return np.inf
    return float(np.abs(field[edges[c, 1]] - field[edges[c, 0]]).min() / (field.max() - field.min()))


def attrs(batch, n_vertex, channels, seed):
    return np.random.default_rng(seed).uniform(0, 1, (batch, n_vertex, channels)).astype(np.float32)


RADII20 = (0.18, 0.2, 0.27, 0.39, 0.35)                     # the five spheres of the res 20 case: each keeps crossing_gap > GAP


# ------------------------------------------------------------------------------- inputs of the per-entry tests (no GAP condition)
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def crossing_gaps(field, edges, iso=0.0):
    """|f_max - f_min| of every crossing edge, in float32 as the operator subtracts them"""
    inside = field > np.float32(iso)
    c = inside[edges[:, 0]] != inside[edges[:, 1]]
    return np.abs(field[edges[c, 1]] - field[edges[c, 0]])


@functools.lru_cache(maxsize=None)
def thin(n, iso, seed):
    """float32(iso) + s 10^u with s = +-1 and u uniform in [-6, 0], rounded to float32: crossing gaps over six decades"""
    rng = np.random.default_rng(seed)
    s, u = rng.choice([-1.0, 1.0], n), rng.uniform(-6.0, 0.0, n)
    return _frozen((float(np.float32(iso)) + s * 10.0 ** u).astype(np.float32))


def thin_batch(n, iso, seed, batch):
    return _frozen(np.stack([thin(n, iso, seed + b) for b in range(batch)]))


def assert_thin(field, edges, iso):
    """the condition of the thin cases, on the input: a crossing gap under 1e-5 of the field's range, one above 1e-1, and none
    zero or subnormal (the gap is a float32 the backward divides by, squared in double)"""
    gaps = crossing_gaps(field, edges, iso)
    share = gaps.astype(np.float64) / (float(field.max()) - float(field.min()))
    assert gaps.size and share.min() < 1e-5 and share.max() > 1e-1, (gaps.size, share.min(), share.max())
    assert (gaps >= np.finfo(np.float32).tiny).all()


@functools.lru_cache(maxsize=None)
def level(n, iso, seed):
    """float32(iso) itself and its two float32 neighbours at random: on the level and below it are outside, above it is inside"""
    at = np.float32(iso)
    three = np.array([np.nextafter(at, np.float32(-np.inf)), at, np.nextafter(at, np.float32(np.inf))], np.float32)
    return _frozen(np.random.default_rng(seed).choice(three, n))


@functools.lru_cache(maxsize=None)
def spheres20():
    """(pos [2,V,3], field [2,V]): spheres of radius 0.3 and 0.25 on shape 0 of grid(20, 1), radii not picked for their gap
    (crossing_gap 0.48 % and 0.27 %, under GAP)"""
    pos = np.repeat(grid(20, 1)[0], 2, axis=0)
    return _frozen(pos, np.stack([sphere(pos[0], 0.3), sphere(pos[1], 0.25)]))


@functools.lru_cache(maxsize=None)
def shuffled8():
    """(pos [1,V,3], tets, edges, tet_edge): grid(8, 1) with its tets shuffled and the corners of every tet permuted — negative
    tets, edge ends in either field order (the list test_arbitrary_numbering_and_a_subdivided_list builds)"""
    pos, tets, _e, _te = grid(8, 1)
    rng = np.random.default_rng(9)
    tets = tets[rng.permutation(tets.shape[0])]
    tets = np.take_along_axis(tets, np.argsort(rng.random(tets.shape), axis=1), axis=1)
    return (pos,) + _frozen(tets, *R.tet_edges(tets))


@functools.lru_cache(maxsize=None)
def subdivided8():
    """(pos [1,V2,3], tets [8T,4], edges, tet_edge, field [1,V2]): shuffled8 subdivided once (midpoints appended in edge order, eight
    children per tet: oracle.generate_subdivision, which hip_ops.subdivide equals) and the sphere of radius 0.3 on it"""
    from oracle import oracle as O
    pos, tets, _e, _te = shuffled8()
    p2, _f2, t2 = O.generate_subdivision(tets, pos[0], np.zeros((pos.shape[1], 1), np.float32))
    p2, t2 = p2.astype(np.float32)[None], t2.astype(np.int64)
    return _frozen(p2, t2, *R.tet_edges(t2), sphere(p2[0], 0.3)[None])


def field8(pos):
    """the four shapes of the res 8 batch: empty, a sphere, empty, a banded random field"""
    V = pos.shape[1]
    return np.stack([np.full(V, -1, np.float32), sphere(pos[1], 0.3), np.full(V, 2, np.float32), banded(V, 3)])


def field20(pos):
    return np.stack([sphere(pos[b], r) for b, r in enumerate(RADII20)])


# name -> attribute widths its backward runs with (0: no attributes)
PER_ENTRY = {"thin8@0.0": WIDTHS, "thin8@0.1": WIDTHS, "thin8@-0.37": WIDTHS, "thin20@0.1": (5,), "spheres20": (4,), "spheres20+0.25": (6,),
             "subdivided8": (2,), "subdivided8+0.25": (7,), "shuffled8-thin": (3,), "kuhn8": (3, 8), "kuhn20": (2,)}
THIN = tuple(n for n in PER_ENTRY if "thin" in n)
FORWARD = ("thin8@0.0", "thin8@0.1", "thin8@-0.37", "spheres20", "subdivided8", "level8@0.1")


@functools.lru_cache(maxsize=None)
def per_entry_case(name):
    """(pos [B,V,3], field [B,V], tets, edges, tet_edge, iso) of a named input of the per-entry tests.  `+0.25` is the same field
    shifted with iso = 0.25: the same inside set, hence the same mesh topology (asserted by the tests as a condition on the input)"""
    if name.endswith("+0.25"):
        pos, field, tets, edges, tet_edge, iso = per_entry_case(name[:-5])
        return pos, _frozen((field + np.float32(0.25)).astype(np.float32)), tets, edges, tet_edge, iso + 0.25
    iso = float(name.split("@")[1]) if "@" in name else 0.0
    if name.startswith("thin8@"):
        pos, tets, edges, tet_edge = grid(8, 3)
        field = thin_batch(pos.shape[1], iso, 100 + 10 * ISOS.index(iso), 3)
    elif name == "thin20@0.1":
        pos, tets, edges, tet_edge = grid(20, 2)
        field = thin_batch(pos.shape[1], iso, 140, 2)
    elif name == "level8@0.1":
        pos, tets, edges, tet_edge = grid(8, 3)
        field = _frozen(np.stack([level(pos.shape[1], iso, 150 + b) for b in range(3)]))
    elif name == "spheres20":
        (pos, field), (_p, tets, edges, tet_edge) = spheres20(), grid(20, 1)
    elif name == "subdivided8":
        pos, tets, edges, tet_edge, field = subdivided8()
    elif name == "shuffled8-thin":
        pos, tets, edges, tet_edge = shuffled8()
        iso = ISOS[2]
        field = thin_batch(pos.shape[1], iso, 160, 1)
    elif name == "kuhn8":
        pos, tets, edges, tet_edge = grid(8, 4)
        field = _frozen(field8(pos))
    elif name == "kuhn20":
        pos, tets, edges, tet_edge = grid(20, 5)
        field = _frozen(field20(pos))
    elif name == "hostile20":                                                          # shape 0 hostile, shape 1 clean
        pos, tets, edges, tet_edge = grid(20, 2)
        field = _frozen(np.stack([hostile(banded(pos.shape[1], 170), 171)[0], banded(pos.shape[1], 172)]))
    else:
        raise KeyError(name)
    if "thin" in name:
        for f in field:
            assert_thin(f, edges, iso)
    return pos, field, tets, edges, tet_edge, iso


def per_entry_gradients(name, C, seed=0):
    """(attr [B,V,C] | None, [g_verts per shape], [g_attr per shape] | None): N(0,1) float32 output gradients, one row per crossing edge"""
    pos, field, _tets, edges, _te, iso = per_entry_case(name)
    B, V = field.shape
    rng = np.random.default_rng([seed, C, sorted(list(PER_ENTRY) + ["hostile20"]).index(name)])
    n = [int((lambda ins: ins[edges[:, 0]] != ins[edges[:, 1]])(field[b] > np.float32(iso)).sum()) for b in range(B)]
    gv = [rng.normal(size=(k, 3)).astype(np.float32) for k in n]
    if C == 0:
        return None, gv, None
    return attrs(B, V, C, 1000 + C), gv, [rng.normal(size=(k, C)).astype(np.float32) for k in n]


HOSTILE = (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)


def hostile(field, seed, iso=0.0):
    """(field with six interior vertices of grid(20) — pairwise not joined by an edge — set to NaN, +inf, -inf, NaN, +inf, -inf;
    affected edges bool [E]: crossing, with a non-finite end; affected vertices bool [V]: an end of such an edge)"""
    _pos, _tets, edges, _te = grid(20, 1)
    V = field.shape[0]
    valence = np.bincount(edges.reshape(-1), minlength=V)
    rng = np.random.default_rng(seed)
    chosen = []
    for v in rng.permutation(np.nonzero(valence == 14)[0]):                            # 14 edges: an interior vertex of a Kuhn grid
        nbrs = np.concatenate([edges[edges[:, 0] == v, 1], edges[edges[:, 1] == v, 0]])
        if not np.isin(chosen, nbrs).any():
            chosen.append(int(v))
        if len(chosen) == len(HOSTILE):
            break
    out = np.array(field, np.float32)
    out[chosen] = HOSTILE
    inside = out > np.float32(iso)
    cross = inside[edges[:, 0]] != inside[edges[:, 1]]
    bad_edge = cross & ~np.isfinite(out[edges]).all(1)
    bad_vertex = np.zeros(V, bool)
    bad_vertex[edges[bad_edge].reshape(-1)] = True
    return _frozen(out, bad_edge, bad_vertex)
