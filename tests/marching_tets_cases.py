"""Seeded inputs shared by the marching-tetrahedra tests (CPU and GPU): jittered Kuhn grids as tests/cases.py makes them, and the
fields the tests put on them."""
import functools

import numpy as np

from deftet_amd import grids
from tests import marching_tets_ref as R

GAP = 0.01                                                   # |f_max - f_min| on crossing edges, as a share of the field's range


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
