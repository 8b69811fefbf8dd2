"""Inputs of the fp64 pin of the rasterizer backward (tests/test_raster_bwd_ref_cpu.py, tests/test_raster_bwd_fp64_gpu.py): faces of
known conditioning with hits placed by construction.  The backward entry takes the face list as an INPUT, so which pixel hits
which face, and how many hits a face collects, is decided here and nothing depends on the forward's coverage decisions.

lattice      one triangle per cell of an n x n lattice of the image plane (cell edge `size`, first corner `origin`), so the faces
             are DISJOINT: three uniform points of the unit square, kept if the draw is well shaped (kappa0 = W^2 / |k3| about
             the centroid <= KAPPA0_MAX); squashed about the centroid along a random unit direction by `flat`; scaled by 0.9 *
             size and centred in the cell; rounded to fp32 (the face stays inside the inner 92 % of its cell).
bands        image: the coordinates of BASELINE configs[4] (grids.project_faces multiplies by 1000, a res-70 face is about 25
             wide); unit: the same picture on [-1, 1]; far: the image band 30,000 units from the origin.
kappa        W^2 / |k3 + eps| * max(1, C / W) in fp64 from the fp32 values, W the larger box extent of the face and C the largest
             |coordinate| among the face and the pixels that hit it: the factor by which a relative error 2^-24 of the coordinates
             grows on the way to a weight (raster.hip, the comment above face_box: |e_1|, |e_2| <= 3.01 u W (|s| + |t|),
             |e_3| <= 6.02 u W^2, and s, t themselves carry u C).  A face is ASSERTED iff kappa <= KAPPA_CAP.
hits         counts[f] pixels have face f in slot 0: p = sum w_i v_i in fp64 with Dirichlet(2,2,2) weights (the centroid where
             min w < 0.05), rounded to fp32.  With knum > 1 a pixel uses r slots, r drawn from 1..knum, and slots 1..r-1 hold
             faces of neighbouring cells: the pixel lies outside them and their weights extrapolate (a legal input of the
             backward; it exercises p = h / knum).  Slots r.. hold -1.  The pixel order is shuffled.
counts       a face draws one count of the case's list; the lists sit on the three layers of edges of the reduction: 4 hits per
             lane, 256 per wave and 1,024 per block in k_bwd_runs, 64 per wave and 1,024 per block in k_bwd_sorted.  The faces are
             in lattice order, the counts are dealt to them at random, so in the sorted order the runs start at every lane and row
             offset.

Recorded on the CPU (tests/test_raster_bwd_ref_cpu.py asserts them): CLASS_COUNTS, the classes by raster_scene.classify_faces at
the band's eps as (REGULAR, SLIVER, DEGENERATE) per lattice, and ASSERTED_SHARE, the share of the faces with a hit that are
asserted, per case.  The unit band runs with eps = 1e-12: at the default 1e-8 every face of it flatter than 1 would be DEGENERATE
by the |k3| >= 1024 eps rule, and the second value of eps is an argument of the entry that no other test varies.
"""
import functools

import numpy as np

from tests import raster_scene as RS

U = 2.0 ** -24
# K: from the fp32 restatement on the CPU, not from a GPU (tests/raster_bwd_ref.py: k_needed_xy / k_needed_feat;
# test_raster_bwd_ref_cpu.py::test_restatement_stays_within_half_of_k).  The restatement's worst k over the asserted faces of every band
# x flat x count list x knum at D = 4, and of the image and unit bands with their shifted copies at D = 3, 6, 9, is
# K_RESTATEMENT_WORST (gfeat in the unit band at flat 1; gxy needs 0.051 at the most); doubled and rounded up to an integer.
K = 1
K_RESTATEMENT_WORST = 0.147
# KAPPA_CAP: the shares below need 1.14e6 (five of the nine faces of image-2^-13-block); the next round figure.  At 2^-24 kappa =
# 0.09 a weight keeps one digit.
KAPPA_CAP = 1.5e6
KAPPA0_MAX = 8.0
MIN_ASSERTED_SHARE = 0.90                # per case, flat 1, 2^-5, 2^-9 of the image and unit bands
MIN_ASSERTED_SHARE_IMAGE_FLATTEST = 0.5  # per case, flat 2^-13 of the image band
MIN_WEIGHT = 0.05

BAND_GEOMETRY = {"image": (-1000.0, 25.0, 1e-8), "unit": (-1.0, 1.0 / 32, 1e-12), "far": (30000.0, 25.0, 1e-8)}     # origin, cell size, eps
BANDS = ["image", "unit", "far"]
FLATS = [1.0, 2.0 ** -5, 2.0 ** -9, 2.0 ** -13]
FLAT_IDS = {1.0: "1", 2.0 ** -5: "2^-5", 2.0 ** -9: "2^-9", 2.0 ** -13: "2^-13"}

# per-face hit counts (a face draws one of them) and the lattice edge of the list
COUNTS_LANE = [0, 0, 1, 1, 2, 3, 4, 5, 7, 8, 9]
COUNTS_WAVE = [63, 64, 65, 255, 256, 257]
COUNTS_BLOCK = [1023, 1024, 1025, 2049, 2100]
LISTS = {"lane": (COUNTS_LANE, 24), "wave": (COUNTS_WAVE, 8), "block": (COUNTS_BLOCK, 3)}     # block: 9 faces, P = 12,342: P * knum = 61,710 at knum = 5
KNUMS = [1, 5]


def case_id(band, flat, kind, knum):
    return "%s-%s-%s-k%d" % (band, FLAT_IDS[flat], kind, knum)


CASES = [(b, f, kind, k) for b in BANDS for f in FLATS for kind in LISTS for k in KNUMS]
CASE_IDS = [case_id(*c) for c in CASES]

# ---- recorded on the CPU; tests/test_raster_bwd_ref_cpu.py holds the cases to them ---------------------------------------------
# (REGULAR, SLIVER, DEGENERATE) by raster_scene.classify_faces at the band's eps, per lattice
CLASS_COUNTS = {
    ("image", 1.0): {"lane": (576, 0, 0), "wave": (64, 0, 0), "block": (9, 0, 0)},
    ("image", 2.0 ** -5): {"lane": (528, 48, 0), "wave": (60, 4, 0), "block": (8, 1, 0)},
    ("image", 2.0 ** -9): {"lane": (29, 547, 0), "wave": (2, 62, 0), "block": (0, 9, 0)},
    ("image", 2.0 ** -13): {"lane": (0, 573, 3), "wave": (0, 64, 0), "block": (0, 9, 0)},
    ("unit", 1.0): {"lane": (576, 0, 0), "wave": (64, 0, 0), "block": (9, 0, 0)},
    ("unit", 2.0 ** -5): {"lane": (537, 39, 0), "wave": (59, 5, 0), "block": (6, 3, 0)},
    ("unit", 2.0 ** -9): {"lane": (25, 551, 0), "wave": (2, 62, 0), "block": (0, 9, 0)},
    ("unit", 2.0 ** -13): {"lane": (0, 571, 5), "wave": (0, 63, 1), "block": (0, 9, 0)},
    ("far", 1.0): {"lane": (576, 0, 0), "wave": (64, 0, 0), "block": (9, 0, 0)},
    ("far", 2.0 ** -5): {"lane": (530, 46, 0), "wave": (62, 2, 0), "block": (8, 1, 0)},
    ("far", 2.0 ** -9): {"lane": (27, 549, 0), "wave": (2, 62, 0), "block": (0, 9, 0)},
    ("far", 2.0 ** -13): {"lane": (0, 532, 44), "wave": (0, 61, 3), "block": (0, 9, 0)},
}
# the share of the faces with a hit that are asserted (kappa <= KAPPA_CAP), per case: lane, wave, block x knum 1, 5.  Required: the
# image and unit bands down to 2^-9 (>= 0.90) and image 2^-13 (>= 0.5); the far band at 2^-13 is unasserted altogether: that is what
# the cap is for (kappa there is 2.7e7 at the median, fp32 keeps no digit of a weight).
ASSERTED_SHARE = {
    ("image", 1.0): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("image", 2.0 ** -5): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("image", 2.0 ** -9): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("image", 2.0 ** -13): (0.813, 0.792, 0.750, 0.750, 0.778, 0.778),
    ("unit", 1.0): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("unit", 2.0 ** -5): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("unit", 2.0 ** -9): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("unit", 2.0 ** -13): (0.898, 0.884, 0.859, 0.859, 0.778, 0.667),
    ("far", 1.0): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("far", 2.0 ** -5): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000),
    ("far", 2.0 ** -9): (0.364, 0.356, 0.453, 0.453, 0.444, 0.444),
    ("far", 2.0 ** -13): (0.000, 0.000, 0.000, 0.000, 0.000, 0.000),
}
SHARE_ORDER = [(kind, knum) for kind in LISTS for knum in KNUMS]


def _k3(v):
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1])


def _extent(v):
    return (v.max(1) - v.min(1)).max(1)


def kappa0(v):
    """[F] fp64: W^2 / |k3| of triangles v [F,3,2] (about the centroid the coordinates are no larger than W: the second factor is 1)"""
    v = np.asarray(v, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _extent(v) ** 2 / np.abs(_k3(v))


def pixel_reach(pix, face, F):
    """[F] fp64: the largest |coordinate| among the pixels that hit a face (0 for a face without a hit); pix [P,2], face [P,knum]"""
    reach = np.zeros(F)
    p, s = np.nonzero(face >= 0)
    np.maximum.at(reach, face[p, s], np.abs(np.asarray(pix, np.float64)[p]).max(1))
    return reach


def kappa(fxy, pix_of_face, eps):
    """[F] fp64 from fxy [F,3,2] (the fp32 values are what the kernels see) and pix_of_face [F] (pixel_reach)"""
    v = np.asarray(fxy, np.float64)
    W = _extent(v)
    C = np.maximum(np.abs(v).max((1, 2)), pix_of_face)
    with np.errstate(divide="ignore", invalid="ignore"):
        return W ** 2 / np.abs(_k3(v) + np.float64(np.float32(eps))) * np.maximum(1.0, C / W)


def cell_corners(band, n):
    """[n*n,2] fp64: the low corner of every cell, x fastest"""
    origin, size, _ = BAND_GEOMETRY[band]
    j, i = np.divmod(np.arange(n * n), n)
    return origin + size * np.stack([i, j], -1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def lattice(band, flat, n, seed=0):
    """fxy f32 [n*n,3,2]"""
    origin, size, _ = BAND_GEOMETRY[band]
    F = n * n
    rng = np.random.default_rng([seed, n, BANDS.index(band), int(round(-np.log2(flat)))])
    kept = []
    while sum(x.shape[0] for x in kept) < F:
        v = rng.random((4 * F, 3, 2))
        c = v.mean(1, keepdims=True)
        a = rng.random((4 * F, 1, 1)) * 2 * np.pi
        d = np.concatenate([np.cos(a), np.sin(a)], 2)
        ok = kappa0(v - c) <= KAPPA0_MAX
        r = v - c
        v = c + r - (1.0 - flat) * (r * d).sum(2, keepdims=True) * d
        ok &= (v.min((1, 2)) >= 0.0) & (v.max((1, 2)) <= 1.0)          # still inside the unit square after the squash
        kept.append(v[ok])
    v = np.concatenate(kept, 0)[:F]
    lo = cell_corners(band, n)[:, None, :]
    fxy = (lo + 0.5 * size + (v - 0.5) * (0.9 * size)).astype(np.float32)
    assert ((fxy > lo + 0.04 * size) & (fxy < lo + 0.96 * size)).all()             # after the rounding to fp32 too
    fxy.setflags(write=False)
    return fxy


def draw_counts(F, choices, seed=0):
    """i64 [F]: the list dealt round to the faces at random (every count of the list is drawn when F >= len(choices))"""
    rng = np.random.default_rng([seed, F, len(choices), 5])
    return np.resize(np.asarray(choices, np.int64), F)[rng.permutation(F)]


def _neighbours(n):
    """i64 [n*n,8]: the faces of the up to eight cells around a cell, -1 beyond the lattice"""
    j, i = np.divmod(np.arange(n * n), n)
    out = []
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if dj or di:
                jj, ii = j + dj, i + di
                out.append(np.where((jj >= 0) & (jj < n) & (ii >= 0) & (ii < n), jj * n + ii, -1))
    return np.stack(out, 1)


def hits(band, fxy, counts, knum, seed=0):
    """-> pix f32 [P,2], face i64 [P,knum], own i64 [P] for counts i64 [F] pixels per face"""
    F = fxy.shape[0]
    n = int(round(F ** 0.5))
    assert n * n == F and counts.shape == (F,)
    rng = np.random.default_rng([seed, F, int(np.sum(counts)), knum, 77])
    own = np.repeat(np.arange(F), counts)
    P = own.shape[0]
    w = rng.dirichlet([2, 2, 2], P)
    w[w.min(1) < MIN_WEIGHT] = 1.0 / 3
    pix = (w[:, :, None] * fxy[own].astype(np.float64)).sum(1)
    face = np.full((P, knum), -1, np.int64)
    face[:, 0] = own
    if knum > 1:
        r = rng.integers(1, knum + 1, P)
        order = np.argsort(rng.random((P, 8)), 1)                    # a random order of the eight neighbours of every pixel,
        nb = np.take_along_axis(_neighbours(n)[own], order, 1)
        nb = np.take_along_axis(nb, np.argsort(nb < 0, 1, kind="stable"), 1)       # those beyond the lattice last
        for s in range(1, knum):
            face[:, s] = np.where(s < r, nb[:, s - 1], -1)           # (a corner cell has three neighbours: a shorter list)
    order = rng.permutation(P)
    pix, face, own = pix[order].astype(np.float32), face[order], own[order]
    assert face.min() >= -1 and face.max() < F
    used = face >= 0
    assert (np.diff(used.astype(np.int8), axis=1) <= 0).all()        # the used slots of a pixel come first
    sf = np.sort(face, 1)
    assert not ((sf[:, 1:] == sf[:, :-1]) & (sf[:, 1:] >= 0)).any()   # no pixel lists a face twice
    return pix, face, own


@functools.lru_cache(maxsize=None)
def case(band, flat, kind, knum, seed=0):
    """One case of the pin: dict(fxy f32 [F,3,2], pix f32 [P,2], face i64 [P,knum], own i64 [P], counts i64 [F], kappa [F],
    asserted bool [F], cls int8 [F], eps, n)."""
    choices, n = LISTS[kind]
    eps = BAND_GEOMETRY[band][2]
    fxy = lattice(band, flat, n, seed)
    counts = draw_counts(n * n, choices, seed)
    pix, face, own = hits(band, fxy, counts, knum, seed)
    k = kappa(fxy, pixel_reach(pix, face, n * n), eps)
    return {"name": case_id(band, flat, kind, knum), "band": band, "flat": flat, "kind": kind, "knum": knum, "n": n, "eps": eps, "fxy": fxy,
            "pix": pix, "face": face, "own": own, "counts": counts, "kappa": k, "asserted": k <= KAPPA_CAP, "cls": RS.classify_faces(fxy, eps)}


def shifted(c, shift=(3.0, -2.0)):
    """The case moved by `shift` cells: a second shape of a batch (the same hit structure on other fp32 values)"""
    size = BAND_GEOMETRY[c["band"]][1]
    d = np.asarray(shift) * size
    fxy = (c["fxy"].astype(np.float64) + d).astype(np.float32)
    pix = (c["pix"].astype(np.float64) + d).astype(np.float32)
    k = kappa(fxy, pixel_reach(pix, c["face"], fxy.shape[0]), c["eps"])
    return dict(c, name=c["name"] + "-shifted", fxy=fxy, pix=pix, kappa=k, asserted=k <= KAPPA_CAP, cls=RS.classify_faces(fxy, c["eps"]))


def hit_counts(c):
    """i64 [F]: the hits of every face over all slots"""
    f = c["face"]
    return np.bincount(f[f >= 0], minlength=c["fxy"].shape[0])


def asserted_share(c):
    """the share of the faces that receive a hit which are asserted"""
    return float(c["asserted"][hit_counts(c) > 0].mean())


def class_counts(cls):
    return tuple(int((cls == k).sum()) for k in (RS.REGULAR, RS.SLIVER, RS.DEGENERATE))


def features(c, D, seed=0):
    """feat f32 [F,3,D], uniform on [0,1) as grids.project_faces makes them"""
    return np.random.default_rng([seed, c["fxy"].shape[0], D, 21]).random((c["fxy"].shape[0], 3, D)).astype(np.float32)


def incoming(c, D, seed=0):
    """gout f32 [P,knum,D]: N(0,1) with magnitudes spread by exp(2 N(0,1)) per slot, so that another order of additions shows"""
    P, knum = c["face"].shape
    rng = np.random.default_rng([seed, P, knum, D, 11])
    return (rng.standard_normal((P, knum, D)) * np.exp(2.0 * rng.standard_normal((P, knum, 1)))).astype(np.float32)


def incoming_heavy_last(c, D, seed=0):
    """incoming() with the gradient of the LAST sorted hit of every face multiplied by the face's hit count, so that this one hit
    weighs about as much as the others together (the "last hit missing" sensitivity case: one average hit of a thousand is 0.1 % of
    the face's sum, which no fp32 bound at kappa = 1e6 can see)"""
    g = incoming(c, D, seed).copy()
    flat_face = c["face"].reshape(-1)
    h = np.nonzero(flat_face >= 0)[0]
    h = h[np.argsort(flat_face[h], kind="stable")]
    f = flat_face[h]
    last = h[np.searchsorted(f, np.unique(f), side="right") - 1]
    g.reshape(-1, D)[last] *= hit_counts(c)[flat_face[last]][:, None].astype(np.float32)
    return g


def sorted_runs(c):
    """(start, stop) i64 [F] of every face's run in the sorted hit order of the backward (by face, ascending slot index inside)"""
    stop = np.cumsum(hit_counts(c))
    return stop - hit_counts(c), stop


def straddles(c, every):
    """bool [F]: the face's run of sorted hits crosses a multiple of `every`"""
    start, stop = sorted_runs(c)
    return (stop > start) & ((start // every) != ((stop - 1) // every))


# ---- a real edge-on view (test 6 of tests/test_raster_bwd_fp64_gpu.py) --------------------------------------------------------------
EDGE_ON_RES, EDGE_ON_ROT, EDGE_ON_KNUM = 10, (0.6155, 0.785), 16     # the cube seen along its space diagonal: one plane family edge-on
EDGE_ON_CLASSES = (1600, 50, 0)                                       # recorded: classify_faces of the 1,650 faces
EDGE_ON_SLIVERS_COVERED = 32                                          # recorded: SLIVER faces in the oracle's NEAREST-16 records (236 hits)
EDGE_ON_MIN_SLIVERS_COVERED = 20


@functools.lru_cache(maxsize=1)
def edge_on_scene():
    """(pix, rngs, fz, fxy, ff, cls): every face of the res-10 Kuhn grid under grids.project_faces(rot=EDGE_ON_ROT), and 1,424 pixels:
    a 32 x 32 grid over the middle 60 % of the image plus, for every SLIVER face, its centroid and seven Dirichlet(2,2,2) points
    (a sliver is under 2 units thick at a pixel pitch of 37: no regular grid of 64 x 64 pixels meets twenty of them).  Whether a pixel
    is covered is left to the rasterizer; the pixels are only put where slivers are."""
    from deftet_amd import grids
    from oracle import oracle as O
    verts, tets = grids.kuhn_grid(EDGE_ON_RES)
    f3 = O.tet_to_face(tets, verts.shape[0], with_boundary=True)[0]
    fz, fxy, ff = grids.project_faces(verts, f3, rot=EDGE_ON_ROT)
    cls = RS.classify_faces(fxy)
    pix, rngs = grids.pixel_grid(32)
    sl = np.nonzero(cls == RS.SLIVER)[0]
    w = np.random.default_rng(0).dirichlet([2, 2, 2], (len(sl), 8))
    w[:, 0] = 1.0 / 3
    extra = (w[..., None] * fxy[0, sl].astype(np.float64)[:, None]).sum(2).reshape(-1, 2).astype(np.float32)
    pix = np.concatenate([pix * np.float32(0.6), extra[None]], 1)
    return pix, np.tile(rngs[:, :1], (1, pix.shape[1], 1)), fz, fxy, ff, cls
