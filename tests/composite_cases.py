"""Inputs of the fp64 pin of the fused composite (tests/test_composite_ref_cpu.py, tests/test_composite_fp64_gpu.py): pixels with
their ranked hit lists made by construction.  The backward entry deftet_sparse_render_composite_bwd_f32 takes the ranked face
[B,P,knum] as an INPUT, so which slot of which pixel holds which face is decided here; the forward tests give the same stacks face
depths that force the same lists out of the rasterizer.

geometry     the pixels are a random subset of grids.pixel_grid(32) (spacing 62.5).  Every face of a pixel's stack is its own
             triangle: three uniform points of the unit square, kept if well shaped (raster_bwd_cases.kappa0 <= KAPPA0_MAX about
             the centroid), scaled to extent EXTENT = 20 and placed so that the pixel has Dirichlet(2,2,2) weights in it (the
             centroid where min w < 0.05); rounded to fp32.  So every face contains its pixel with weights >= 0.04 and reaches less
             than 40 from it: no other pixel is inside.  Shape and weights are drawn per face: the weights differ from slot to slot.
             Every face is hit exactly once (except in `shared`), three more faces lie at pixels outside the subset and have no hit,
             and the face numbers are shuffled, so the sorted order of the reduction mixes pixels and slots.
counts       TABLE: the hit counts n that must occur per knum — around every window edge (64 ranked slots per window), with and
             without empty slots (Rseed = (knum - n) 1e-10 v_empty), and knum a multiple of 64 with every slot used (the backward's
             count loop ends without its break).  A case deals its counts round to the pixels at random.  The thin cases k65 and
             k128 carry n = 0 in addition: the empty-slot seed is (knum - n) 1e-10 of its terms, half an ulp at the most wherever
             a layer is in front of it, and only a pixel without a layer shows that it is there (test_composite_ref_cpu.py,
             sensitivity).
profiles     PROFILES, the opacity channel; constant over a face's corners except `varying`.  A face that is to have opacity
             EXACTLY 1.0 keeps redrawing its shape and weights until w0 + w1 + w2 is exactly 1 in fp32 and in fp64 (the kernels'
             and the reference's order of operations), so that the carry behind it is exactly zero in both.
depths       the forward tests give face (p, slot) the depth -100 - 2.5 slot - 0.05 p on its three corners: distinct, inside the
             render range [-1000, 0] of grids.pixel_grid, nearest first in construction order.

Recorded on the CPU: K_RESTATEMENT_WORST, the largest k the fp32 restatement of tests/composite_ref.py needs over every asserted
entry of every case; K is twice that, rounded up to an integer (the rule of raster_bwd_cases.K).
"""
import functools

import numpy as np

from deftet_amd import grids
from tests import raster_bwd_cases as RB

U = 2.0 ** -24
TINY = 2.0 ** -126
ALPHA_LO = float(np.float32(1e-10))      # the clamp as the kernels and torch in fp32 have it: [1e-10f, 1.0f] (1 - 1e-10 rounds to 1.0f)
ALPHA_HI = 1.0
EPS = 1e-8
FAR_DEPTH = -6.0
EXTENT = 20.0
MIN_WEIGHT = 0.05
WINDOW = 64

# K: from the fp32 restatement on the CPU, never from a GPU (composite_ref.k_needed; test_composite_ref_cpu.py::
# test_restatement_stays_within_half_of_k).  K_RESTATEMENT_WORST is the restatement's worst need over the layer gradients and the
# forward outputs of every case.
K = 4
K_RESTATEMENT_WORST = 1.741

TABLE = {
    1: (0, 1),
    4: (0, 3, 4),
    63: (62, 63),
    64: (0, 1, 63, 64),
    65: (63, 64, 65),
    128: (64, 65, 127, 128),
    300: (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 299, 300),
}
PROFILES = ("thin", "mid", "opaque", "clamp", "one_at_edge", "nan", "varying")
GRADS = ("all", "colour", "coverage", "depth")
EDGE_SLOTS = (63, 64, 127, 128)          # where one_at_edge puts its opacity of exactly 1.0
NAN_SLOT = 70
SHARED_COUNTS = (65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 299, 300)
THIN_T300_MIN = 0.02


def _spec(name, knum, P, profile, grads="all", depth=0, D=4, bg=1.0, counts=None, B=1, shared=False, stack=None):
    return dict(name=name, knum=knum, P=P, profile=profile, grads=grads, depth=depth, D=D, bg=bg,
                counts=tuple(TABLE[knum] if counts is None else counts), B=B, shared=shared, stack=stack)


# D counts every channel: 2, 4, 6 without a depth channel, 3, 4, 6 with it
SPECS = [
    _spec("k1-P3-thin", 1, 3, "thin", D=2),
    _spec("k4-P5-mid", 4, 5, "mid", depth=1, D=4, bg=0.25),
    _spec("k63-P3-thin", 63, 3, "thin", depth=1, D=3),
    _spec("k64-P4-thin", 64, 4, "thin", D=4),
    _spec("k64-P1-mid", 64, 1, "mid", D=4, counts=(64,)),
    _spec("k65-P4-thin", 65, 4, "thin", depth=1, D=6, bg=0.25, counts=(0,) + TABLE[65]),
    _spec("k128-P5-thin", 128, 5, "thin", D=6, counts=(0,) + TABLE[128]),
    _spec("k128-P4-mid", 128, 4, "mid", depth=1, D=4),
    _spec("k300-P41-thin-all", 300, 41, "thin", depth=1, D=4),
    _spec("k300-P41-thin-colour", 300, 41, "thin", grads="colour", D=4, bg=0.25),
    _spec("k300-P41-thin-coverage", 300, 41, "thin", grads="coverage", D=2),
    _spec("k300-P41-thin-depth", 300, 41, "thin", grads="depth", depth=1, D=6),
    _spec("k300-P41-mid", 300, 41, "mid", depth=1, D=4, bg=0.25),
    _spec("k300-P41-opaque", 300, 41, "opaque", depth=1, D=3),
    _spec("k300-P41-clamp", 300, 41, "clamp", D=4),
    _spec("k300-P41-one_at_edge", 300, 41, "one_at_edge", depth=1, D=4),
    _spec("k300-P41-nan", 300, 41, "nan", depth=1, D=4),
    _spec("k300-P41-varying", 300, 41, "varying", D=4, bg=0.25),
    _spec("k300-P41-thin-B2", 300, 41, "thin", depth=1, D=4, B=2),
    _spec("k300-P41-thin-shared", 300, 41, "thin", depth=1, D=4, counts=SHARED_COUNTS, shared=True),
    _spec("k300-P3-thin-stack320", 300, 3, "thin", depth=1, D=4, counts=(300,), stack=320),
]
CASE_IDS = [s["name"] for s in SPECS]
_BY_NAME = {s["name"]: s for s in SPECS}


def is_multi_window_thin(spec):
    return spec["profile"] == "thin" and spec["knum"] > WINDOW


@functools.lru_cache(maxsize=1)
def all_pixels():
    return grids.pixel_grid(32)[0][0]                                 # f32 [1024,2]


def _weights(rng, m):
    w = rng.dirichlet([2, 2, 2], m)
    w[w.min(1) < MIN_WEIGHT] = 1.0 / 3
    return w


def _triangles(rng, centre):
    """f32 [m,3,2]: one well-shaped triangle of extent EXTENT around every point of centre [m,2], the point at drawn weights"""
    m = centre.shape[0]
    kept, have = [], 0
    while have < m:
        v = rng.random((4 * m + 16, 3, 2))
        r = v - v.mean(1, keepdims=True)
        r = r[RB.kappa0(r) <= RB.KAPPA0_MAX]
        kept.append(r)
        have += r.shape[0]
    r = np.concatenate(kept, 0)[:m]
    r = r * (EXTENT / (r.max(1) - r.min(1)).max(1))[:, None, None]
    w = _weights(rng, m)
    at = (w[:, :, None] * r).sum(1, keepdims=True)
    return (np.asarray(centre, np.float64)[:, None, :] + r - at).astype(np.float32)


def bary(pix, tri, dtype, eps=EPS):
    """(w0, w1, w2) of pix [m,2] in tri [m,3,2], the contract's expression in `dtype` operation by operation"""
    t = dtype
    pix, tri = np.asarray(pix, t), np.asarray(tri, t)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    m, pp, nn, q = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    s, tt = pix[:, 0] - a[:, 0], pix[:, 1] - a[:, 1]
    k1, k2, k3 = s * q - nn * tt, m * tt - s * pp, m * q - nn * pp
    den = k3 + t(eps)                                                # (the kernels receive eps as a float, the fp64 reference as a double)
    w1, w2 = k1 / den, k2 / den
    return t(1) - w1 - w2, w1, w2


def sums_to_one(pix, tri):
    """bool [m]: (w0 + w1) + w2 == 1 exactly in fp32 and in fp64: a face with opacity 1.0 on its corners has a layer of exactly 1.0"""
    ok = np.ones(pix.shape[0], bool)
    for t in (np.float32, np.float64):
        w0, w1, w2 = bary(pix, tri, t)
        ok &= ((w0 + w1) + w2) == t(1)
    return ok


def _deal(rng, counts, P):
    assert P >= len(counts)                                           # every count of the list is dealt
    return np.resize(np.asarray(counts, np.int64), P)[rng.permutation(P)]


def _opacity(rng, spec, n, slot_of, pixel_of):
    """-> (a f32 [H,3] per hit (own faces), exact bool [H]: the opacity is to be exactly 1.0)"""
    H = slot_of.shape[0]
    prof = spec["profile"]
    a = np.repeat(rng.uniform(0.002, 0.02, (H, 1)), 3, 1)
    exact = np.zeros(H, bool)
    if prof == "mid":
        a = np.repeat(rng.uniform(0.05, 0.95, (H, 1)), 3, 1)
    elif prof == "opaque":
        a[:] = 0.9
    elif prof == "clamp":
        kind = rng.choice(4, H, p=[0.66, 0.30, 0.02, 0.02])           # thin, exactly 0, exactly 1, 1.5
        a[kind == 1] = 0.0
        a[kind == 2] = 1.0
        a[kind == 3] = 1.5
        exact = kind == 2
    elif prof == "one_at_edge":
        big = np.nonzero(n > max(EDGE_SLOTS))[0]                      # every other such pixel, the four slots in turn
        for i, p in enumerate(big[::2]):
            h = (pixel_of == p) & (slot_of == EDGE_SLOTS[i % 4])
            a[h], exact[h] = 1.0, True
    elif prof == "nan":
        p = np.nonzero(n > 128)[0][0]
        a[(pixel_of == p) & (slot_of == NAN_SLOT)] = np.nan
    elif prof == "varying":
        a = rng.uniform(0.002, 0.02, (H, 3))
    return a.astype(np.float32), exact


def _shape(spec, b, seed=0):
    """One shape of a case (batch entry b): dict(pix, fxy, fz, feat, face i32 [P,knum], stack i32 [P,S], n, a_exact ...)"""
    knum, P, D = spec["knum"], spec["P"], spec["D"]
    rng = np.random.default_rng([seed, SPECS.index(spec), b, 3])
    sel = np.random.default_rng([seed, SPECS.index(spec), 1]).permutation(all_pixels().shape[0])    # the same pixels in every shape
    pix = all_pixels()[sel[:P]]
    n = _deal(np.random.default_rng([seed, SPECS.index(spec), 2]), spec["counts"], P)
    if b > 0:                                                          # shorter lists at the same pixels: the count before it in the table
        table = np.asarray(sorted(set(spec["counts"])))
        n = table[np.maximum(np.searchsorted(table, n) - 1, 0)]
    S = spec["stack"] or knum
    length = np.full(P, S) if spec["stack"] else n                     # faces per stack
    own_len = length - 1 if spec["shared"] else length
    pixel_of = np.repeat(np.arange(P), own_len)
    rank_of = np.concatenate([np.arange(k) for k in own_len]) if P else np.zeros(0, np.int64)
    if spec["shared"]:                                                 # the shared face takes a slot of 64 or more: the own faces step over it
        at = np.array([rng.integers(WINDOW, k) for k in n])
        slot_of = rank_of + (rank_of >= at[pixel_of])
    else:
        slot_of = rank_of
    H = pixel_of.shape[0]
    tri = _triangles(rng, pix[pixel_of])
    a, exact = _opacity(rng, spec, n, slot_of, pixel_of)
    for _ in range(200):
        bad = np.nonzero(exact & ~sums_to_one(pix[pixel_of], tri))[0]
        if not bad.size:
            break
        tri[bad] = _triangles(rng, pix[pixel_of[bad]])
    assert not (exact & ~sums_to_one(pix[pixel_of], tri)).any()
    spare = _triangles(rng, all_pixels()[sel[P: P + 3]])               # three faces no pixel of the case is in
    parts_xy, parts_z = [tri, spare], [-100.0 - 2.5 * slot_of - 0.05 * pixel_of, np.full(3, -500.0)]
    if spec["shared"]:
        parts_xy.append(np.array([[[-3000.0, -2500.0], [3000.0, -2500.0], [0.0, 4000.0]]], np.float32))
        parts_z.append(np.array([-100.0 - 2.5 * WINDOW - 2.25]))       # behind slot 64 of every pixel, in front of slot 65
    fxy0, fz0 = np.concatenate(parts_xy, 0), np.concatenate(parts_z, 0)
    F = fxy0.shape[0]
    feat0 = rng.random((F, 3, D)).astype(np.float32)
    ach = 1 if spec["depth"] else 0
    if spec["depth"]:
        feat0[:, :, 0] = rng.uniform(-5.0, -1.0, (F, 3)).astype(np.float32)
    feat0[:, :, ach] = np.repeat(rng.uniform(0.002, 0.02, (F, 1)), 3, 1).astype(np.float32)
    feat0[:H, :, ach] = a
    number = rng.permutation(F)                                        # face h of the construction is face number[h] of the case
    fxy, fz, feat = np.empty_like(fxy0), np.empty((F, 3), np.float32), np.empty_like(feat0)
    fxy[number], feat[number] = fxy0, feat0
    fz[number] = np.repeat(fz0[:, None], 3, 1).astype(np.float32)
    stack = np.full((P, S), -1, np.int32)
    stack[pixel_of, slot_of] = number[:H]
    if spec["shared"]:
        stack[np.arange(P), at] = number[F - 1]
    face = np.ascontiguousarray(stack[:, :knum])
    exact_face = np.zeros(F, bool)
    exact_face[number[:H]] = exact
    out = dict(pix=pix, fxy=fxy, fz=fz, feat=feat, face=face, stack=stack, n=np.minimum(length, knum), exact_one=exact_face,
               shared_face=int(number[F - 1]) if spec["shared"] else -1, spare=number[H: H + 3])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _pad_faces(sh, F):
    """the shape with faces without a hit appended up to F (the shapes of a batch share F)"""
    add = F - sh["fxy"].shape[0]
    if add == 0:
        return sh
    out = dict(sh)
    for k in ("fxy", "fz", "feat"):
        out[k] = np.concatenate([sh[k], np.repeat(sh[k][sh["spare"][:1]], add, 0)], 0)   # copies of a face no pixel is in
        out[k].setflags(write=False)
    out["exact_one"] = np.concatenate([sh["exact_one"], np.zeros(add, bool)])
    return out


def incoming(spec, seed=0):
    """(g_colour [B,P,Dc], g_coverage [B,P,1], g_depth [B,P,1]) f32 N(0,1), None for the outputs the case's loss does not use"""
    B, P, Dc = spec["B"], spec["P"], spec["D"] - (2 if spec["depth"] else 1)
    rng = np.random.default_rng([seed, SPECS.index(spec), 9])
    gc, gv, gd = (rng.standard_normal((B, P, k)).astype(np.float32) for k in (Dc, 1, 1))
    which = spec["grads"]
    return (gc if which in ("all", "colour") else None, gv if which in ("all", "coverage") else None,
            gd if which in ("all", "depth") and spec["depth"] else None)


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """dict(spec, shapes: B dicts of _shape, g: incoming)"""
    spec = _BY_NAME[name]
    assert spec["grads"] != "depth" or spec["depth"]
    shapes = [_shape(spec, b, seed) for b in range(spec["B"])]
    F = max(sh["fxy"].shape[0] for sh in shapes)
    shapes = [_pad_faces(sh, F) for sh in shapes]
    assert spec["P"] * spec["knum"] <= 66000
    return dict(spec=spec, shapes=shapes, g=incoming(spec, seed))


def shape_grads(c, b):
    """the incoming gradients of shape b: (g_colour [P,Dc], g_coverage [P], g_depth [P]) or None each"""
    gc, gv, gd = c["g"]
    return (None if gc is None else gc[b], None if gv is None else gv[b, :, 0], None if gd is None else gd[b, :, 0])
