"""The full-size rasterizer scenes and the pixels on which the GPU result is compared with the CPU oracle.

The oracle (oracle/deftet_oracle_render.c) tests every face against every pixel: 521,850 faces x 262,144 pixels is out of
reach, 16 k pixels are a few seconds on 16 threads.  A uniform sample of that size would meet about five of the 330 pixels
that a sliver face of the BASELINE view covers, so the pixels are CHOSEN: `select_pixels` finds, with the oracle alone, the
pixels that the faces on the rasterizer's special paths cover, adds their neighbourhoods, the image border and a random rest.
Nothing here looks at a GPU result.
"""
import functools

import numpy as np

from deftet_amd import grids

REGULAR, SLIVER, DEGENERATE = 0, 1, 2
NEAREST, FIRST = 0, 1

SCENES = {"baseline": {}, "axis_aligned": {"rot": (0.0, 0.0)}}       # keyword arguments of grids.project_faces; 512 x 512 pixels
N_PIX = 512


def classify_faces(face_xy, eps=1e-8):
    """Class of every face of face_xy [F,3,2] (or [1,F,3,2]) as the rasterizer's face_box sees it (raster.hip, the comment
    block above face_box), in fp32 with the kernel's operation order:
        finite     all six |coordinates| <= 2^20
        k3         (bx-ax)(cy-ay) - (cx-ax)(by-ay), each product and the difference rounded to fp32
        w          the larger extent of the bounding box
        REGULAR    finite, |k3| >= 2^-7 w^2,  |k3| >= 1024 |eps|, w > 0
        SLIVER     not regular, finite, |k3| >= 2^-16 w^2, |k3| >= 1024 |eps|, w > 0, w >= 2^-16 max|coordinate|
        DEGENERATE everything else (it keeps the unbounded entry of the wide list)
    Returns an int8 array [F]."""
    xy = np.asarray(face_xy, np.float32)
    if xy.ndim == 4:
        assert xy.shape[0] == 1
        xy = xy[0]
    f32 = np.float32
    eps = f32(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = xy[:, 0], xy[:, 1], xy[:, 2]
        finite = (np.abs(xy).reshape(len(xy), 6) <= f32(1048576.0)).all(1)          # NaN compares false
        m, pp, n, q = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
        k3 = m * q - n * pp
        lox, hix = np.fmin(a[:, 0], np.fmin(b[:, 0], c[:, 0])), np.fmax(a[:, 0], np.fmax(b[:, 0], c[:, 0]))
        loy, hiy = np.fmin(a[:, 1], np.fmin(b[:, 1], c[:, 1])), np.fmax(a[:, 1], np.fmax(b[:, 1], c[:, 1]))
        w = np.fmax(hix - lox, hiy - loy)
        ww = w * w
        big_enough = (np.abs(k3) >= f32(1024.0) * np.abs(eps)) & (w > 0)
        regular = finite & (np.abs(k3) >= f32(2.0 ** -7) * ww) & big_enough
        cmax = np.fmax(np.fmax(np.abs(lox), np.abs(hix)), np.fmax(np.abs(loy), np.abs(hiy)))
        sliver = ~regular & finite & (np.abs(k3) >= f32(2.0 ** -16) * ww) & big_enough & (w >= f32(2.0 ** -16) * cmax)
    assert k3.dtype == np.float32 and ww.dtype == np.float32 and cmax.dtype == np.float32       # no fp64 crept in
    cls = np.full(len(xy), DEGENERATE, np.int8)
    cls[sliver] = SLIVER
    cls[regular] = REGULAR
    return cls


def adversarial_soup():
    """(pix, rngs, fz, fxy, ff): 400 faces (small ones, zero-area, collinear, NaN / Inf / huge, duplicate, reversed, out of the
    depth range) and 1,500 pixels (on vertices, NaN, Inf, huge, a narrow depth window)"""
    rng = np.random.default_rng(3)
    F = 400
    fxy = rng.uniform(-1, 1, (1, F, 3, 2)).astype(np.float32)
    fxy[0, :150] = fxy[0, :150] * 0.1 + rng.uniform(-0.9, 0.9, (150, 1, 2)).astype(np.float32)     # small faces (tiles)
    fxy[0, 150:160, 2] = fxy[0, 150:160, 0]                                                          # zero area
    fxy[0, 160:165, 2] = (fxy[0, 160:165, 0] + fxy[0, 160:165, 1]) / 2                               # collinear
    fxy[0, 165, 0, 0] = np.nan
    fxy[0, 166, 1] = np.inf
    fxy[0, 167] *= 1e7
    fxy[0, 168] = fxy[0, 3]                                                                          # duplicate face
    fxy[0, 169] = fxy[0, 5][::-1]                                                                    # reversed winding
    fz = rng.uniform(-5, -1, (1, F, 3)).astype(np.float32)
    fz[0, 170:175] = 5.0                                                                             # outside the depth range
    ff = rng.random((1, F, 3, 5)).astype(np.float32)
    P = 1500
    pix = rng.uniform(-1.1, 1.1, (1, P, 2)).astype(np.float32)
    pix[0, :100] = fxy[0, rng.integers(0, 150, 100), rng.integers(0, 3, 100)]                        # on vertices
    pix[0, 100] = np.nan
    pix[0, 101, 0] = np.inf
    pix[0, 102] = 3e6
    rngs = np.tile(np.array([-1000.0, 0.0], np.float32), (1, P, 1))
    rngs[0, 200:300] = [-3.0, -2.0]                                                                  # narrow depth window
    return pix, rngs, fz, fxy, ff


class Selection:
    """sel: the sorted unique union; set1..set4 as described at select_pixels (set4: the random pixels that were ADDED, disjoint from
    the other three); cls: classify_faces of the scene; blocks: number of 8 x 8 blocks that hold a set-1 pixel, before the cap"""
    def __init__(self, sel, set1, set2, set3, set4, cls, blocks):
        self.sel, self.set1, self.set2, self.set3, self.set4, self.cls, self.blocks = sel, set1, set2, set3, set4, cls, blocks

    def sizes(self):
        return {"set1": len(self.set1), "set2": len(self.set2), "set3": len(self.set3), "set4": len(self.set4), "total": len(self.sel),
                "blocks": self.blocks}


def select_pixels(pix, rngs, fz, fxy, ff, seed, eps=1e-8, total=16384, max_blocks=64):
    """Pixel indices (into the row-major n x n image `pix` [1, n*n, 2]) for the comparison with the oracle:
      1. every pixel covered by a non-regular face (sliver or degenerate): the oracle run on those faces alone over ALL pixels.
         Only "covered by at least one" is asked, so the run is FIRST with knum = 1 — it stops at a pixel's first kept face
         and its output stays at one slot per pixel whatever the number of covering faces (2,500 on the diagonal of the
         axis-aligned view);
      2. all pixels of the 8 x 8 pixel blocks that hold a pixel of set 1; more than `max_blocks` such blocks: the max_blocks
         with the most set-1 pixels, ties by block index (set 1 itself is never cut);
      3. the first and last row and column at stride 8, and the four corners;
      4. a seeded uniform sample of the remaining pixels that brings the total to `total` (none if sets 1-3 already reach it).
    """
    from oracle import oracle as O
    P = pix.shape[1]
    n = int(round(P ** 0.5))
    assert pix.shape[0] == 1 and n * n == P and n % 8 == 0
    cls = classify_faces(fxy, eps)
    nr = np.nonzero(cls != REGULAR)[0]
    if len(nr):
        _, face, _ = O.sparse_render_fwd(pix, rngs, fz[:, nr], fxy[:, nr], ff[:, nr][..., :1], knum=1, eps=eps, policy=FIRST, omp=True)
        set1 = np.nonzero(face[0, :, 0] >= 0)[0]
    else:
        set1 = np.zeros(0, np.int64)
    nb = n // 8
    blk = (set1 // n // 8) * nb + (set1 % n) // 8
    ids, cnt = np.unique(blk, return_counts=True)
    order = np.lexsort((ids, -cnt))[:max_blocks]                       # most set-1 pixels first, then the lower block index
    by, bx = np.divmod(ids[order], nb)
    dy, dx = np.divmod(np.arange(64), 8)
    set2 = np.unique(((by[:, None] * 8 + dy[None]) * n + bx[:, None] * 8 + dx[None]).ravel())
    s = np.arange(0, n, 8)
    set3 = np.unique(np.concatenate([s, (n - 1) * n + s, s * n, s * n + n - 1, [0, n - 1, (n - 1) * n, n * n - 1]]))
    fixed = np.unique(np.concatenate([set1, set2, set3]))
    rest = np.setdiff1d(np.arange(P), fixed)
    need = min(max(total - len(fixed), 0), len(rest))
    set4 = np.sort(np.random.default_rng(seed).choice(rest, need, replace=False))
    sel = np.unique(np.concatenate([fixed, set4]))
    return Selection(sel, set1, set2, set3, set4, cls, len(ids))


@functools.lru_cache(maxsize=2)
def scene(name, res=70):
    """(pix, rngs, fz, fxy, ff) of a full-size scene: every unique face of the res-70 Kuhn grid under the named camera, 512^2 rays"""
    from oracle import oracle as O
    verts, tets = grids.kuhn_grid(res)
    f3, _, _, _, _ = O.tet_to_face(tets, verts.shape[0], with_boundary=True)
    fz, fxy, ff = grids.project_faces(verts, f3, **SCENES[name])
    pix, rngs = grids.pixel_grid(N_PIX)
    return pix, rngs, fz, fxy, ff


@functools.lru_cache(maxsize=2)
def selection(name, seed=0):
    return select_pixels(*scene(name), seed=seed)


@functools.lru_cache(maxsize=4)
def oracle_rows(name, knum, policy):
    """(feat, face, w) of the oracle on the selected pixels of a scene (cached: the composite tests ask for the same rows again)"""
    from oracle import oracle as O
    pix, rngs, fz, fxy, ff = scene(name)
    sel = selection(name).sel
    return O.sparse_render_fwd(pix[:, sel], rngs[:, sel], fz, fxy, ff, knum=knum, policy=policy, omp=True)


def record_depths(face, w, fz):
    """fp32 depth of every slot of an oracle record (face [R,K], w [R,K,3]) in the contract's order (w0 z0 + w1 z1) + w2 z2;
    NaN in the unused slots"""
    zz = fz[0][np.clip(face, 0, None)]
    z = (w[..., 0] * zz[..., 0] + w[..., 1] * zz[..., 1]) + w[..., 2] * zz[..., 2]
    assert z.dtype == np.float32
    return np.where(face >= 0, z, np.float32(np.nan))


def depth_tie_pairs(face, w, fz):
    """number of adjacent valid slots with bit-equal depth — order that only the face index decides"""
    z = record_depths(face, w, fz)
    return int((z[:, 1:] == z[:, :-1]).sum())                     # NaN (unused slot) never compares equal
