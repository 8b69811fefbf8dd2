"""CPU tests of the render oracle's OpenMP entry and of the pixel selection of the full-size rasterizer tests
(tests/raster_scene.py): the parallel entry must give the serial entry's bits, and the selection must be what it says."""
import numpy as np
import pytest

from tests import raster_scene as RS


def _same(a, b):
    for x, y in zip(a, b):                                             # feat, face, w
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))      # bit for bit: signed zeros and NaN payloads included


@pytest.mark.parametrize("policy", [RS.NEAREST, RS.FIRST])
def test_omp_entry_equals_serial_on_the_adversarial_soup(oracle, policy):
    pix, rngs, fz, fxy, ff = RS.adversarial_soup()
    for knum in (8, 300):
        serial = oracle.sparse_render_fwd(pix, rngs, fz, fxy, ff, knum=knum, policy=policy)
        _same(serial, oracle.sparse_render_fwd(pix, rngs, fz, fxy, ff, knum=knum, policy=policy, omp=True))
        assert (serial[1] >= 0).sum() > 1000


@pytest.mark.parametrize("policy", [RS.NEAREST, RS.FIRST])
def test_omp_entry_equals_serial_on_the_res70_scene(oracle, policy):
    pix, rngs, fz, fxy, ff = RS.scene("baseline")
    sel = np.sort(np.random.default_rng(5).choice(pix.shape[1], 512, replace=False))
    serial = oracle.sparse_render_fwd(pix[:, sel], rngs[:, sel], fz, fxy, ff, knum=64, policy=policy)
    _same(serial, oracle.sparse_render_fwd(pix[:, sel], rngs[:, sel], fz, fxy, ff, knum=64, policy=policy, omp=True))
    n = (serial[1] >= 0).sum(-1)
    assert (n == 64).mean() > 0.5 and (n == 0).any()


def test_omp_entry_batches_and_empty_inputs(oracle):
    """B > 1 (the parallel loop runs over batch x pixel) and the empty shapes"""
    pix, rngs, fz, fxy, ff = RS.adversarial_soup()
    rep = lambda a, s: np.concatenate([a, (a * np.float32(s)).astype(np.float32)], 0)
    args = (rep(pix[:, :300], 0.5), rep(rngs[:, :300], 1.0), rep(fz, 1.0), rep(fxy, 0.8), rep(ff, 0.5))
    serial = oracle.sparse_render_fwd(*args, knum=5)
    _same(serial, oracle.sparse_render_fwd(*args, knum=5, omp=True))
    assert (serial[1][0] >= 0).any() and (serial[1][1] >= 0).any() and not np.array_equal(serial[1][0], serial[1][1])
    feat, face, w = oracle.sparse_render_fwd(pix[:, :0], rngs[:, :0], fz, fxy, ff, knum=4, omp=True)
    assert face.shape == (1, 0, 4)
    feat, face, w = oracle.sparse_render_fwd(pix[:, :7], rngs[:, :7], fz[:, :0], fxy[:, :0], ff[:, :0], knum=4, omp=True)
    assert (face == -1).all() and (feat == 0).all() and (w == 0).all()


def test_classify_faces_classes():
    """one face per clause of face_box's classification"""
    tri = lambda h, L=100.0, o=0.0: [[o, o], [o + L, o], [o + L / 2, o + h]]
    u = 2.0 ** -9                                                      # the spacing of fp32 numbers near 30,000
    xy = np.array([
        tri(50.0),                     # well shaped
        tri(100.0 * 2.0 ** -5),        # area 2^-5 of the extent squared: still regular (2^-7 is the limit)
        tri(100.0 * 2.0 ** -9),        # sliver
        tri(100.0 * 2.0 ** -15),       # sliver
        tri(u, 204 * u, 1000.0),       # sliver: area 1/204 of the extent squared, extent 0.4 at coordinates ~1,000
        tri(100.0 * 2.0 ** -18),       # thinner than 2^-16: degenerate
        tri(0.0),                      # collinear
        [[1, 1], [1, 1], [1, 1]],      # a point: w = 0
        tri(1e-3 * 2.0 ** -9, 1e-3),   # a sliver so small that |k3| < 1024 eps
        tri(u, 204 * u, 30000.0),      # the same sliver as above at coordinates ~30,000: its extent is below 2^-16 of them
        tri(50.0, 100.0, 2.0e6),       # beyond 2^20
        [[np.nan, 0], [1, 0], [0, 1]],
        [[0, 0], [np.inf, 0], [0, 1]],
    ], np.float32)
    want = [RS.REGULAR, RS.REGULAR, RS.SLIVER, RS.SLIVER, RS.SLIVER] + [RS.DEGENERATE] * 8
    assert RS.classify_faces(xy, 1e-8).tolist() == want
    assert RS.classify_faces(xy[None], 1e-8).tolist() == want
    # |k3| = 5000, 312, 19.5, 0.31 against 1024 eps = 10.24
    assert RS.classify_faces(xy[:4], 1e-2).tolist() == [RS.REGULAR, RS.REGULAR, RS.SLIVER, RS.DEGENERATE]
    assert RS.classify_faces(xy[:4], -1e-2).tolist() == [RS.REGULAR, RS.REGULAR, RS.SLIVER, RS.DEGENERATE]


def test_select_pixels_sets(oracle):
    """The four sets on a small scene where set 1 can be found another way (the unbounded record of the non-regular faces): a
    128 x 128 image, regular faces, a dozen slivers and a collinear face."""
    from deftet_amd import grids
    n = 128
    rng = np.random.default_rng(2)
    pix, rngs = grids.pixel_grid(n)
    F = 300
    fxy = (rng.uniform(-900, 900, (F, 1, 2)) + rng.uniform(-80, 80, (F, 3, 2))).astype(np.float32)
    for i in range(12):                                                # slivers ~ 50 pixels long, a fifth of a pixel pitch wide or less
        a = rng.uniform(-700, 700, 2)
        th = rng.uniform(0, np.pi)
        d, dp = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
        L = 800.0
        fxy[20 * i] = [a, a + L * d, a + 0.5 * L * d + L * 2.0 ** -(8 + i % 4) * dp]
    fxy[5, 2] = (fxy[5, 0] + fxy[5, 1]) / 2                            # collinear
    fxy = fxy[None]
    fz = rng.uniform(-5, -1, (1, F, 3)).astype(np.float32)
    ff = rng.random((1, F, 3, 4)).astype(np.float32)
    S = RS.select_pixels(pix, rngs, fz, fxy, ff, seed=1, total=3000, max_blocks=6)
    nr = np.nonzero(S.cls != RS.REGULAR)[0]
    assert (S.cls == RS.SLIVER).sum() >= 10 and (S.cls == RS.DEGENERATE).sum() >= 1
    full = oracle.sparse_render_fwd(pix, rngs, fz[:, nr], fxy[:, nr], ff[:, nr], knum=len(nr) + 1)[1][0]
    assert (full[:, -1] == -1).all()
    want1 = np.nonzero((full >= 0).any(-1))[0]
    assert np.array_equal(S.set1, want1) and len(want1) > 20
    # set 2: whole 8 x 8 blocks, the six with the most set-1 pixels, the lower block index on a tie
    blk = lambda p: (p // n // 8) * (n // 8) + (p % n) // 8
    ids, cnt = np.unique(blk(S.set1), return_counts=True)
    assert S.blocks == len(ids) > 6
    got_blocks, n_in = np.unique(blk(S.set2), return_counts=True)
    assert len(got_blocks) == 6 and (n_in == 64).all() and np.isin(got_blocks, ids).all()
    kept = np.isin(ids, got_blocks)
    assert cnt[kept].min() >= cnt[~kept].max()
    at_cut = cnt == cnt[kept].min()                                    # blocks that tie at the cut: the lower indices were taken
    assert not (~kept[at_cut][:-1] & kept[at_cut][1:]).any()
    # set 3: border pixels only, all four corners, stride 8 along each side
    r, c = np.divmod(S.set3, n)
    assert ((r == 0) | (r == n - 1) | (c == 0) | (c == n - 1)).all() and np.isin([0, n - 1, (n - 1) * n, n * n - 1], S.set3).all()
    assert len(S.set3) == 4 * (n // 8)               # (0, 0) is on two sides; the far corner is the one pixel no stride reaches
    # set 4 and the union
    fixed = np.unique(np.concatenate([S.set1, S.set2, S.set3]))
    assert not np.isin(S.set4, fixed).any() and len(np.unique(S.set4)) == len(S.set4)
    assert np.array_equal(S.sel, np.unique(np.concatenate([fixed, S.set4]))) and len(S.sel) == 3000
    assert (np.diff(S.sel) > 0).all() and S.sel.min() >= 0 and S.sel.max() < n * n
    again = RS.select_pixels(pix, rngs, fz, fxy, ff, seed=1, total=3000, max_blocks=6)
    assert np.array_equal(again.sel, S.sel)
    other = RS.select_pixels(pix, rngs, fz, fxy, ff, seed=2, total=3000, max_blocks=6)
    assert np.array_equal(other.set1, S.set1) and not np.array_equal(other.set4, S.set4)
    small = RS.select_pixels(pix, rngs, fz, fxy, ff, seed=1, total=10, max_blocks=6)                  # sets 1-3 are never cut
    assert np.array_equal(small.sel, fixed) and len(small.set4) == 0
