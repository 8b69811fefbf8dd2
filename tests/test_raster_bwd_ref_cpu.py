"""tests/raster_bwd_ref.py and tests/raster_bwd_cases.py kept honest: the CPU half of the fp64 pin of the rasterizer backward
(tests/test_raster_bwd_fp64_gpu.py is the GPU half).

* the analytic fp64 reference is what fp64 torch autograd of the contract's interpolation (oracle.sparse_render_torch) gives;
* the fp32 restatement of k_bwd_sorted's arithmetic stays within the bounds taken with K / 2 in place of K on every asserted face of
  every case, at every feature width the GPU tests run: that is where K comes from (its worst need is recorded as
  K_RESTATEMENT_WORST), and the GPU is held to bounds twice as wide as what the restatement needs on the same inputs;
* the asserted shares and the face classes are the recorded ones, and the required shares hold: conditions on the inputs;
* SENSITIVITY: a restatement with one deliberate defect (gk3 without its w2 term; gn with pp and q swapped; a face's sum without its
  last hit) leaves the bound on at least one asserted face of every image case, so the bound can fail.  The gradients of these
  cases are incoming_heavy_last: the last sorted hit of a face weighs as much as the others together, since one average hit of
  1,023 is a thousandth of the sum and a face at kappa = 1e6 is not known that well in fp32 to begin with.
"""
import numpy as np
import pytest
import torch

from tests import raster_bwd_cases as C
from tests import raster_bwd_ref as R
from tests import raster_scene as RS

WIDTHS = {"image": (4, 3, 6, 9), "unit": (4, 3, 6, 9), "far": (4,)}              # the feature widths the GPU tests run per band
BAND_FLATS = [(b, f) for b in C.BANDS for f in C.FLATS]
BAND_FLAT_IDS = ["%s-%s" % (b, C.FLAT_IDS[f]) for b, f in BAND_FLATS]


def _errors(c, D, g=None, defect=None):
    """(ref, per-face max error of gxy, of gfeat) of the restatement on a case"""
    feat = C.features(c, D)
    g = C.incoming(c, D) if g is None else g
    ref = R.analytic(c["pix"], c["fxy"], feat, c["face"], g, c["eps"])
    gxy, gfeat, _ = R.restatement(c["pix"], c["fxy"], feat, c["face"], g, c["eps"], defect=defect)
    assert not gxy[ref["n"] == 0].any() and not gfeat[ref["n"] == 0].any()
    return ref, np.abs(gxy - ref["gxy"]).max((1, 2)), np.abs(gfeat - ref["gfeat"]).max((1, 2))


@pytest.mark.parametrize("band,flat", BAND_FLATS, ids=BAND_FLAT_IDS)
def test_shares_classes_and_the_construction(band, flat):
    for i, (kind, knum) in enumerate(C.SHARE_ORDER):
        c = C.case(band, flat, kind, knum)
        F, n = c["fxy"].shape[0], c["n"]
        share = C.asserted_share(c)
        print("%s: asserted share %.3f, classes %s, kappa median %.3g max %.3g" % (c["name"], share, C.class_counts(c["cls"]),
                                                                                    np.median(c["kappa"]), c["kappa"].max()))
        assert abs(share - C.ASSERTED_SHARE[(band, flat)][i]) < 5e-4, (c["name"], share)
        assert C.class_counts(c["cls"]) == C.CLASS_COUNTS[(band, flat)][kind], c["name"]
        if band in ("image", "unit") and flat >= 2.0 ** -9:
            assert share >= C.MIN_ASSERTED_SHARE, (c["name"], share)
        if band == "image" and flat == 2.0 ** -13:
            assert share >= C.MIN_ASSERTED_SHARE_IMAGE_FLATTEST, (c["name"], share)
        reg, sli, _ = C.class_counts(c["cls"])
        if flat == 1.0:
            assert reg > 0.9 * F                                     # mostly REGULAR
        if band == "image" and flat <= 2.0 ** -9:
            assert sli > 0.9 * F                                     # mostly SLIVER
        # what a case builds on: fp32, indices in [-1, F), slot 0 the pixel's own face with the drawn count, the block list's size
        assert c["fxy"].dtype == np.float32 and c["pix"].dtype == np.float32 and c["face"].dtype == np.int64
        assert c["face"].min() >= -1 and c["face"].max() < F and np.array_equal(c["face"][:, 0], c["own"])
        assert np.array_equal(np.bincount(c["own"], minlength=F), c["counts"])
        assert set(c["counts"]) == set(C.LISTS[kind][0])             # every count of the list is drawn
        assert c["face"].size <= 66000
        if knum == 1:
            assert np.array_equal(C.hit_counts(c), c["counts"])
        else:
            used = (c["face"] >= 0).sum(1)
            assert used.min() == 1 and used.max() == knum and (C.hit_counts(c) >= c["counts"]).all()
            # a slot beyond 0 holds the face of a neighbouring cell: the pixel lies outside it
            p, s = np.nonzero(c["face"][:, 1:] >= 0)
            a, b = np.divmod(c["face"][p, s + 1], n), np.divmod(c["own"][p], n)
            assert (np.maximum(np.abs(a[0] - b[0]), np.abs(a[1] - b[1])) == 1).all()
    # the runs of the sorted order start at every offset inside a lane (mod 4) and a row (mod 16), and cross waves and blocks
    c = C.case(band, flat, "lane", 1)
    start = C.sorted_runs(c)[0][C.hit_counts(c) > 0]
    assert set(start % 4) == set(range(4)) and set(start % 16) == set(range(16))
    assert C.straddles(c, 256).any() and C.straddles(c, 1024).any() and start.max() > 2048          # more than two blocks
    assert C.straddles(C.case(band, flat, "wave", 1), 1024).any()


def test_kappa_is_what_it_says():
    # the unit right triangle: W = 1, k3 = 1; moved away by 100 the coordinates cost another 101
    t = np.array([[[0, 0], [1, 0], [0, 1]]], np.float64)
    none = np.zeros(1)
    assert np.allclose(C.kappa(t, none, 0.0), 1.0) and np.allclose(C.kappa(t + 100.0, none, 0.0), 101.0)
    assert np.allclose(C.kappa(t * 1e-3, none, 0.0), 1.0)            # scale free
    assert np.allclose(C.kappa(t, np.array([7.0]), 0.0), 7.0)        # a pixel 7 away that hits it
    flat = t.copy()
    flat[0, 2, 1] = 2.0 ** -9
    assert np.allclose(C.kappa(flat, none, 0.0), 512.0) and np.allclose(C.kappa(flat, none, 2.0 ** -9), 256.0)     # den = k3 + eps
    assert np.allclose(C.kappa(t[:, ::-1], none, 0.5), 2.0)          # reversed winding: k3 = -1, den = -0.5
    assert np.allclose(C.kappa0(t), 1.0)


@pytest.mark.parametrize("band,flat", [("image", 2.0 ** -9), ("unit", 1.0), ("far", 2.0 ** -5)])
def test_analytic_reference_is_the_fp64_autograd_of_the_contract(oracle, band, flat):
    for kind, knum, D in (("lane", 5, 4), ("wave", 1, 3)):
        c = C.case(band, flat, kind, knum)
        feat, g = C.features(c, D), C.incoming(c, D)
        ref = R.analytic(c["pix"], c["fxy"], feat, c["face"], g, c["eps"])
        xy = torch.from_numpy(c["fxy"].copy()).double()[None].requires_grad_(True)
        ff = torch.from_numpy(feat).double()[None].requires_grad_(True)
        out = oracle.sparse_render_torch(torch.from_numpy(c["pix"]).double()[None], xy, ff, torch.from_numpy(c["face"])[None],
                                         eps=float(np.float32(c["eps"])))
        (out * torch.from_numpy(g).double()[None]).sum().backward()
        gxy, gff = xy.grad[0].numpy(), ff.grad[0].numpy()
        has = ref["n"] > 0
        assert np.array_equal(ref["n"], C.hit_counts(c)) and has.sum() > 50
        assert (np.abs(ref["gxy"] - gxy).max((1, 2))[has] <= 1e-9 * ref["scale_xy"][has]).all()
        assert (np.abs(ref["gfeat"] - gff).max((1, 2))[has] <= 1e-9 * ref["S_feat"][has]).all()
        assert not ref["gxy"][~has].any() and not ref["gfeat"][~has].any() and not gxy[~has].any()
        assert (ref["S_xy"] <= 3.0 * ref["T_xy"] + 1e-300).all()     # no entry exceeds the scale of its terms
        if knum == 1:                                                # inside, by construction (up to the rounding of the pixel)
            assert ref["w"].min() > 0.04 - c["kappa"][ref["f"]].max() * C.U and np.abs(ref["w"].sum(1) - 1).max() < 1e-9


@pytest.mark.parametrize("band,flat", BAND_FLATS, ids=BAND_FLAT_IDS)
def test_restatement_stays_within_half_of_k(band, flat):
    worst = {"gxy": -np.inf, "gfeat": -np.inf}
    for kind, knum in C.SHARE_ORDER:
        c = C.case(band, flat, kind, knum)
        for D in WIDTHS[band]:
            for s in ([c] if D == 4 else [c, C.shifted(c)]):          # the run-time widths run with a shifted copy as a second shape
                ref, exy, efe = _errors(s, D)
                a = s["asserted"] & (ref["n"] > 0)
                if not a.any():
                    continue
                worst["gxy"] = max(worst["gxy"], R.k_needed_xy(exy, ref, s["kappa"])[a].max())
                worst["gfeat"] = max(worst["gfeat"], R.k_needed_feat(efe, ref, s["kappa"])[a].max())
                assert (exy[a] <= R.bound_xy(ref, s["kappa"], C.K / 2)[a]).all(), (s["name"], D)
                assert (efe[a] <= R.bound_feat(ref, s["kappa"], C.K / 2)[a]).all(), (s["name"], D)
    print("k the restatement needs, %s-%s: %s" % (band, C.FLAT_IDS[flat], {k: "%.3f" % v for k, v in worst.items()}))
    assert max(worst.values()) <= C.K_RESTATEMENT_WORST + 5e-4 <= C.K / 2
    if (band, flat) == ("unit", 1.0):                                # where the recorded worst comes from
        assert worst["gfeat"] >= C.K_RESTATEMENT_WORST - 5e-4
    assert C.K == int(np.ceil(2 * C.K_RESTATEMENT_WORST))


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("flat", C.FLATS, ids=[C.FLAT_IDS[f] for f in C.FLATS])
def test_a_defect_leaves_the_bound_in_every_image_case(flat, defect):
    for kind, knum in C.SHARE_ORDER:
        c = C.case("image", flat, kind, knum)
        ref, exy, efe = _errors(c, 4, g=C.incoming_heavy_last(c, 4), defect=defect)
        a = c["asserted"] & (ref["n"] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rxy, rfe = (exy / R.bound_xy(ref, c["kappa"]))[a], (efe / R.bound_feat(ref, c["kappa"]))[a]
        out = int(((rxy > 1) | (rfe > 1)).sum())
        print("%s, %s: %d of %d asserted faces out of bound, worst error / bound %.3g (gxy) %.3g (gfeat)" % (c["name"], defect, out, a.sum(),
                                                                                                          rxy.max(), rfe.max()))
        assert out >= 1, (c["name"], defect, rxy.max(), rfe.max())
        # and the same inputs without the defect stay inside
        _, exy, efe = _errors(c, 4, g=C.incoming_heavy_last(c, 4))
        assert (exy[a] <= R.bound_xy(ref, c["kappa"])[a]).all() and (efe[a] <= R.bound_feat(ref, c["kappa"])[a]).all()


def test_restatement_adds_in_ascending_sorted_hit_order():
    """three hits on one face whose fp32 sum depends on the order: the restatement's is ascending in p * knum + slot"""
    fxy = np.array([[[0, 0], [1, 0], [0, 1]]], np.float32)
    feat = np.array([[[0.0], [1.0], [2.0]]], np.float32)
    pix = np.array([[0.25, 0.25], [0.25, 0.25], [0.3, 0.1]], np.float32)
    face = np.zeros((3, 1), np.int64)
    g = np.array([[[1e8]], [[-1e8]], [[1.0]]], np.float32)          # (a - a) + b = b, (b - a) + a = 0
    one = [R.restatement(pix[i: i + 1], fxy, feat, face[:1], g[i: i + 1], 0.0)[1][0] for i in range(3)]     # one hit: the term itself
    got = R.restatement(pix, fxy, feat, face, g, 0.0)[1][0]
    assert np.array_equal(got, (one[0] + one[1]) + one[2]) and not np.array_equal(got, (one[2] + one[1]) + one[0])
    assert np.array_equal(R.restatement(pix[::-1], fxy, feat, face, g[::-1], 0.0)[1][0], (one[2] + one[1]) + one[0])
    # two slots of one pixel on two faces, and an unused slot between used ones of other pixels
    face2 = np.array([[0, 1], [1, -1], [-1, -1]], np.int64)
    fxy2 = np.concatenate([fxy, fxy + 2], 0)
    feat2 = np.concatenate([feat, feat], 0)
    g2 = np.ones((3, 2, 1), np.float32)
    gxy, gfeat, w = R.restatement(pix, fxy2, feat2, face2, g2, 0.0)
    ref = R.analytic(pix, fxy2, feat2, face2, g2, 0.0)
    assert list(ref["n"]) == [1, 2] and list(ref["p"]) == [0, 0, 1] and list(ref["slot"]) == [0, 1, 0]
    assert np.allclose(gfeat, ref["gfeat"], rtol=1e-6) and np.allclose(w, ref["w"], rtol=1e-6, atol=1e-6)


def test_the_edge_on_view_has_covered_slivers(oracle):
    """the choice of test 6 of the GPU file, with classify_faces and the oracle alone"""
    pix, rngs, fz, fxy, ff, cls = C.edge_on_scene()
    assert pix.shape[1] <= 64 * 64 and C.EDGE_ON_RES <= 10
    assert C.class_counts(cls) == C.EDGE_ON_CLASSES
    _, face, _ = oracle.sparse_render_fwd(pix, rngs, fz, fxy, ff, knum=C.EDGE_ON_KNUM, omp=True)
    n = np.bincount(face[face >= 0], minlength=fxy.shape[1])
    covered = (cls == RS.SLIVER) & (n > 0)
    k = C.kappa(fxy[0], C.pixel_reach(pix[0], face[0], fxy.shape[1]), 1e-8)
    print("edge-on view: %d SLIVER faces in the records with %d hits, kappa of them <= %.3g" % (covered.sum(), n[covered].sum(), k[covered].max()))
    assert covered.sum() == C.EDGE_ON_SLIVERS_COVERED >= C.EDGE_ON_MIN_SLIVERS_COVERED
    assert (k[covered] <= C.KAPPA_CAP).all()                         # and they are compared, not merely run
    # The restatement on the oracle's face list (the forward is pinned to it bit for bit) stays within the bounds at K.  Not at K / 2,
    # and the scene is no part of K's derivation: its coordinates are three times a face's extent where a lattice's are forty times,
    # so kappa is 3.4 at the median, and one REGULAR face with a single hit needs k = 0.64 for its gfeat.
    g = np.random.default_rng(6).standard_normal((pix.shape[1], C.EDGE_ON_KNUM, ff.shape[3])).astype(np.float32)
    ref = R.analytic(pix[0], fxy[0], ff[0], face[0], g, 1e-8)
    gxy, gfeat, _ = R.restatement(pix[0], fxy[0], ff[0], face[0], g, 1e-8)
    a = (k <= C.KAPPA_CAP) & (n > 0)
    kx = R.k_needed_xy(np.abs(gxy - ref["gxy"]).max((1, 2)), ref, k)[a].max()
    kf = R.k_needed_feat(np.abs(gfeat - ref["gfeat"]).max((1, 2)), ref, k)[a].max()
    print("edge-on view: k the restatement needs %.3f (gxy) %.3f (gfeat), kappa median %.3g over %d asserted faces" % (kx, kf, np.median(k[a]), a.sum()))
    assert a.sum() > 500 and max(kx, kf) <= 0.64 <= C.K
