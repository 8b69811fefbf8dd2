"""The rasterizer backward (k_bwd_runs and k_bwd_sorted of csrc/raster.hip; DESIGN.md section 6, "What is pinned")
against fp64 on faces of known conditioning and on the edges of the reduction (tests/raster_bwd_cases.py; test_raster_bwd_ref_cpu.py
is the CPU half and says where K and KAPPA_CAP come from).  Every call goes to deftet_sparse_render_bwd_f32 with a face list made
by construction — which pixel hits which face, and how many hits a face collects: 4 per lane, 256 per wave, 1,024 per block for
k_bwd_runs, 64 and 1,024 for k_bwd_sorted — so nothing depends on the forward's coverage.  Per ASSERTED face (kappa <= KAPPA_CAP),
with u = 2^-24 and K = raster_bwd_cases.K:

    gxy     max|err| <= (K kappa_f + n_f) u scale_xy[f] + K D u T_xy[f]          gfeat   max|err| <= (K kappa_f + n_f) u S_feat[f]

1 bound         default path (k_bwd_runs, D = 4): band x flat x {lane, wave, block} x knum 1, 5; faces without a hit exactly zero; two
                runs bit-equal on every face with at most 1,024 hits (larger ones meet through atomics: the bound only).
2 width         k_bwd_sorted: D = 3, 6, 9, B = 2 (the second shape a shifted copy with other features), bands image and unit.
3 unaligned     the image cases of 1 with the features 4 bytes off a 16-byte boundary, which sends D = 4 to k_bwd_sorted (the
                library's launch counters say which kernel ran): the same bounds, and the two kernels agree within the sum of
                their bounds.
4 isolation     the gout rows of every hit of about 5 % of the faces (some at a wave edge, some at a block edge of the sorted order)
                set to NaN or +Inf: every OTHER face with at most 1,024 hits is bit-equal to the run with those rows zeroed, the
                poisoned faces are non-finite.
5 weights       the forward's out_w on a flat = 2^-9 lattice and the backward's recomputed weights (gout = 1 in channel 0: gfeat[f,:,0]
                of a face with one hit IS (w0, w1, w2)), bit for bit.
6 edge-on       a res-10 Kuhn grid seen along the cube's diagonal through autograd, knum = 16: per-face bounds on the face list
                the forward returned (32 SLIVER faces are in it; the regular-scene tests of test_raster_gpu.py keep global bounds).

DEGENERATE and unasserted faces are in the inputs on purpose and carry hits; they are never compared with a bound, but their
neighbours in the sorted order are.  Worst error / bound of an MI355X run: profiles/raster_bwd_tolerances.jsonl.
"""
import numpy as np
import pytest
import torch

from tests import raster_bwd_cases as C
from tests import raster_bwd_kernels as K
from tests import raster_bwd_ref as R
from tests import raster_scene as RS
from tests.tol import check_bound

pytestmark = pytest.mark.gpu

RUNS_BLOCK = 1024                      # sorted hits per block of k_bwd_runs and of k_bwd_sorted: larger faces meet through atomics


def _t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)                       # (a copy: the cases' arrays are read-only)


def backward(dev, pix, fxy, feat, face, gout, eps, unaligned=False):
    """deftet_sparse_render_bwd_f32 on numpy inputs with a leading batch axis -> (gxy [B,F,3,2], gfeat [B,F,3,D]) as numpy; the
    outputs are filled with NaN before the call (the entry clears them).  unaligned: the features start 4 bytes off a 16-byte
    boundary."""
    from deftet_amd import _lib
    lib = _lib.load()
    B, P, knum = face.shape
    F, D = fxy.shape[1], feat.shape[3]
    assert pix.shape == (B, P, 2) and fxy.shape == (B, F, 3, 2) and feat.shape == (B, F, 3, D) and gout.shape == (B, P, knum, D)
    assert face.dtype == np.int64 and face.min() >= -1 and face.max() < F           # no index is out of range
    tp, txy, tff, tface, tg = (_t(x, dev) for x in (pix, fxy, feat, face, gout))
    if unaligned:
        tff = K.off_by_four_bytes(tff)
    assert tff.data_ptr() % 16 == (4 if unaligned else 0) and tg.data_ptr() % 16 == 0
    assert tp.dtype == txy.dtype == tff.dtype == tg.dtype == torch.float32
    gxy = torch.full_like(txy, float("nan"))
    gff = torch.full_like(tff, float("nan"))
    with _lib.on_device(dev):
        ws = _lib.workspace(dev, lib.deftet_sparse_render_bwd_workspace_bytes(B, P, F, knum))
        _lib.check(lib.deftet_sparse_render_bwd_f32(_lib.ptr(tp), _lib.ptr(txy), _lib.ptr(tff), _lib.ptr(tface), None, _lib.ptr(tg),
                                                    _lib.ptr(gxy), _lib.ptr(gff), B, P, F, D, knum, float(eps), _lib.ptr(ws), ws.numel(),
                                                    _lib.current_stream(dev)), "deftet_sparse_render_bwd_f32")
    torch.cuda.synchronize()
    return gxy.cpu().numpy(), gff.cpu().numpy()


def run_case(dev, c, D=4, gout=None, shapes=None, unaligned=False):
    """the backward on a case (or on `shapes`, cases of one structure as a batch) with its seeded features and gradients"""
    shapes = [c] if shapes is None else shapes
    feat = np.stack([C.features(s, D, seed=b) for b, s in enumerate(shapes)])
    g = np.stack([C.incoming(s, D, seed=b) for b, s in enumerate(shapes)]) if gout is None else gout
    out = backward(dev, np.stack([s["pix"] for s in shapes]), np.stack([s["fxy"] for s in shapes]), feat,
                   np.stack([s["face"] for s in shapes]), g, c["eps"], unaligned=unaligned)
    return feat, g, out


def hold(tag, c, feat, g, gxy, gfeat):
    """one shape against fp64 within its bounds on the asserted faces; exactly zero without a hit.  -> (ref, worst ratios)"""
    ref = R.analytic(c["pix"], c["fxy"], feat, c["face"], g, c["eps"])
    a = c["asserted"] & (ref["n"] > 0)
    worst = (check_bound(tag + ", gxy", gxy, ref["gxy"], R.bound_xy(ref, c["kappa"])[:, None, None], mask=a[:, None, None]),
             check_bound(tag + ", gfeat", gfeat, ref["gfeat"], R.bound_feat(ref, c["kappa"])[:, None, None], mask=a[:, None, None]))
    none = ref["n"] == 0
    assert not gxy[none].any() and not gfeat[none].any()
    return ref, worst


def small_faces(c):
    """bool [F]: at most 1,024 hits — written in a fixed order whatever the run's place in the sorted order (a run of 1,024 that
    straddles a block edge adds two partial sums into the cleared output: two terms, either order the same bits)"""
    return C.hit_counts(c) <= RUNS_BLOCK


# ------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("band,flat,kind,knum", C.CASES, ids=C.CASE_IDS)
def test_bound_default_path(cuda, band, flat, kind, knum):
    c = C.case(band, flat, kind, knum)
    feat, g, (gxy, gfeat) = run_case(cuda, c)
    ref, _ = hold("raster bwd pin, %s, k_bwd_runs" % c["name"], c, feat[0], g[0], gxy[0], gfeat[0])
    assert np.array_equal(ref["n"], C.hit_counts(c)) and ((ref["n"] == 0).any() or (kind, knum) != ("lane", 1))
    _, _, (gxy2, gfeat2) = run_case(cuda, c)
    s = small_faces(c)
    assert (s.any() or (kind, knum) == ("block", 5)) and np.array_equal(gxy[0][s], gxy2[0][s], equal_nan=True) and np.array_equal(gfeat[0][s], gfeat2[0][s], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("D", [3, 6, 9])
@pytest.mark.parametrize("band,flat,kind,knum", [x for x in C.CASES if x[0] != "far"], ids=[i for i in C.CASE_IDS if not i.startswith("far")])
def test_bound_run_time_width(cuda, band, flat, kind, knum, D):
    c = C.case(band, flat, kind, knum)
    shapes = [c, C.shifted(c)]
    feat, g, (gxy, gfeat) = run_case(cuda, c, D=D, shapes=shapes)
    assert not np.array_equal(feat[0], feat[1]) and not np.array_equal(shapes[0]["fxy"], shapes[1]["fxy"])
    for b, s in enumerate(shapes):
        hold("raster bwd pin, %s[%d], k_bwd_sorted D=%d" % (c["name"], b, D), s, feat[b], g[b], gxy[b], gfeat[b])
    _, _, (gxy2, gfeat2) = run_case(cuda, c, D=D, shapes=shapes)
    s = small_faces(c)
    assert np.array_equal(gxy[:, s], gxy2[:, s], equal_nan=True) and np.array_equal(gfeat[:, s], gfeat2[:, s], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------- 3
IMAGE_CASES = [x for x in C.CASES if x[0] == "image"]


def test_bound_and_agreement_of_the_sorted_kernel_on_unaligned_features(cuda):
    """D = 4 with features that are not 16-byte aligned goes to k_bwd_sorted: both kernels in this process, on the same inputs"""
    ran = 0
    for x in IMAGE_CASES:
        c = C.case(*x)
        feat, g, (gxy, gfeat) = K.ran_only(b"k_bwd_runs", lambda: run_case(cuda, c))
        sfeat_in, sg, (sxy, sfeat) = K.ran_only(b"k_bwd_sorted", lambda: run_case(cuda, c, unaligned=True))
        assert np.array_equal(sfeat_in, feat) and np.array_equal(sg, g)
        sxy, sfeat = sxy[0], sfeat[0]
        tag = "raster bwd pin, %s, k_bwd_sorted, D=4 unaligned" % c["name"]
        ref, _ = hold(tag, c, feat[0], g[0], sxy, sfeat)
        a = (c["asserted"] & (ref["n"] > 0))[:, None, None]
        check_bound(tag + " vs k_bwd_runs, gxy", sxy, gxy[0], 2 * R.bound_xy(ref, c["kappa"])[:, None, None], mask=a)
        check_bound(tag + " vs k_bwd_runs, gfeat", sfeat, gfeat[0], 2 * R.bound_feat(ref, c["kappa"])[:, None, None], mask=a)
        assert not sxy[ref["n"] == 0].any() and not sfeat[ref["n"] == 0].any()
        ran += 1
    assert ran == len(IMAGE_CASES) == 24


# ------------------------------------------------------------------------------------------------------------------------- 4
def poisoned_faces(c, seed=0):
    """about 5 % of the faces with a hit (two at the least): first one whose run of sorted hits crosses a block edge (a multiple of
    1,024), then one that crosses a wave edge of k_bwd_runs (256) and one of k_bwd_sorted (64) only, then one that ENDS on a wave
    edge and one that STARTS on one, the rest at random"""
    n = C.hit_counts(c)
    start, stop = C.sorted_runs(c)
    rng = np.random.default_rng([seed, n.shape[0], 31])
    want = max(2, int(round(0.05 * (n > 0).sum())))
    groups = [C.straddles(c, 1024), C.straddles(c, 256) & ~C.straddles(c, 1024), C.straddles(c, 64) & ~C.straddles(c, 256),
              (n > 0) & (stop % 256 == 0), (n > 0) & (start % 256 == 0), (n > 0) & (stop % 64 == 0), n > 0]
    chosen = []
    for grp in groups:
        for f in rng.permutation(np.nonzero(grp)[0]):
            if f not in chosen and f - 1 not in chosen and f + 1 not in chosen:     # a poisoned face has clean neighbours in the order
                chosen.append(int(f))
                break
    rest = [int(f) for f in rng.permutation(np.nonzero(n > 0)[0]) if f not in chosen]
    chosen += rest[: max(0, want - len(chosen))]
    return np.array(sorted(chosen[: max(want, 2)])), groups


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("kind,knum,D", [("wave", 1, 4), ("wave", 5, 4), ("block", 1, 4), ("lane", 5, 4), ("wave", 5, 6), ("block", 1, 3)])
def test_a_non_finite_face_stays_alone(cuda, kind, knum, D, poison):
    c = C.case("image", 2.0 ** -5, kind, knum)
    bad, groups = poisoned_faces(c)
    n = C.hit_counts(c)
    assert len(bad) >= 2 and (n[bad] > 0).all()
    if kind != "lane":
        assert groups[0][bad].any() and (groups[1][bad].any() or kind == "block")   # at a block edge, at a wave edge
    g = C.incoming(c, D)
    rows = np.isin(c["face"], bad)                                   # [P,knum]: every hit of a poisoned face
    g_bad, g_zero = g.copy(), g.copy()
    g_bad[rows], g_zero[rows] = poison, 0.0
    _, _, (bxy, bfeat) = run_case(cuda, c, D=D, gout=g_bad[None])
    _, _, (zxy, zfeat) = run_case(cuda, c, D=D, gout=g_zero[None])
    other = np.ones(n.shape[0], bool)
    other[bad] = False
    same = other & small_faces(c)
    assert same.sum() >= 2 and np.isfinite(zxy).all() and np.isfinite(zfeat).all()
    assert np.array_equal(bxy[0][same].view(np.int32), zxy[0][same].view(np.int32))
    assert np.array_equal(bfeat[0][same].view(np.int32), zfeat[0][same].view(np.int32))
    assert np.isfinite(bxy[0][other]).all() and np.isfinite(bfeat[0][other]).all()               # the large faces too
    assert not np.isfinite(bxy[0][bad]).any() and not np.isfinite(bfeat[0][bad]).any()
    assert not zxy[0][bad].any() and not zfeat[0][bad].any()         # (w * 0 summed: the zeroed faces are exactly zero)


# ------------------------------------------------------------------------------------------------------------------------- 5
MIN_SINGLE_HIT_FACES = 100             # the oracle gives 106 such faces on this lattice (counted in the test before the GPU is asked)


def test_backward_recomputes_the_forwards_weights_bit_for_bit(cuda, oracle):
    from deftet_amd import _lib
    c = C.case("image", 2.0 ** -9, "lane", 1)
    F, P = c["fxy"].shape[0], c["pix"].shape[0]
    pix, fxy = c["pix"][None], c["fxy"][None]
    rngs = np.tile(np.array([-1000.0, 0.0], np.float32), (1, P, 1))
    fz = np.full((1, F, 3), -1.0, np.float32)
    feat = C.features(c, 4)[None]
    _, oface, _ = oracle.sparse_render_fwd(pix, rngs, fz, fxy, feat, knum=1, eps=c["eps"])
    on = np.bincount(oface[oface >= 0], minlength=F)
    assert (on == 1).sum() == 106 >= MIN_SINGLE_HIT_FACES
    lib = _lib.load()
    tp, tr, tz, txy, tff = (_t(x, cuda) for x in (pix, rngs, fz, fxy, feat))
    ofeat = torch.empty(1, P, 1, 4, device=cuda)
    face = torch.empty(1, P, 1, dtype=torch.int64, device=cuda)
    w = torch.full((1, P, 1, 3), float("nan"), device=cuda)
    with _lib.on_device(cuda):
        ws = _lib.workspace(cuda, lib.deftet_sparse_render_workspace_bytes(1, P, F, 1))
        _lib.check(lib.deftet_sparse_render_fwd_policy_f32(_lib.ptr(tp), _lib.ptr(tr), _lib.ptr(tz), _lib.ptr(txy), _lib.ptr(tff), _lib.ptr(ofeat),
                                                           _lib.ptr(face), _lib.ptr(w), 1, P, F, 4, 1, float(c["eps"]), RS.NEAREST, _lib.ptr(ws),
                                                           ws.numel(), _lib.current_stream(cuda)), "deftet_sparse_render_fwd_policy_f32")
    torch.cuda.synchronize()
    face, w = face.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(face, oface)
    hit = face[0, :, 0] >= 0
    assert (face[0, hit, 0] == c["own"][hit]).all()                  # disjoint faces: a pixel can only be in its own
    n = np.bincount(face[0, hit, 0], minlength=F)
    single = np.nonzero(n == 1)[0]
    assert len(single) >= MIN_SINGLE_HIT_FACES
    g = np.zeros((1, P, 1, 4), np.float32)
    g[..., 0] = 1.0
    _, gfeat = backward(cuda, pix, fxy, feat, face, g, c["eps"])
    pixel_of = np.full(F, -1)
    pixel_of[face[0, hit, 0]] = np.nonzero(hit)[0]
    want = w[0, pixel_of[single], 0]                                 # [S,3]
    assert np.isfinite(want).all() and (want != 0).all()
    assert np.array_equal(gfeat[0, single, :, 0].view(np.int32), want.view(np.int32))
    assert not gfeat[0, single, :, 1:].any()


# ------------------------------------------------------------------------------------------------------------------------- 6
def test_edge_on_view_through_autograd_per_face(cuda):
    from deftet_amd.render import deftet_sparse_render
    pix, rngs, fz, fxy, ff, cls = C.edge_on_scene()
    tp, tr, tz = (_t(x, cuda) for x in (pix, rngs, fz))
    txy, tff = _t(fxy, cuda).requires_grad_(True), _t(ff, cuda).requires_grad_(True)
    feat, face = deftet_sparse_render(tp, tr, tz, txy, tff, knum=C.EDGE_ON_KNUM, policy=RS.NEAREST)
    face_np = face.cpu().numpy()
    g = np.random.default_rng(6).standard_normal(tuple(feat.shape)).astype(np.float32)      # (the gradients test_raster_bwd_ref_cpu.py uses)
    gxy, gfeat = torch.autograd.grad(feat, (txy, tff), _t(g, cuda))
    F = fxy.shape[1]
    ref = R.analytic(pix[0], fxy[0], ff[0], face_np[0], g[0], 1e-8)
    kappa = C.kappa(fxy[0], C.pixel_reach(pix[0], face_np[0], F), 1e-8)
    a = (kappa <= C.KAPPA_CAP) & (ref["n"] > 0)
    covered = (cls == RS.SLIVER) & (ref["n"] > 0)
    assert (covered & a).sum() >= C.EDGE_ON_MIN_SLIVERS_COVERED and a.sum() > 500
    tag = "raster bwd pin, edge-on res %d k%d through autograd" % (C.EDGE_ON_RES, C.EDGE_ON_KNUM)
    check_bound(tag + ", gxy", gxy[0].cpu().numpy(), ref["gxy"], R.bound_xy(ref, kappa)[:, None, None], mask=a[:, None, None])
    check_bound(tag + ", gfeat", gfeat[0].cpu().numpy(), ref["gfeat"], R.bound_feat(ref, kappa)[:, None, None], mask=a[:, None, None])
    check_bound(tag + ", gxy of the slivers", gxy[0].cpu().numpy(), ref["gxy"], R.bound_xy(ref, kappa)[:, None, None], mask=(covered & a)[:, None, None])
    none = ref["n"] == 0
    assert none.any() and not gxy[0].cpu().numpy()[none].any() and not gfeat[0].cpu().numpy()[none].any()
