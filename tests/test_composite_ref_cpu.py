"""The CPU half of the fp64 pin of the fused composite (tests/composite_cases.py, tests/composite_ref.py;
tests/test_composite_fp64_gpu.py is the GPU half): the cases contain what they claim, the fp32 restatement of the two kernels stays
within HALF the per-entry bounds (K is derived from it, never from a GPU), the closed form the bounds are made of equals the fp64
autograd the GPU is compared with, and the bounds can fail: one planted defect at a time leaves them.

Sensitivity, as measured (largest k needed, layer gradients / forward outputs; K = 4):
  T restarts at 1 at slot 64               2.6e5 and more on every multi-window thin case.  It is an error of the size of the
                                           value itself at slot 64 under ANY norm (max-norm 3.9 on k128-P4-mid): the forward at
                                           knum = 300 of test_render_composite_gpu.py sees it; no gradient test had a second window.
  Q not carried into the window before     1e3 .. 9e4; max-norm on the mid profile 4.5e-7 (k128), 3.7e-7 (k300)
  vNext and aNext taken as 0 at lane 63    1e3 .. 9e4; max-norm on the mid profile 4.5e-7, 3.7e-7
  the last used slot has a successor       2e4 .. 2e7 (slot n evaluated as the zero layer it is: Q_{n-1} = v_{n-1} - v_empty);
                                           max-norm 4.5e-7 on k128-P4-mid, where every pixel has 64 layers or more in front.  (On
                                           k300-P41-mid a pixel with ONE layer has its last slot in front: visible to any norm.)
  Rseed omitted (both kernels' seed)       the seed is (knum - n) 1e-10 of its terms: at most 300e-10 = half an ulp of v_empty,
                                           which stands next to it in Q_{n-1} = v_{n-1} - Rseed and in V_{n-1} of the bound.  No
                                           fp32 bound can see it behind a layer; a pixel WITHOUT a layer has a coverage of exactly
                                           knum 1e-10 and sees it (k 1.7e7).  Every thin case with the table's counts has such a
                                           pixel (k65 and k128 carry n = 0 for this); `shared` and `stack320` cannot have one, and
                                           there the defect stays inside the bound, which is asserted as what it is.
"""
import functools
import math

import numpy as np
import pytest

from tests import composite_cases as C
from tests import composite_ref as CR
from tests import raster_bwd_ref as R

SHAPES = [(s["name"], b) for s in C.SPECS for b in range(s["B"])]
SHAPE_IDS = ["%s[%d]" % x for x in SHAPES]
MID_CASES = ("k128-P4-mid", "k300-P41-mid")
NO_EMPTY_PIXEL = ("k300-P41-thin-shared", "k300-P3-thin-stack320")


def inputs(name, b):
    c = C.case(name)
    sp, sh = c["spec"], c["shapes"][b]
    return sp, sh, (sh["pix"], sh["fxy"], sh["feat"], sh["face"], C.shape_grads(c, b), sp["depth"], sp["bg"])


@functools.lru_cache(maxsize=None)
def evaluated(name, b):
    """(exact, restatement, analytic) of a shape, computed once and left unchanged"""
    _, _, args = inputs(name, b)
    return CR.exact(*args), CR.restatement(*args), CR.analytic(*args)


def reduced(sh, G):
    """the fp32 face reduction (raster_bwd_ref.restatement) of fp32 layer gradients"""
    gxy, gfeat, _ = R.restatement(sh["pix"], sh["fxy"], sh["feat"], sh["face"].astype(np.int64), G, C.EPS)
    return gxy, gfeat


def clean_pixels(ex):
    return np.isfinite(ex["cov"])


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_cases_contain_what_they_claim():
    pairs, Ps, profiles, grads, widths, bgs = set(), set(), set(), set(), set(), set()
    grid = C.all_pixels().astype(np.float64)
    for name, b in SHAPES:
        sp, sh, _ = inputs(name, b)
        P, knum = sh["face"].shape
        assert (P, knum) == (sp["P"], sp["knum"]) and P * knum <= 66000
        used = sh["face"] >= 0
        assert (used == (np.arange(knum)[None] < sh["n"][:, None])).all()
        if b == 0:
            pairs |= {(knum, int(n)) for n in sh["n"]}
        Ps.add(P), profiles.add(sp["profile"]), grads.add(sp["grads"]), widths.add((sp["depth"], sp["D"])), bgs.add(sp["bg"])
        F = sh["fxy"].shape[0]
        stack = sh["stack"]
        hits = np.bincount(stack[stack >= 0], minlength=F)
        if sp["shared"]:
            f = sh["shared_face"]
            at = np.argwhere(sh["face"] == f)
            assert hits[f] == P and (at[:, 1] >= C.WINDOW).all() and len(set(at[:, 1])) > 8      # in every list, behind the first window
            hits[f] = 1
        assert hits.max() == 1 and (hits == 0).sum() >= 3               # one hit per face; faces without a hit
        # every face of a stack contains its pixel, with weights >= 0.04, and reaches less than a pixel spacing from it
        p, s = np.nonzero(stack >= 0)
        own = stack[p, s] != sh["shared_face"]
        p, f = p[own], stack[p, s][own]
        w = np.stack(C.bary(sh["pix"][p], sh["fxy"][f], np.float64), 1)
        assert w.min() >= 0.04
        reach = np.abs(sh["fxy"][f].astype(np.float64) - sh["pix"][p].astype(np.float64)[:, None]).max((1, 2))
        assert reach.max() < 40.0 < 62.5
        for q in range(0, len(f), 997):                                 # and spot-checked against the whole pixel grid
            wq = np.stack(C.bary(grid, np.repeat(sh["fxy"][f[q]][None], len(grid), 0), np.float64), 1)
            assert (wq.min(1) >= 0).sum() == 1
        one = sh["exact_one"][f]
        assert C.sums_to_one(sh["pix"][p][one], sh["fxy"][f][one]).all()
    for knum, counts in C.TABLE.items():
        for n in counts:
            assert (knum, n) in pairs, (knum, n)
    assert Ps == {1, 3, 4, 5, 41} and profiles == set(C.PROFILES) and grads == set(C.GRADS) and bgs == {1.0, 0.25}
    assert widths >= {(0, 2), (0, 4), (0, 6), (1, 3), (1, 4), (1, 6)}
    assert sum(C.is_multi_window_thin(s) for s in C.SPECS) >= 8


def test_profiles_are_what_they_claim():
    ex = evaluated("k300-P41-thin-all", 0)[0]
    full = ex["n"] == 300
    assert full.any() and (ex["T_end"][full] >= C.THIN_T300_MIN).all()            # every window carries weight
    ex = evaluated("k300-P41-opaque", 0)[0]
    assert (ex["T"][ex["n"] >= 64, 63] < C.TINY).all()                            # T leaves the fp32 normal range in the first window
    sp, sh, _ = inputs("k300-P41-clamp", 0)
    a = sh["feat"][sh["face"][sh["face"] >= 0]][:, 0, 0]
    assert (a == 0.0).sum() > 500 and (a == 1.0).sum() > 20 and (a == 1.5).sum() > 20
    ex = evaluated("k300-P41-clamp", 0)[0]
    masked = ex["used"] & ~ex["passes"]
    assert masked.sum() > 500 and (ex["used"] & (ex["alpha"] == 1.0) & ex["passes"]).sum() > 20   # exactly 1.0 passes, 0.0 and 1.5 do not
    sp, sh, _ = inputs("k300-P41-one_at_edge", 0)
    ex = evaluated("k300-P41-one_at_edge", 0)[0]
    p, s = np.nonzero(ex["used"] & (ex["alpha"] == 1.0))
    assert set(s) == set(C.EDGE_SLOTS) and (ex["T"][p, s + 1] == 0.0).all() and (ex["T"][p, s] > 0.1).all()    # the carry is exactly zero
    sp, sh, _ = inputs("k300-P41-varying", 0)
    f = sh["face"][sh["face"] >= 0]
    assert (sh["feat"][f][:, 0, 0] != sh["feat"][f][:, 1, 0]).all()
    an = evaluated("k300-P41-varying", 0)[2]
    assert np.abs(an["gxy"]).max() > 0
    c = C.case("k300-P41-thin-B2")
    n0, n1 = c["shapes"][0]["n"], c["shapes"][1]["n"]
    assert (n1 <= n0).all() and (n1 < n0).sum() >= 38 and np.array_equal(c["shapes"][0]["pix"], c["shapes"][1]["pix"])
    sh = C.case("k300-P3-thin-stack320")["shapes"][0]
    assert sh["stack"].shape == (3, 320) and (sh["stack"] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("name,b", SHAPES, ids=SHAPE_IDS)
def test_closed_form_equals_autograd(name, b):
    """the closed form the bounds are made of, reduced by face in fp64, is the fp64 autograd the GPU is compared with"""
    sp, sh, args = inputs(name, b)
    ex, _, an = evaluated(name, b)
    red = R.analytic(sh["pix"], sh["fxy"], sh["feat"], sh["face"].astype(np.int64), ex["G"], C.EPS)
    bxy, bfeat, _, _ = CR.face_bounds(*args[:4], ex)
    for got, want, bound in ((red["gxy"], an["gxy"], bxy), (red["gfeat"], an["gfeat"], bfeat)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want) & np.isfinite(bound)                     # (a face of the NaN pixel has no bound: the pattern only)
        assert (np.abs(got - want)[ok] <= 1e-6 * bound[ok] + 1e-300).all()        # fp64 against fp64: a millionth of the fp32 bound
    ok = clean_pixels(ex)
    fb = CR.forward_bounds(ex)
    for key, bound in (("colour", fb[0]), ("cov", fb[1])) + ((("dep", fb[2]),) if sp["depth"] else ()):
        assert np.array_equal(np.isnan(ex[key]), np.isnan(an[key]))
        # (alpha_composite's lower limit is 1e-10, the kernels' and the closed form's is 1e-10f: 1.3e-18 apart, per empty slot)
        assert (np.abs(ex[key] - an[key])[ok] <= 1e-6 * bound[ok] + 6 * sp["knum"] * abs(C.ALPHA_LO - 1e-10)).all()
    if not CR.needs_fp32_limits(*args[2:4], sp["depth"]):
        lim = CR.analytic(*args, composite=CR.composite_fp32_limits)              # the fp32 limits change nothing where they do not act
        slack = 6 * sp["knum"] * abs(C.ALPHA_LO - 1e-10)
        for key, bound in (("colour", fb[0]), ("cov", fb[1]), ("gxy", bxy), ("gfeat", bfeat)):
            ok = ~np.isnan(an[key]) & np.isfinite(bound)
            assert (np.abs(lim[key] - an[key])[ok] <= 1e-6 * bound[ok] + slack).all()


def test_fp32_limits_are_needed_where_an_opacity_is_one():
    names = [s["name"] for s in C.SPECS if CR.needs_fp32_limits(C.case(s["name"])["shapes"][0]["feat"], C.case(s["name"])["shapes"][0]["face"], s["depth"])]
    assert names == ["k300-P41-clamp", "k300-P41-one_at_edge"]
    import torch
    from deftet_amd.render import alpha_composite
    layers = torch.tensor([[[[1.0, 0.5], [0.3, 0.7]]]], dtype=torch.float32, requires_grad=True)     # fp32: an opacity of 1.0 passes its gradient
    c, v, _ = alpha_composite(layers)
    (g,) = torch.autograd.grad(c.sum() + 2 * v.sum(), layers)
    l64 = layers.detach().double().requires_grad_(True)
    c64, v64, _ = CR.composite_fp32_limits(l64, None, 1.0, -6.0)
    (g64,) = torch.autograd.grad(c64.sum() + 2 * v64.sum(), l64)
    assert g[0, 0, 0, 0].item() != 0 and torch.allclose(g.double(), g64, rtol=1e-6, atol=1e-7)
    (gm,) = torch.autograd.grad(sum(x.sum() for x in alpha_composite(l64)[:2]), l64)
    assert gm[0, 0, 0, 0].item() == 0                                # in fp64 alpha_composite masks it: not what the operator computes


# ---------------------------------------------------------------------------------------------------------------- K
def test_restatement_stays_within_half_of_k():
    worst, entries, asserted = -np.inf, 0, 0
    for name, b in SHAPES:
        sp, sh, args = inputs(name, b)
        ex, rs, an = evaluated(name, b)
        ok = clean_pixels(ex)
        assert ok.all() or sp["profile"] == "nan"
        kl = CR.k_needed_layers(rs["G"], ex)[ok]
        kf = CR.k_needed_forward(rs, ex)[ok]
        worst = max(worst, float(kf.max()), float(kl.max()) if kl.size else -np.inf)
        # entry by entry, with K / 2: the layer gradients, the forward outputs, and gxy / gfeat after the fp32 face reduction
        E = CR.layer_bound(ex, C.K / 2)
        assert (np.abs(rs["G"].astype(np.float64) - ex["G"])[ok] <= E[ok]).all()
        assert not rs["G"][~ex["used"]].any()
        entries += int(ex["used"][ok].sum()) * sp["D"]
        asserted += int(np.isfinite(E[ok][ex["used"][ok]]).sum())
        fb = CR.forward_bounds(ex, C.K / 2)
        for key, bound in (("colour", fb[0]), ("cov", fb[1])) + ((("dep", fb[2]),) if sp["depth"] else ()):
            assert (np.abs(rs[key].astype(np.float64) - an[key])[ok] <= bound[ok]).all(), (name, key)
        bxy, bfeat, nf, _ = CR.face_bounds(*args[:4], ex, k=C.K / 2)
        gxy, gfeat = reduced(sh, rs["G"])
        clean_face = np.isfinite(an["gfeat"]).all((1, 2))
        for got, want, bound in ((gxy, an["gxy"], bxy), (gfeat, an["gfeat"], bfeat)):
            assert (np.abs(got.astype(np.float64) - want)[clean_face] <= bound[clean_face]).all(), name
            assert not got[nf == 0].any() and not want[nf == 0].any()
    # the share of the entries that is asserted is 1: every used slot of every pixel without a NaN, no mask
    assert asserted == entries > 300000
    assert abs(worst - C.K_RESTATEMENT_WORST) <= 0.02 * C.K_RESTATEMENT_WORST, worst
    assert C.K == math.ceil(2 * C.K_RESTATEMENT_WORST) and worst <= C.K / 2


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def needs(name, b, defect):
    """(largest k the defective restatement needs over layer gradients and forward outputs, its max-norm errors against fp64)"""
    sp, sh, args = inputs(name, b)
    ex, _, an = evaluated(name, b)
    rs = CR.restatement(*args, defect=defect)
    k = max(float(CR.k_needed_layers(rs["G"], ex).max()), float(CR.k_needed_forward(rs, ex).max()))
    gxy, gfeat = reduced(sh, rs["G"])
    maxnorm = max(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), C.TINY)      # (gxy is all zero under a coverage-only loss)
                  for got, want in ((gxy, an["gxy"]), (gfeat, an["gfeat"]), (rs["colour"], an["colour"]), (rs["cov"], an["cov"])))
    return k, float(maxnorm)


THIN = [(s["name"], b) for s in C.SPECS if C.is_multi_window_thin(s) for b in range(s["B"])]


@pytest.mark.parametrize("defect", CR.DEFECTS)
def test_a_planted_defect_leaves_the_bound_on_every_multi_window_thin_case(defect):
    assert len(THIN) >= 9
    for name, b in THIN:
        k, _ = needs(name, b, defect)
        if defect == CR.DEFECTS[3] and name in NO_EMPTY_PIXEL:
            # no pixel without a layer: the seed is below half an ulp of what it is added to (the module docstring)
            assert (C.case(name)["shapes"][b]["n"] >= C.WINDOW).all() and k <= C.K / 2, (name, k)
            continue
        if defect == CR.DEFECTS[3]:
            assert (C.case(name)["shapes"][b]["n"] == 0).any()
        assert k > C.K, (name, b, defect, k)


def test_max_norm_on_the_mid_profile_misses_the_dropped_carries():
    """why the comparisons before this pin could not see them: behind twenty layers of the mid profile T is below 1e-5"""
    for name in MID_CASES:
        for defect in (CR.DEFECTS[1], CR.DEFECTS[2], CR.DEFECTS[3]):
            k, maxnorm = needs(name, 0, defect)
            assert maxnorm <= 1e-5, (name, defect, maxnorm)
            assert k > C.K or defect == CR.DEFECTS[3]                       # while the per-entry bound sees the carries there too
    k, maxnorm = needs("k128-P4-mid", 0, CR.DEFECTS[4])                            # every pixel has 64 layers or more
    assert maxnorm <= 1e-5 and k > C.K
    k, maxnorm = needs("k128-P4-mid", 0, CR.DEFECTS[0])                            # T = 1 at slot 64 is an error of order one under any norm
    assert maxnorm > 1.0 and k > C.K


# ---------------------------------------------------------------------------------------------------------------- NaN
def test_nan_case_follows_the_references_pattern():
    sp, sh, args = inputs("k300-P41-nan", 0)
    ex, rs, an = evaluated("k300-P41-nan", 0)
    bad = ~clean_pixels(ex)
    assert bad.sum() == 1 and sh["n"][bad][0] > C.NAN_SLOT
    for key in ("colour", "cov", "dep"):
        assert np.array_equal(np.isnan(rs[key]), np.isnan(an[key])) and np.isnan(an[key][bad]).all() and not np.isnan(an[key][~bad]).any()
    gxy, gfeat = reduced(sh, rs["G"])
    assert np.array_equal(np.isnan(gxy), np.isnan(an["gxy"])) and np.array_equal(np.isnan(gfeat), np.isnan(an["gfeat"]))
    faces = sh["face"][bad][0][: sh["n"][bad][0]]
    touched = np.zeros(sh["fxy"].shape[0], bool)
    touched[faces] = True
    assert np.isnan(an["gxy"][touched]).all() and not np.isnan(an["gxy"][~touched]).any() and not np.isnan(an["gfeat"][~touched]).any()
    a = 1
    front, behind = faces[: C.NAN_SLOT], faces[C.NAN_SLOT + 1:]
    assert np.isnan(an["gfeat"][front][:, :, a]).all() and not np.isnan(an["gfeat"][front][:, :, [0, 2, 3]]).any()   # in front: the opacity only
    assert np.isnan(an["gfeat"][behind]).all()
    assert (an["gfeat"][faces[C.NAN_SLOT]][:, a] == 0).all()                       # the NaN itself is outside the clamp: masked
