"""The CPU side of the winding-number contract: tests/winding_ref.py — the fp64 restatement of the tree of
winding_number.hip — is checked against the plain fp64 sum of check_sign_ref.py, its error E0 is measured again and compared with the
recorded one, and the inputs of test_winding_gpu.py are shown to be fair: the points a classification test sets aside stay under
caps that are conditions on the inputs, not measurements.

Measured here (3,000 uniform + 1,000 near-surface points per mesh, beta = 3): E0 = 1.637e-2 (shell8; per mesh: sphere8 2.3e-3,
sphere24 9.0e-3, torus24x12 1.26e-2, shell8 1.64e-2, mixed8 1.9e-3, open8 2.1e-3, open24 9.2e-3, flipped8 2.7e-3, sphere2 3e-16,
sphere4 4.6e-4, sphere12 1.19e-2, sphere33 1.27e-2).  beta = 2 gives 3.3e-2 and beta = 2.5 1.9e-2 over the same set.
Set aside: open8 / open24 1.9 % / 2.1 % of the points within 0.1 of 0.5 (0.95 % / 0.97 % within 0.05); watertight meshes at most
0.075 %."""
import json
import os

import numpy as np
import pytest

from tests import check_sign_ref as R
from tests import winding_cases as W
from tests import winding_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_depth_chooser_and_the_depths_the_cases_cover():
    assert [T.levels(F) for F in (0, 1, 12, 15, 16, 63, 64, 224, 255, 256, 1023, 1024, 4095, 4096, 100000, 1 << 30)] == \
        [0, 0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5, 5]
    assert sorted({T.levels(W.case(n)[1].shape[0]) for n in W.FAST_CASES}) == [0, 1, 2, 3, 4, 5]
    assert T.level_offset(0) == 0 and T.level_offset(1) == 1 and T.level_offset(2) == 9 and T.level_offset(6) == 37449


def test_cases_are_what_they_claim():
    for name in W.MAKERS:
        v, f, p = W.case(name)
        assert v.dtype == np.float32 and f.dtype == np.int64 and p.shape == (W.N_UNIFORM + W.N_NEAR, 3) and p.dtype == np.float32
    full = W.case("sphere8")[1].shape[0]
    assert W.case("open8")[1].shape[0] < full and W.case("flipped8")[1].shape[0] == full
    w = W.exact64("flipped8")
    assert round(float(w.min())) == -1 and np.abs(w - np.round(w)).max() < 1e-6
    assert round(float(W.exact64("mixed8").max())) == 2
    w = W.exact64("open8")
    assert 0.1 < float(np.abs(w - np.round(w)).max()) <= 0.5          # an open mesh: not an integer everywhere


def test_tree_nodes_cover_their_faces_and_sum_to_the_mesh():
    v, f, _ = W.case("torus24x12")
    tree = T.build(v, f)
    L, tri, seg = tree["L"], tree["tri"], tree["seg"]
    assert L == 3 and seg[-1] == f.shape[0] and sorted(tree["order"]) == list(range(f.shape[0]))
    area_vec = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    for l in range(L + 1):
        N, rad, C, A = tree["levels"][l]
        assert np.allclose(N.sum(0), area_vec.sum(0), atol=1e-12) and np.isclose(A.sum(), np.linalg.norm(area_vec, axis=1).sum())
        span = 1 << (3 * (L - l))                                     # the leaves below node m are m span .. (m + 1) span
        for m in range(1 << (3 * l)):
            s, e = seg[m * span], seg[(m + 1) * span]
            assert (rad[m] < 0) == (s == e)
            if e > s:
                assert np.linalg.norm(tri[s:e].reshape(-1, 3) - C[m][None], axis=1).max() <= rad[m] * (1 + 1e-12)


@pytest.mark.parametrize("name", ["sphere8", "mixed8", "open8", "flipped8"])
def test_exact_restatement_is_the_reference_sum(name):
    v, f, p = W.case(name)
    assert float(np.abs(T.exact(v, f, p) - W.exact64(name)).max()) <= 1e-12


def test_E0_is_the_recorded_one_and_meets_the_condition():
    worst = {}
    for name in W.E0_CASES:
        v, f, p = W.case(name)
        w, n_node, n_face = T.fast(T.build(v, f), p, W.BETA)
        worst[name] = float(np.abs(w - W.exact64(name)).max())
        print("%-11s F=%5d L=%d  E0=%.3e  node terms %.0f  exact faces %.0f" % (name, f.shape[0], T.levels(f.shape[0]), worst[name],
                                                                               n_node.mean(), n_face.mean()))
    e0 = max(worst.values())
    print("E0 = %.6e (recorded %.6e)" % (e0, W.E0))
    assert abs(e0 - W.E0) <= 1e-6 * W.E0
    assert W.E_FAST == 2.0 * W.E0 and W.E_FAST <= W.E_FAST_CAP and W.EXACT_TOL <= 1e-3 and W.BETA == T.BETA


def test_recorded_tolerances_are_the_ones_the_tests_use():
    rec = json.load(open(os.path.join(ROOT, "profiles", "r07_winding_tolerances.json")))
    assert rec["beta"] == W.BETA and rec["E0"] == W.E0 and rec["E"] == W.E_FAST
    assert rec["exact_path_max_abs_diff_vs_fp64"] == W.EXACT_MEASURED and rec["exact_path_bound"] == W.EXACT_TOL
    assert {int(k): v for k, v in rec["L_of_F"].items()} == {F: T.levels(F) for F in (8, 48, 224, 528, 2208, 4056, 4224, 100000)}


@pytest.mark.parametrize("name", W.OPEN)
def test_open_sphere_band_is_a_small_share(name):
    w = W.exact64(name)
    share = float((np.abs(w - 0.5) < W.BAND).mean())
    print("%s: %.2f %% within %.2f of 0.5 (%.2f %% within 0.05)" % (name, 100 * share, W.BAND, 100 * float((np.abs(w - 0.5) < 0.05).mean())))
    assert share <= 0.05


@pytest.mark.parametrize("name", W.WATERTIGHT)
def test_watertight_set_aside_is_a_small_share_and_parity_holds_elsewhere(name):
    v, f, p = W.case(name)
    aside = R.set_aside(v, f, p)
    print("%s: %.3f %% set aside" % (name, 100 * float(aside.mean())))
    assert float(aside.mean()) <= 0.005
    w = W.exact64(name)
    assert float(np.abs(w - np.round(w)).max()) < 1e-6                # closed: an integer everywhere off the surface
