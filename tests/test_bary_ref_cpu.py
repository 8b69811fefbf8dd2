"""tests/bary_ref.py and tests/bary_cases.py kept honest, and the CPU half of the fp64 pin of the point-in-tet weights and backward
(tests/test_bary_backward_gpu.py is the GPU half):

* the analytic fp64 reference (w, dL/dtet, dL/dp) is what fp64 torch autograd of the reference's barycentric formula
  (oracle.bary_torch) gives, to 1e-10 per tet, on every band;
* the tets are disjoint and every query lies in the tet it was made in: the CPU oracle answers own[q] for every query of an
  asserted tet and -1 for every query placed in a cell's empty margin;
* in every band at least 90 % of the tets that receive a hit are asserted (kappa <= 5e4) - a condition on the inputs;
* the fp32 restatement of the kernels' arithmetic stays within the bounds taken with K / 4 in place of K.  That is where K = 2
  comes from: the GPU is held to bounds four times as wide as what its own operation order needs on these inputs.
"""
import numpy as np
import pytest
import torch

from tests import bary_cases as C
from tests import bary_ref as R

KINDS = ["records", "records, second of a pair", "overflow", "lists"]      # every shape the GPU tests run on a band


@pytest.fixture(scope="module")
def shapes():
    out = {}
    for b in C.BANDS:
        pair = C.pair_batch(b)
        out[(b, "records")], out[(b, "records, second of a pair")] = C.records_shape(b), pair[1]
        out[(b, "overflow")], out[(b, "lists")] = C.overflow_shape(b), C.lists_shape(b)
        assert np.array_equal(pair[0]["tet"], out[(b, "records")]["tet"]) and pair[0]["pts"].shape == pair[1]["pts"].shape
    return out


def _ratio(err, bound):
    return float((err / bound).max())


def test_share_of_asserted_tets_per_band(shapes):
    for key, s in shapes.items():
        share = C.asserted_share(s)
        print("asserted share %s: %.3f (kappa median %.3g, max %.3g)" % (key, share, np.median(s["kappa"]), s["kappa"].max()))
        assert share >= C.MIN_ASSERTED_SHARE, (key, share)
        assert (s["counts"][s["asserted"]] > 0).sum() >= 100          # and they are many
    # the three things a case builds on: fp32 tets inside their cells (lattice() asserts it), own in range, about 10 % misses
    for b in C.BANDS:
        s = shapes[(b, "overflow")]
        assert s["tet"].dtype == np.float32 and s["pts"].dtype == np.float32 and s["tet"].shape == (512, 4, 3)
        assert 0.05 < (s["own"] < 0).mean() < 0.15
        assert np.array_equal(np.bincount(s["own"][s["own"] >= 0], minlength=512), s["counts"])
        assert (s["counts"] == 40).sum() == 2 and (s["counts"] == 9).sum() >= 8 and s["counts"].max() == 40
        assert s["asserted"][s["counts"] >= 9].all()                 # the long sums are on asserted tets
        for kind in KINDS:                                           # which backward a shape reaches (hip_ops.bwd_uses_records)
            assert (shapes[(b, kind)]["pts"].shape[0] <= 2 * 512) == (kind != "lists"), (b, kind)


def test_kappa_is_what_it_says():
    # the regular corner tet with unit legs: L = sqrt 2, 6V = 1; moved away by 100 the coordinates cost another 101 / sqrt 2
    t = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float64)
    assert np.allclose(C.kappa(t), 2 ** 1.5)
    assert np.allclose(C.kappa(t + 100.0), 2 ** 1.5 * 101 / 2 ** 0.5)
    assert np.allclose(C.kappa(t * 1e-3), 2 ** 1.5)                   # scale free
    flat = t.copy()
    flat[0, 3, 2] = 0.01
    assert np.allclose(C.kappa(flat), 2 ** 1.5 / 0.01)
    assert np.isinf(C.kappa(np.zeros((1, 4, 3)) + t[:, :1])[0]) or np.isnan(C.kappa(np.zeros((1, 4, 3)) + t[:, :1])[0])


@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_oracle_answers_the_tet_a_query_was_made_in(oracle, shapes, band):
    for kind in KINDS:
        s = shapes[(band, kind)]
        cond = oracle.point_in_tet(s["tet"][None], s["pts"][None]).reshape(-1).astype(np.int64)
        own = s["own"]
        check = (own < 0) | s["asserted"][np.maximum(own, 0)]
        assert np.array_equal(cond[check], own[check]), (band, kind, int((cond[check] != own[check]).sum()))
        assert (cond[own < 0] == -1).all() and (own < 0).any()


@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_analytic_reference_is_the_fp64_autograd_of_the_reference_formula(oracle, shapes, band):
    s = shapes[(band, "lists")]
    gw, go = C.incoming(s)
    ref = R.analytic(s["tet"], s["pts"], s["own"], gw, go)
    hit, t = torch.from_numpy(ref["hit"]), torch.from_numpy(ref["t"])
    tet = torch.from_numpy(s["tet"]).double().requires_grad_(True)
    pts = torch.from_numpy(s["pts"]).double().requires_grad_(True)
    sel = tet[t]
    w = torch.stack(oracle.bary_torch(sel[:, 0], sel[:, 1], sel[:, 2], sel[:, 3], pts), -1) * hit[:, None]
    (w * torch.from_numpy(gw).double()).sum().backward()
    w, gt, gp = w.detach().numpy(), tet.grad.numpy(), pts.grad.numpy()
    assert np.abs(ref["w"] - w).max() <= 1e-10
    assert (ref["w"][ref["hit"]].min() > 0.04) and np.abs(ref["w"][ref["hit"]].sum(1) - 1).max() < 1e-9      # inside, by construction
    assert not ref["w"][~ref["hit"]].any() and not ref["G"][~ref["hit"]].any() and not gp[~ref["hit"]].any()
    has = ref["n"] > 0
    scale_t = np.abs(gt).max((1, 2))
    assert (np.abs(ref["grad_tet"] - gt).max((1, 2))[has] <= 1e-10 * scale_t[has]).all()
    assert not ref["grad_tet"][~has].any() and not gt[~has].any()
    scale_q = np.zeros(s["tet"].shape[0])
    np.maximum.at(scale_q, ref["t"][ref["hit"]], np.abs(gp[ref["hit"]]).max(1))
    assert (np.abs(ref["G"] - gp).max(1) <= 1e-10 * scale_q[ref["t"]])[ref["hit"]].all()
    # grad_pred: the plain sums, the misses on tet 0
    want = np.zeros(s["tet"].shape[0])
    np.add.at(want, ref["t"], go.astype(np.float64))
    assert np.abs(ref["grad_pred"] - want).max() <= 1e-12 * np.abs(go).sum()
    assert ref["pred_n"].sum() == s["pts"].shape[0] and ref["pred_n"][0] == (ref["t"] == 0).sum() >= (~ref["hit"]).sum() > 0
    # to the vertices of the soup topology: the same numbers in other places
    idx = C.soup_topology(s["tet"].shape[0])
    gpos = R.scatter_to_vertices(ref["grad_tet"], idx, idx.size)
    assert np.array_equal(gpos[idx], ref["grad_tet"]) and not np.array_equal(idx.reshape(-1), np.arange(idx.size))
    assert np.array_equal(C.soup_positions(s["tet"], idx)[idx], s["tet"])


@pytest.mark.parametrize("band", C.BANDS, ids=C.BAND_IDS)
def test_fp32_restatement_stays_within_a_quarter_of_k(oracle, shapes, band):
    _restatement_within_a_quarter_of_k(oracle, "%s-%g" % band, [shapes[(band, kind)] for kind in KINDS])


def test_fp32_restatement_on_the_butterfly_and_mixed_shapes(oracle):
    b = C.butterfly_shape()
    assert b["counts"].max() == C.BUTTERFLY_HITS and b["asserted"][b["counts"].argmax()] and b["pts"].shape[0] <= 2 * b["tet"].shape[0]
    assert np.sort(b["counts"])[-2] <= 1 and C.asserted_share(b) >= C.MIN_ASSERTED_SHARE
    mixed = C.mixed_batch()
    assert len({s["pts"].shape[0] for s in mixed}) == 1 and [(s["band"], s["flat"]) for s in mixed] == C.MIXED_BANDS
    for s in mixed:
        assert C.asserted_share(s) >= C.MIN_ASSERTED_SHARE and s["pts"].shape[0] <= 2 * 512
    _restatement_within_a_quarter_of_k(oracle, "butterfly, mixed", [b] + mixed, min_q=100, min_t=30)


def test_fp32_restatement_on_the_jittered_grid_of_test_weights_and_backward(oracle):
    """tests/test_point_in_tet_gpu.py::test_weights_and_backward holds dL/dp and dL/dtet to the same bounds on its Kuhn grid"""
    from tests import cases
    tet, pts = cases.jittered(8, 4000, 2)
    cond = oracle.point_in_tet(tet, pts)[..., 0]
    some = []
    for b in range(2):
        k = C.kappa(tet[b])
        assert k.max() <= 100
        some.append({"tet": tet[b], "pts": pts[b], "own": cond[b].astype(np.int64), "kappa": k, "asserted": k <= C.KAPPA_CAP})
    # kappa is at most 9 there, and among 8,000 queries some have four terms that cancel: dL/dp is held to the scale of its terms
    _restatement_within_a_quarter_of_k(oracle, "jittered res 8", some, gw=np.random.default_rng(4000).standard_normal((2, 4000, 4)).astype(np.float32),
                                       terms=True)


def _restatement_within_a_quarter_of_k(oracle, name, some_shapes, min_q=300, min_t=100, gw=None, terms=False):
    worst = {"w": 0.0, "w forward": 0.0, "grad_pts": 0.0, "grad_tet": 0.0}
    given = gw
    if True:
        for b, s in enumerate(some_shapes):
            gw = given[b] if given is not None else C.incoming(s)[0]
            ref = R.analytic(s["tet"], s["pts"], s["own"], gw)
            w32, G32, gt32 = R.restatement(s["tet"], s["pts"], s["own"], gw)
            fwd = oracle.bary(s["tet"][None], s["pts"][None], s["own"].astype(np.float32)[None])[0]      # the forward's association
            q = ref["hit"] & s["asserted"][ref["t"]]
            ta = s["asserted"] & (ref["n"] > 0)
            assert q.sum() > min_q and ta.sum() > min_t
            k4 = C.K / 4
            worst["w"] = max(worst["w"], _ratio(np.abs(w32 - ref["w"]).max(1)[q], R.bound_w(ref, s["kappa"], k4)[q]))
            worst["w forward"] = max(worst["w forward"], _ratio(np.abs(fwd - ref["w"]).max(1)[q], R.bound_w(ref, s["kappa"], k4)[q]))
            worst["grad_pts"] = max(worst["grad_pts"], _ratio(np.abs(G32 - ref["G"]).max(1)[q], R.bound_G(ref, s["kappa"], k4, terms)[q]))
            worst["grad_tet"] = max(worst["grad_tet"], _ratio(np.abs(gt32 - ref["grad_tet"]).max((1, 2))[ta], R.bound_tet(ref, s["kappa"], k4)[ta]))
            assert not gt32[ref["n"] == 0].any() and not w32[~ref["hit"]].any()
    print("restatement over its K/4 bound, %s: %s" % (name, {k: "%.3f" % v for k, v in worst.items()}))
    for k, v in worst.items():
        assert v <= 1.0, (name, k, v)


def test_restatement_adds_in_ascending_query_order():
    """three hits on one tet whose fp32 sum depends on the order: the restatement's is the ascending one"""
    tet = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    pts = np.array([[0.25, 0.25, 0.25], [0.1, 0.2, 0.3], [0.3, 0.1, 0.2]], np.float32)
    gw = np.array([[1e8, 0, 0, 0], [1, 2, 3, 4], [-1e8, 0, 0, 0]], np.float32)
    cond = np.zeros(3)
    _, _, gt = R.restatement(tet, pts, cond, gw)
    term = [R.restatement(tet, pts[q: q + 1], cond[:1], gw[q: q + 1])[2][0] for q in range(3)]     # one hit: the term itself
    assert np.array_equal(gt[0], (term[0] + term[1]) + term[2])
    assert not np.array_equal(gt[0], (term[2] + term[1]) + term[0])
    assert np.array_equal(R.restatement(tet, pts[::-1], cond, gw[::-1])[2][0], (term[2] + term[1]) + term[0])
