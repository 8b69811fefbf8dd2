"""The point-to-triangle backward (operator A9, hip_ops.tri_dist_bwd) against fp64 and at its wave edges.  Every case runs the
three device paths: the deterministic sorted path, the per-point atomic path, and the grouped path (order=) with the forward's
own point order, the identity and a seeded random permutation.

pin         every path, and tet_analytic_distance_f_batch(...).backward(), equals the fp64 envelope gradient
            (tests/tri_dist_ref.py) where the operator is the true gradient: points of the face and the vertex class.  The bound
            is 4 x the error the CPU oracle itself has against fp64 on the same input (the 4 covers the summation order of the
            atomic paths over at most 22 terms per face).
edges       P in {1, 63, 64, 65, 255, 256, 257, 64 * 256 + 77} x {one face for all points, a face of its own per point, a
            random face with skipped entries}: the ragged last wave, 1 to 64 ballot rounds per wave, more than one block.
            Deterministic == oracle bit for bit; the order-dependent paths bit for bit where nothing is summed, else within
            n_f * 2^-24 * sum |term| of the fp64 sum of the per-point terms.
ragged      a shape without faces and a shape with half of them in one batch.
non-finite  +-inf and NaN in the incoming gradient: the same non-finite entries as the oracle in every path, including the
            inf * 0 the reference adds to the far endpoint of an edge, which the grouped path's `v != 0` must not lose.
front end   strided and float64 inputs and a side stream through tet_analytic_distance_f_batch.

Measured on an MI355X, max-norm error against the fp64 gradient on the pin (208 faces, 1653 clear face-class and 205 clear
vertex-class points, at most 20 per face, scale 0.22): CPU oracle 8.02e-07, hence the bound 3.21e-06; deterministic 8.02e-07
(bit-equal to the oracle), atomic 8.02e-07, grouped 7.85e-07 with each of the three orders, through autograd 7.85e-07 to
8.02e-07 (it runs the grouped path, whose atomics land in a different order from run to run).
"""
import numpy as np
import pytest
import torch

from tests import tri_dist_cases as C
from tests import tri_dist_ref as R
from tests.tol import check_close

pytestmark = pytest.mark.gpu

PATHS = ["deterministic", "atomic", "order=forward", "order=identity", "order=random"]
ORDER_DEPENDENT = PATHS[1:]


def _t(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _assert_permutation(order, B, P):
    assert order is not None and order.dtype == torch.int32 and order.shape == (B, P)
    assert torch.equal(order.long().sort(1).values, torch.arange(P, device=order.device).expand(B, -1))


def _run_paths(cuda, pts, face, cf, g, fwd_order, seed=5):
    """name -> [B,F,3,3] numpy, for the five device paths"""
    from deftet_amd import hip_ops
    B, P = pts.shape[:2]
    ident = torch.arange(P, device=cuda, dtype=torch.int32).expand(B, -1).contiguous()
    gen = torch.Generator().manual_seed(seed)
    rand = torch.stack([torch.randperm(P, generator=gen) for _ in range(B)]).to(torch.int32).to(cuda)
    for o in (fwd_order, ident, rand):
        _assert_permutation(o, B, P)                                 # the grouped kernel trusts its order
    out = {"deterministic": hip_ops.tri_dist_bwd(pts, face, cf, g, deterministic=True),
           "atomic": hip_ops.tri_dist_bwd(pts, face, cf, g),
           "order=forward": hip_ops.tri_dist_bwd(pts, face, cf, g, order=fwd_order),
           "order=identity": hip_ops.tri_dist_bwd(pts, face, cf, g, order=ident),
           "order=random": hip_ops.tri_dist_bwd(pts, face, cf, g, order=rand)}
    assert list(out) == PATHS
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- a. fp64 pin ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pin(cuda, oracle):
    from deftet_amd import hip_ops
    tri, pts, rng = C.pin_surface_and_points(oracle)
    d = {"tri": tri, "pts": pts, "t_tri": _t(tri[None], cuda), "t_pts": _t(pts[None], cuda),
         "t_nfb": torch.tensor([float(tri.shape[0])], device=cuda)}
    _, f, order = hip_ops.tri_dist_fwd(d["t_pts"], d["t_tri"], d["t_nfb"], want_order=True)
    d["t_cf"], d["t_order"], d["cf"] = f, order, f.cpu().numpy()
    d["g"], d["cls"], d["clear"] = C.pin_gradient(tri, pts, d["cf"], rng)
    d["stats"] = C.check_pin_conditions(tri, d["cf"], d["cls"], d["clear"])
    return d


def test_pin_every_path_equals_the_fp64_envelope_gradient(cuda, oracle, pin):
    from deftet_amd.layers.DefTet.tet_analytic_distance_batch.utils import tet_analytic_distance_f_batch
    tri, pts, g = pin["tri"], pin["pts"], pin["g"]
    want = R.envelope_gradient(pts, tri, pin["cf"], g)
    ora = oracle.tri_dist_bwd(pts[None], tri[None], pin["cf"], g.reshape(1, -1, 1))[0]
    oracle_err = C.maxnorm(ora, want)
    bound = 4 * oracle_err
    print("A9 bwd pin: %s, scale %.3g, oracle max-norm error %.3g" % (pin["stats"], np.abs(want).max(), oracle_err))
    assert 0 < oracle_err < 1e-4                                     # the CPU half holds it to its derived bound
    t_g = _t(g.reshape(1, -1, 1), cuda)
    got = _run_paths(cuda, pin["t_pts"], pin["t_tri"], pin["t_cf"], t_g, pin["t_order"])
    assert np.array_equal(got["deterministic"][0], ora)
    fr = pin["t_tri"].clone().requires_grad_(True)
    dd, ff = tet_analytic_distance_f_batch(pin["t_pts"], fr, pin["t_nfb"])
    assert torch.equal(ff, pin["t_cf"])
    (dd * t_g).sum().backward()
    got["autograd"] = fr.grad.cpu().numpy()
    errs = {k: C.maxnorm(v[0], want) for k, v in got.items()}
    print("A9 bwd pin: device max-norm errors %s, bound %.3g" % ({k: "%.3g" % e for k, e in errs.items()}, bound))
    for k, v in got.items():
        check_close("A9 bwd fp64 pin, %s" % k, v[0], want, bound)


# ---- b. wave and block edges ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", C.EDGE_P)
@pytest.mark.parametrize("pattern", C.EDGE_PATTERNS)
def test_wave_and_block_edges(cuda, oracle, pattern, P):
    from deftet_amd import hip_ops
    pts, face, cf, g = C.edge_case(pattern, P)
    F = face.shape[1]
    assert pts.shape == (1, P, 3) and F == {"one_face": 1, "distinct": P, "mixed": max(1, P // 7)}[pattern]
    ora = oracle.tri_dist_bwd(pts, face, cf, g)
    assert np.isfinite(ora).all() and (P < 63 or (ora != 0).any())
    t_pts, t_face, t_cf, t_g = (_t(x, cuda) for x in (pts, face, cf, g))
    _, _, fwd_order = hip_ops.tri_dist_fwd(t_pts, t_face, torch.tensor([float(F)], device=cuda), want_order=True)
    got = _run_paths(cuda, t_pts, t_face, t_cf, t_g, fwd_order, seed=P)
    assert np.array_equal(got["deterministic"], ora)
    if pattern == "distinct":                                        # one contribution per row: nothing is summed
        assert np.array_equal(np.sort(cf.reshape(-1)), np.arange(P))
        for k in ORDER_DEPENDENT:
            assert np.array_equal(got[k], ora), k
        return
    terms = C.per_point_terms(oracle, pts, face, cf, g)
    want, bound = C.order_bound(terms, cf, F)
    assert (np.abs(ora[0] - want) <= bound).all()                    # the serial order is one of the orders
    for k in ORDER_DEPENDENT:
        err = np.abs(got[k][0] - want)
        assert (err <= bound).all(), (k, float((err - bound).max()), int((err > bound).sum()))
    if pattern == "mixed" and P >= 63:
        c = cf.reshape(-1)
        assert (c == -1).any() and (c == F).any() and ((c >= 0) & (c < F)).any()


# ---- c. ragged batch --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged(cuda, oracle):
    from deftet_amd import hip_ops
    from tests.test_surface_ops_gpu import _sphere_surfaces
    radii = [0.3, 0.3, 0.3]                                          # one radius, three jitters of the grid
    v, faces = _sphere_surfaces(cuda, oracle, radii)
    F = min(int(f.shape[0]) for f in faces)
    face = torch.stack([v[b][faces[b][:F]] for b in range(3)]).contiguous()
    nfb = torch.tensor([float(F), 0.0, float(F // 2)], device=cuda)
    rng = np.random.default_rng(21)
    d3 = rng.standard_normal((3, 4000, 3))
    pts = _t((d3 / np.linalg.norm(d3, axis=2, keepdims=True) * np.array(radii)[:, None, None]).astype(np.float32), cuda)
    g = _t(rng.standard_normal((3, 4000, 1)).astype(np.float32), cuda)
    _, cf, order = hip_ops.tri_dist_fwd(pts, face, nfb, want_order=True)
    return {"F": F, "face": face, "nfb": nfb, "pts": pts, "g": g, "cf": cf, "order": order}


def test_ragged_batch_with_an_empty_shape(cuda, oracle, ragged):
    F, cf = ragged["F"], ragged["cf"]
    assert F >= 200
    assert (cf[0] >= 0).all() and (cf[1] == -1).all() and (cf[2] >= 0).all() and (cf[2] < F // 2).all()
    ora = oracle.tri_dist_bwd(ragged["pts"].cpu().numpy(), ragged["face"].cpu().numpy(), cf.cpu().numpy(), ragged["g"].cpu().numpy())
    assert (ora[0] != 0).any() and (ora[2, : F // 2] != 0).any()
    got = _run_paths(cuda, ragged["pts"], ragged["face"], cf, ragged["g"], ragged["order"])
    assert np.array_equal(got["deterministic"], ora)
    for k, v in got.items():
        assert not v[1].any(), k                                     # no faces: exactly zero
        assert not v[2, F // 2:].any(), k                            # beyond the shape's faces: exactly zero
        check_close("A9 bwd ragged batch, %s" % k, v, ora, 2e-5)


# ---- d. non-finite incoming gradient ----------------------------------------------------------------------------------------

def test_non_finite_incoming_gradient(cuda, oracle, pin):
    tri, pts, cls, clear = pin["tri"], pin["pts"], pin["cls"], pin["clear"]
    cf = pin["cf"].reshape(-1).astype(np.int64)
    g, idx, shared, edge_faces = C.non_finite_gradient(tri, pts, cf, cls, clear, pin["g"])
    g_finite = g.copy()
    g_finite[idx] = 0
    want = R.envelope_gradient(pts, tri, cf, g_finite)               # right wherever no non-finite point reaches
    ora = oracle.tri_dist_bwd(pts[None], tri[None], pin["cf"], g.reshape(1, -1, 1))[0]
    finite = np.isfinite(ora)
    assert np.isnan(ora[shared]).all()
    for f in edge_faces:                                             # t * inf on the first endpoint, 0 * inf on the far one
        assert (~finite[f]).sum() >= 6 and np.isnan(ora[f]).sum() >= 3
    touched = np.zeros(tri.shape[0], bool)
    touched[cf[idx]] = True
    assert finite[~touched].all() and not finite[touched].all()
    bound = 4 * C.maxnorm(ora[finite], want[finite])
    got = _run_paths(cuda, pin["t_pts"], pin["t_tri"], pin["t_cf"], _t(g.reshape(1, -1, 1), cuda), pin["t_order"])
    assert np.array_equal(got["deterministic"][0], ora, equal_nan=True)
    for k, v in got.items():
        assert np.array_equal(np.isfinite(v[0]), finite), k
        assert np.array_equal(v[0][~finite], ora[~finite], equal_nan=True), k     # NaN, +inf or -inf: the same kind
        check_close("A9 bwd non-finite gradient, finite entries, %s" % k, v[0], want, bound, mask=finite)


# ---- e. front end -----------------------------------------------------------------------------------------------------------

def test_front_end_strides_dtypes_and_streams(cuda, ragged, monkeypatch):
    from deftet_amd.layers.DefTet.tet_analytic_distance_batch.utils import tet_analytic_distance_f_batch
    monkeypatch.setenv("DEFTET_HIP_DETERMINISTIC", "1")
    pts, face, nfb, g = ragged["pts"], ragged["face"], ragged["nfb"], ragged["g"]

    def run(p, f, n):
        p, f, n = p.requires_grad_(True), f.requires_grad_(True), n.requires_grad_(True)
        d, cf = tet_analytic_distance_f_batch(p, f, n)
        (d * g).sum().backward()
        assert p.grad is None and n.grad is None                     # the gradient goes to the faces only
        assert d.dtype == torch.float32 and torch.equal(cf, ragged["cf"])
        return f.grad

    base = run(pts.clone(), face.clone(), nfb.clone())
    assert base.dtype == torch.float32 and base.abs().max() > 0
    assert torch.equal(base, run(pts.clone(), face.clone(), nfb.clone()))
    # strided views on a side stream
    sp = pts.transpose(1, 2).contiguous().transpose(1, 2)
    sf = face.transpose(1, 2).contiguous().transpose(1, 2)
    assert not sp.is_contiguous() and not sf.is_contiguous() and torch.equal(sp, pts) and torch.equal(sf, face)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        strided = run(sp, sf, nfb.clone())
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(strided, base)
    # float64 in, float64 gradient out, the same values
    wide = run(pts.double(), face.double(), nfb.double())
    assert wide.dtype == torch.float64 and torch.equal(wide.float(), base) and torch.equal(wide, base.double())
