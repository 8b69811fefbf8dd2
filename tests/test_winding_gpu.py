"""The generalised winding number on the GPU (winding_number.hip) against the fp64 sum of tests/check_sign_ref.py, on the shared
inputs of tests/winding_cases.py.  The bounds are the recorded ones (profiles/r07_winding_tolerances.json):
the exact path within EXACT_TOL = min(4 x its measured difference, 1e-3), the fast path within E_FAST = 2 E0 <= 0.05, E0 the
error of the fp64 restatement of the tree (tests/winding_ref.py, checked in test_winding_ref_cpu.py).  Every comparison prints its
figure before it asserts.

Measured on an MI355X — exact path: 0 / 3.14e-6 / 3.51e-6 / 1.19e-6 at F = 0 / 1 / 12 / 224 (EXACT_TOL = 1.40e-5); fast path:
sphere8 2.3e-3, sphere24 9.0e-3, torus24x12 1.26e-2, shell8 1.64e-2 (the point that sets E0), mixed8 1.9e-3, open8 2.2e-3, flipped8
2.7e-3, spheres of 8 / 48 / 528 / 4,224 faces 2.3e-6 / 4.6e-4 / 1.19e-2 / 1.27e-2, cone 4.8e-4, far field 3.8e-3 of its scale,
mid size 9.7e-3 against the exact path (E = 3.27e-2)."""
import numpy as np
import pytest
import torch

from tests import check_sign_ref as R
from tests import winding_cases as W
from tests import winding_ref as T

pytestmark = pytest.mark.gpu


def _t(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _wn(cuda, v, f, p, **kw):
    from deftet_amd import hip_ops
    v, p = np.asarray(v), np.asarray(p)
    if v.ndim == 2:
        v, p = v[None], p[None]
    return hip_ops.winding_number(_t(v, cuda), _t(f, cuda), _t(p, cuda), **kw)


def _shapes(v, B):
    """B shapes from one vertex array: shape b scaled by 1 - 0.1 b and shifted"""
    return np.stack([(v.astype(np.float64) * (1.0 - 0.1 * b) + 0.02 * b).astype(np.float32) for b in range(B)])


TRIANGLE = (np.float32([[0.1, 0.0, 0.05], [0.5, 0.1, 0.0], [0.2, 0.6, 0.3]]), np.int64([[0, 1, 2]]))


def _edge_mesh(F):
    if F == 0:
        return R.cube()[0], np.zeros((0, 3), np.int64)
    if F == 1:
        return TRIANGLE
    if F == 12:
        v, f = R.cube()
        return R.rotate(v, 21), f
    v, f, _ = W.case("sphere8")
    assert f.shape[0] == F
    return v, f


# ------------------------------------------------------------------------------------------ exact path
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", [0, 1, 12, 224])
def test_exact_against_fp64_at_wave_edges(cuda, F, B):
    """N in {1, 63, 64, 65, 4000}: the first N of the same 4,000 points, so that one fp64 reference serves all five and a point's
    value can be compared across them bit for bit"""
    v, f = _edge_mesh(F)
    vb = _shapes(v, B)
    fp = f if F else R.cube()[1]                                      # (points need a surface to be placed at)
    pts = np.stack([R.points_for(vb[b], fp, 3000, 1000, 40 + b) for b in range(B)])
    want = np.stack([R.winding_number(vb[b], f, pts[b]) for b in range(B)])
    full, worst = None, 0.0
    for N in (4000, 65, 64, 63, 1):
        got = _wn(cuda, vb, f, pts[:, :N], algo="exact").cpu().numpy()
        assert got.shape == (B, N) and got.dtype == np.float32
        worst = max(worst, float(np.abs(got - want[:, :N]).max()))
        if full is None:
            full = got
        assert np.array_equal(got, full[:, :N])
    print("exact F=%d B=%d: max |gpu - fp64| = %.3e (bound %.3e)" % (F, B, worst, W.EXACT_TOL))
    assert worst <= W.EXACT_TOL
    if F == 0:
        assert not full.any()


# ------------------------------------------------------------------------------------------ fast path
@pytest.mark.parametrize("name", W.FAST_CASES)
def test_fast_against_fp64_within_E(cuda, name):
    """uniform points and points at NEAR_OFFSET from the surface; the spheres of 8 / 48 / 224 / 528 / 2,208 / 4,224 faces take the tree
    depths 0-5; mixed8 has 12 cube faces whose leaf radius forces opening and values up to 2; flipped8 gives -1 inside.  The sorted
    and the unsorted walk put a point into different waves: same bits."""
    from deftet_amd import _lib
    v, f, p = W.case(name)
    want = W.exact64(name)
    assert _lib.load().deftet_winding_number_levels(f.shape[0]) == T.levels(f.shape[0])
    got = _wn(cuda, v, f, p, algo="fast")[0].cpu().numpy()
    err = float(np.abs(got - want).max())
    print("fast %s F=%d L=%d: max |gpu - fp64| = %.3e (E = %.3e)" % (name, f.shape[0], T.levels(f.shape[0]), err, W.E_FAST))
    assert W.E_FAST <= W.E_FAST_CAP and err <= W.E_FAST
    assert np.array_equal(got, _wn(cuda, v, f, p, algo="fast_unsorted")[0].cpu().numpy())
    if name == "mixed8":
        assert round(float(want.max())) == 2 and abs(float(got.max()) - 2.0) <= W.E_FAST
    if name == "flipped8":
        assert round(float(want.min())) == -1 and abs(float(got.min()) + 1.0) <= W.E_FAST


def test_fast_with_all_faces_in_one_leaf(cuda):
    v, f = W.cone()
    tree = T.build(v, f)
    assert tree["L"] == 1 and list(tree["seg"]) == [0] * 8 + [24]
    p = R.points_for(v, f, 2000, 500, 5)
    got = _wn(cuda, v, f, p, algo="fast")[0].cpu().numpy()
    err = float(np.abs(got - R.winding_number(v, f, p)).max())
    print("fast cone: max |gpu - fp64| = %.3e" % err)
    assert err <= W.E_FAST


def test_fast_far_outside_the_box_takes_the_root_as_one_dipole(cuda):
    """20 to 100 box diagonals away every point is farther than beta radii from the root (radius <= one diagonal), so its value is
    the root's dipole alone.  Bound: the first-order expansion about the centre leaves at most ~3 (r / d) of the scale A / (4 pi d^2)
    of the value; r / d <= 1 / 20 here, hence 0.15 of that scale (fp32 adds 1e-6 of it)."""
    v, f, _ = W.case("open8")
    rng = np.random.default_rng(3)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    p = (d * diag * rng.uniform(20.0, 100.0, size=(500, 1))).astype(np.float32)
    want = R.winding_number(v, f, p)
    tree = T.build(v, f)
    _w, n_node, n_face = T.fast(tree, p, W.BETA)
    assert n_node.max() == 1 and n_face.max() == 0
    _N, _R, C, A = tree["levels"][0]
    scale = A[0] / (4.0 * np.pi * ((p.astype(np.float64) - C[0][None]) ** 2).sum(1))
    got = _wn(cuda, v, f, p, algo="fast")[0].cpu().numpy()
    rel = float((np.abs(got - want) / scale).max())
    print("fast far field: max |gpu - fp64| / (A / 4 pi d^2) = %.3e" % rel)
    assert rel <= 0.15 and float(np.abs(got - want).max()) <= W.E_FAST


def test_mid_size_fast_against_exact_on_the_gpu(cuda):
    """the centroids of the res 20 grid (6,000 tets), two jittered shapes, against uv_sphere(32) (3,968 faces)"""
    from deftet_amd import grids
    verts, tets = grids.kuhn_grid(20)
    pos = grids.jittered_positions(verts, 20, 2, 0.1)
    cen = grids.gather_tets(pos, tets).mean(2).astype(np.float32)
    assert cen.shape == (2, 6000, 3)
    v, f = R.uv_sphere(32)
    vb = np.stack([R.rotate(v, 31), R.rotate(v * 0.8, 32)])
    fast, exact = _wn(cuda, vb, f, cen, algo="fast"), _wn(cuda, vb, f, cen, algo="exact")
    err = float((fast - exact).abs().max())
    print("mid size: max |fast - exact| = %.3e" % err)
    assert f.shape[0] == 3968 and err <= W.E_FAST
    assert int(((exact - exact.round()).abs() < 0.01).sum()) > 0.9 * exact.numel()      # (a closed mesh: integers but next to the surface)


# ------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("algo", ["exact", "fast", "fast_unsorted"])
def test_value_does_not_depend_on_wave_neighbours_or_the_run(cuda, algo):
    v, f, p = W.case("torus24x12")
    a = _wn(cuda, v, f, p, algo=algo)[0]
    assert torch.equal(a, _wn(cuda, v, f, p, algo=algo)[0])
    perm = np.random.default_rng(9).permutation(p.shape[0])
    b = _wn(cuda, v, f, p[perm], algo=algo)[0]
    assert torch.equal(a[_t(perm, cuda)], b)
    assert torch.equal(a[:777], _wn(cuda, v, f, p[:777], algo=algo)[0])


@pytest.mark.parametrize("algo", ["exact", "fast"])
def test_ragged_equals_the_single_calls_bit_for_bit(cuda, algo):
    from deftet_amd import hip_ops
    names = ("sphere24", None, "open8")                              # 2,208 faces (L = 4), no face at all, 160 faces (L = 2)
    meshes = [W.case(n)[:2] if n else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)) for n in names]
    pts = np.stack([W.case("sphere24")[2][:2500], W.case("sphere8")[2][:2500], W.case("open8")[2][:2500]])
    got = hip_ops.winding_number_ragged([_t(v, cuda) for v, _ in meshes], [_t(f, cuda) for _, f in meshes], _t(pts, cuda), algo=algo)
    assert got.shape == (3, 2500)
    for b, (v, f) in enumerate(meshes):
        assert torch.equal(got[b], _wn(cuda, v, f, pts[b], algo=algo)[0]), b
    assert not got[1].any()


# ------------------------------------------------------------------------------------------ classification
@pytest.mark.parametrize("name", W.WATERTIGHT)
def test_parity_rule_equals_check_sign_on_watertight_meshes(cuda, name):
    from deftet_amd import hip_ops
    v, f, p = W.case(name)
    keep = ~R.set_aside(v, f, p)
    assert keep.mean() >= 0.995
    for algo in ("exact", "fast"):
        inside = hip_ops.winding_inside(_wn(cuda, v, f, p, algo=algo), "parity")[0].cpu().numpy()
        ray = hip_ops.check_sign(_t(v[None], cuda), _t(f, cuda), _t(p[None], cuda))[0].cpu().numpy()
        assert np.array_equal(inside[keep], ray[keep]), algo


@pytest.mark.parametrize("name", W.OPEN)
def test_positive_rule_on_the_open_sphere(cuda, name):
    from deftet_amd import hip_ops
    v, f, p = W.case(name)
    w64 = W.exact64(name)
    keep = np.abs(w64 - 0.5) >= W.BAND
    assert keep.mean() >= 0.95
    for algo in ("exact", "fast"):
        inside = hip_ops.winding_inside(_wn(cuda, v, f, p, algo=algo), "positive")[0].cpu().numpy()
        assert np.array_equal(inside[keep], (w64 > 0.5)[keep]), algo


def test_the_two_rules_differ_inside_the_inner_sphere_of_mixed(cuda):
    """w = 2 inside the sphere (inside both surfaces), 1 between sphere and cube, 0 outside: "positive" calls the first two inside,
    "parity" only the second"""
    from deftet_amd import hip_ops
    v, f, p = W.case("mixed8")
    w64 = W.exact64("mixed8")
    settled = np.abs(w64 - np.round(w64)) < 0.01
    two, one, zero = (settled & (np.round(w64) == k) for k in (2, 1, 0))
    assert two.sum() > 50 and one.sum() > 500 and zero.sum() > 200
    w = _wn(cuda, v, f, p)
    pos, par = (hip_ops.winding_inside(w, r)[0].cpu().numpy() for r in ("positive", "parity"))
    assert pos[two].all() and not par[two].any()
    assert pos[one].all() and par[one].all()
    assert not pos[zero].any() and not par[zero].any()
    with pytest.raises(ValueError):
        hip_ops.winding_inside(w, "majority")


# ------------------------------------------------------------------------------------------ callers
def _tet_batch(cuda, B):
    from deftet_amd import grids
    verts, tets = grids.kuhn_grid(12)
    pos = grids.jittered_positions(verts, 12, B, 0.1)
    return _t(grids.gather_tets(pos, tets).astype(np.float32), cuda)


@pytest.mark.parametrize("ragged", [False, True])
def test_check_tet_inside_sdfs_by_winding_number(cuda, ragged):
    from deftet_amd.layers.DefTet.deftet import DefTet
    tet = _tet_batch(cuda, 2)
    v, f, _ = W.case("sphere8")
    v2, f2, _ = W.case("torus24x12")
    if ragged:
        mesh = [[_t(v, cuda), _t(v2, cuda)], [[_t(f, cuda)], [_t(f2, cuda)]]]
        per_shape = [(v, f), (v2, f2)]
    else:
        ft, vb = _t(f, cuda), _shapes(v, 2)
        mesh = [[_t(vb[0], cuda), _t(vb[1], cuda)], [ft[None], ft[None]]]
        per_shape = [(vb[0], f), (vb[1], f)]
    net = DefTet()
    base, parity, wind = net.check_tet_inside_sdfs(tet, mesh), net.check_tet_inside_sdfs(tet, mesh, method="parity"), \
        net.check_tet_inside_sdfs(tet, mesh, method="winding")
    assert torch.equal(base, parity) and wind.shape == base.shape and wind.dtype == base.dtype
    cen = tet.mean(2).cpu().numpy()
    for b, (vv, ff) in enumerate(per_shape):
        keep = ~R.set_aside(vv, ff, cen[b])
        assert np.array_equal(wind[b, :, 0].cpu().numpy()[keep], parity[b, :, 0].cpu().numpy()[keep]), b
    assert 0 < float(wind.sum()) < wind.numel()
    with pytest.raises(ValueError):
        net.check_tet_inside_sdfs(tet, mesh, method="rays")


def test_mesh_to_sdf_sign_by_winding_number(cuda):
    from deftet_amd import dataprep
    v, f, p = W.case("shell8")
    vt, ft, pt = _t(v[None], cuda), _t(f, cuda), _t(p[None], cuda)
    base, parity, wind = dataprep.mesh_to_sdf(vt, ft, pt), dataprep.mesh_to_sdf(vt, ft, pt, sign="parity"), \
        dataprep.mesh_to_sdf(vt, ft, pt, sign="winding")
    assert torch.equal(base, parity)
    keep = _t(~R.set_aside(v, f, p), cuda)
    assert torch.equal(wind[0][keep], parity[0][keep])
    assert bool((wind > 0).any()) and bool((wind < 0).any())
    with pytest.raises(ValueError):
        dataprep.mesh_to_sdf(vt, ft, pt, sign="rays")


def test_surface_metrics_iou_by_winding_number(cuda):
    from deftet_amd import metrics
    v, f, p = W.case("sphere8")
    vt, ft, pt = _t(v, cuda), _t(f, cuda), _t(p[None], cuda)
    fv = vt[ft][None].contiguous()
    nf = torch.tensor([f.shape[0]], dtype=torch.int32, device=cuda)
    surf = _t(R.near_surface_points(v, f, 512, 3)[None], cuda)
    occ = _t(W.exact64("sphere8")[None] > 0.5, cuda).float()
    u = torch.rand(1, 512, 3, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    kw = dict(uniforms=u, pred_verts=[vt], pred_faces_idx=[ft], sdf_points=pt, gt_occ=occ)
    a = metrics.surface_metrics(fv, nf, fv, nf, surf, **kw)
    b = metrics.surface_metrics(fv, nf, fv, nf, surf, inside_test="parity", **kw)
    c = metrics.surface_metrics(fv, nf, fv, nf, surf, inside_test="winding", **kw)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert float(c["iou"][0]) >= 0.995 and all(torch.equal(a[k], c[k]) for k in a if k != "iou")


# ------------------------------------------------------------------------------------------ bad input
@pytest.mark.parametrize("algo", ["exact", "fast"])
def test_bad_input_raises_or_gives_nan(cuda, algo):
    from deftet_amd import hip_ops
    v, f, p = W.case("sphere8")
    vb, pb = _t(_shapes(v, 2), cuda), _t(np.stack([p[:300], p[300:600]]), cuda)
    good = hip_ops.winding_number(vb, _t(f, cuda), pb, algo=algo)
    bad_f = f.copy()
    bad_f[17, 1] = v.shape[0]                                         # one past the last vertex
    with pytest.raises(IndexError):
        hip_ops.winding_number(vb, _t(bad_f, cuda), pb, algo=algo)
    assert bool(torch.isnan(hip_ops.winding_number(vb, _t(bad_f, cuda), pb, algo=algo, check=False)).all())
    nan_p = pb.clone()
    nan_p[1, 5, 2] = float("nan")
    nan_p[0, 70, 0] = float("inf")
    with pytest.raises(ValueError):
        hip_ops.winding_number(vb, _t(f, cuda), nan_p, algo=algo)
    w = hip_ops.winding_number(vb, _t(f, cuda), nan_p, algo=algo, check=False)
    hit = torch.zeros_like(w, dtype=torch.bool)
    hit[1, 5] = hit[0, 70] = True
    assert bool(torch.isnan(w[hit]).all()) and torch.equal(w[~hit], good[~hit])
    nan_v = vb.clone()
    nan_v[1, int(f[3, 0]), 1] = float("nan")                         # a corner of a face of shape 1 only
    with pytest.raises(ValueError):
        hip_ops.winding_number(nan_v, _t(f, cuda), pb, algo=algo)
    w = hip_ops.winding_number(nan_v, _t(f, cuda), pb, algo=algo, check=False)
    assert bool(torch.isnan(w[1]).all()) and torch.equal(w[0], good[0])
