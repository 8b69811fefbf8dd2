"""The evaluation metrics on the GPU: point-to-mesh grid == scan bit for bit (adversarial soups, full size),
== the numpy fp32 restatement, close to fp64 Ericson where tri_dist_fwd is not; sided distance; sampling against its restatement
and the areas; surface_metrics against an fp64 restatement, run to run, ragged batches; a caller through the Kaolin shim."""
import importlib
import sys

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _soup(rng, F, scale=1.0):
    tri = (rng.normal(size=(F, 3, 3)) * 0.05 + rng.uniform(-1, 1, size=(F, 1, 3))) * scale
    k = F // 10
    tri[:k, 2] = tri[:k, 0] + 0.5 * (tri[:k, 1] - tri[:k, 0])                   # collinear
    tri[k:2 * k, :, 2] = tri[k:2 * k, :1, 2] + 1e-6 * rng.normal(size=(k, 3))    # near-flat in z
    tri[2 * k:3 * k, :, 0] = tri[2 * k:3 * k, :1, 0]                             # vertical (x constant)
    tri[3 * k:4 * k] = tri[3 * k:4 * k, :1] + 1e-7 * rng.normal(size=(k, 3, 3))  # tiny
    tri[4 * k:5 * k] = tri[5 * k:6 * k]                                          # duplicates: ties
    tri[6 * k, 0, 0] = np.nan
    tri[6 * k + 1, 1, 2] = np.inf
    tri[6 * k + 2] = tri[6 * k + 2, :1]                                          # a point
    tri[6 * k + 3, 2] = 50.0                                                     # one huge face
    return tri.astype(np.float32)


def _points(rng, P, scale=1.0):
    p = rng.uniform(-1.2, 1.2, size=(P, 3)) * scale
    p[:4] = [[40, 0, 0], [-30, 25, 3], [0, 0, 1e4], [np.nan, 0, 0]]              # far and non-finite points
    return p.astype(np.float32)


def _pm(p, f, n=None, brute=False):
    from deftet_amd import metrics
    return metrics.point_to_mesh_distance(p, f, n, brute=brute)


def _equal3(a, b):
    for x, y in zip(a, b):
        assert torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0))
        assert torch.equal(torch.isnan(x.float()), torch.isnan(y.float()))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_grid_equals_scan_on_adversarial_soups(cuda, seed):
    rng = np.random.default_rng(seed)
    F, P = 3000, 5000
    f = np.stack([_soup(rng, F), _soup(rng, F, 3.0)])
    p = np.stack([_points(rng, P), _points(rng, P, 3.0)])
    ft, pt = _t(f, cuda), _t(p, cuda)
    nf = torch.tensor([F, F - 700], dtype=torch.int32, device=cuda)
    g, s = _pm(pt, ft, nf), _pm(pt, ft, nf, brute=True)
    _equal3(g, s)
    assert torch.isnan(g[0][:, 3]).all() and (g[1][:, 3] == -1).all()
    assert (g[1][torch.isfinite(pt).all(-1)] >= 0).all()


def test_empty_and_all_nonfinite_shapes(cuda):
    p = torch.rand(3, 50, 3, device=cuda)
    f = torch.rand(3, 4, 3, 3, device=cuda)
    f[2] = float("nan")
    nf = torch.tensor([0, 4, 4], dtype=torch.int32, device=cuda)
    for brute in (False, True):
        d, i, t = _pm(p, f, nf, brute=brute)
        for b in (0, 2):
            assert torch.isinf(d[b]).all() and (i[b] == -1).all() and (t[b] == -1).all()
        assert (i[1] >= 0).all()
    _equal3(_pm(p, f, nf), _pm(p, f, nf, brute=True))


def test_matches_numpy_fp32_restatement(cuda):
    rng = np.random.default_rng(7)
    f, p = _soup(rng, 300), _points(rng, 400)
    d, i, t = (x[0].cpu().numpy() for x in _pm(_t(p[None], cuda), _t(f[None], cuda)))
    rd, ri, rt = R.point_to_mesh(p, f)
    assert np.array_equal(np.nan_to_num(d, nan=-1), np.nan_to_num(rd, nan=-1))
    assert np.array_equal(i, ri) and np.array_equal(t, rt)


def test_close_to_fp64_where_tri_dist_fwd_is_not(cuda):
    from deftet_amd import hip_ops
    rng = np.random.default_rng(11)
    F = 200
    tri = rng.normal(size=(F, 3, 3)).astype(np.float32) * 0.3
    tri[:F // 2, :, 0] = tri[:F // 2, :1, 0]                                            # vertical faces (x constant)
    tri[F // 2:, :, 0] = tri[F // 2:, :1, 0] + 1e-4 * rng.normal(size=(F - F // 2, 3)).astype(np.float32)   # near-vertical
    p = rng.normal(size=(2000, 3)).astype(np.float32)
    d, _, _ = _pm(_t(p[None], cuda), _t(tri[None], cuda))
    d64, _, _ = R.point_to_mesh(p.astype(np.float64), tri.astype(np.float64), np.float64)
    L2 = float(np.square(np.concatenate([p, tri.reshape(-1, 3)]).max(0) - np.concatenate([p, tri.reshape(-1, 3)]).min(0)).sum())
    err = np.abs(d[0].cpu().numpy().astype(np.float64) - d64).max()
    assert err <= 1e-6 * L2, (err, L2)
    a9, _ = hip_ops.tri_dist_fwd(_t(p[None], cuda), _t(tri[None], cuda), torch.tensor([float(F)], device=cuda))
    assert np.abs(a9[0, :, 0].cpu().numpy().astype(np.float64) - d64).max() > 1e3 * max(err, 1e-12)


def _sphere(n_lat, r=0.4):
    sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
    from tools.eval_metrics_ab import uv_sphere, predicted_surface
    return uv_sphere, predicted_surface


def test_full_size_grid_equals_scan(cuda):
    uv_sphere, predicted_surface = _sphere(0)
    gv, gf = uv_sphere(205000)
    assert len(gf) >= 200000
    pv, pf = predicted_surface(70)
    rng = np.random.default_rng(1)
    p = (rng.normal(size=(100000, 3)) * 0.25).astype(np.float32)
    for v, f in ((gv, gf), (pv, pf)):
        tri = _t(v[f][None], cuda)
        _equal3(_pm(_t(p[None], cuda), tri), _pm(_t(p[None], cuda), tri, brute=True))


def test_ragged_batch_equals_per_shape(cuda):
    rng = np.random.default_rng(4)
    f = np.stack([_soup(rng, 1000), _soup(rng, 1000, 2.0), _soup(rng, 1000, 0.5)])
    p = np.stack([_points(rng, 800) for _ in range(3)])
    n = [1000, 321, 17]
    ft, pt = _t(f, cuda), _t(p, cuda)
    g = _pm(pt, ft, torch.tensor(n, dtype=torch.int32, device=cuda))
    for b in range(3):
        _equal3([x[b] for x in g], [x[0] for x in _pm(pt[b:b + 1], ft[b:b + 1, :n[b]])])


def test_sided_distance(cuda):
    from deftet_amd import hip_ops, metrics
    g = torch.Generator(device=cuda).manual_seed(0)
    a = torch.rand(1, 100000, 3, device=cuda, generator=g)
    b = torch.rand(1, 100000, 3, device=cuda, generator=g)
    b[0, 5:10] = b[0, 0:5]                                                     # exact ties
    d, i = metrics.sided_distance(a, b)
    assert i.dtype == torch.int64 and torch.equal(i.int(), hip_ops.nn_index(a, b))
    diff = b[0][i[0]] - a[0]
    dd = torch.zeros_like(d[0])
    dd += diff[:, 0] * diff[:, 0]
    dd += diff[:, 1] * diff[:, 1]
    dd += diff[:, 2] * diff[:, 2]
    assert torch.equal(d[0], dd)
    m = torch.cat([torch.cdist(a[0, k:k + 4096].double(), b[0].double()).min(1).values for k in range(0, 100000, 4096)]) ** 2
    assert (d[0].double() - m).abs().max() <= 1e-6


def test_sampling_matches_restatement_and_areas(cuda):
    from deftet_amd import metrics
    rng = np.random.default_rng(9)
    F, N = 500, 20000
    f = rng.normal(size=(3, F, 3, 3)).astype(np.float32)
    f[:, ::7, 2] = f[:, ::7, 1]                                                  # zero area
    u = rng.random((3, N, 3)).astype(np.float32)
    n = [F, 123, 1]
    f[2, 0] = rng.normal(size=(3, 3))
    pts, ch, empty = metrics.sample_faces(_t(f, cuda), torch.tensor(n, dtype=torch.int32, device=cuda), _t(u, cuda))
    assert (empty == 0).all()
    for b in range(3):
        rp, rc = R.sample(f[b, :n[b]], u[b])
        assert np.array_equal(ch[b].cpu().numpy(), rc)
        assert np.array_equal(pts[b].cpu().numpy(), rp)
        assert not np.isin(rc, np.where(R.face_areas(f[b, :n[b]]) == 0)[0]).any()


def test_sampling_chi_square(cuda):
    from deftet_amd import metrics
    rng = np.random.default_rng(2)
    F, N = 64, 1000000
    f = rng.normal(size=(1, F, 3, 3)).astype(np.float32)
    f[0, :4, 2] = f[0, :4, 1]
    g = torch.Generator(device=cuda).manual_seed(123)
    u = torch.rand(1, N, 3, device=cuda, generator=g)
    _, ch, _ = metrics.sample_faces(_t(f, cuda), None, u)
    cnt = np.bincount(ch[0].cpu().numpy(), minlength=F)
    assert cnt[:4].sum() == 0
    a = R.face_areas(f[0]).astype(np.float64)
    e = a / a.sum() * N
    chi2 = (((cnt - e) ** 2)[4:] / e[4:]).sum()
    assert chi2 < 120, chi2                                                      # 59 degrees of freedom: p < 1e-6 beyond 120


def test_sampling_empty_shapes(cuda):
    from deftet_amd import metrics
    f = torch.zeros(2, 3, 3, 3, device=cuda)
    f[1] = torch.rand(3, 3, 3, device=cuda)
    pts, ch, empty = metrics.sample_faces(f, torch.tensor([3, 0], dtype=torch.int32, device=cuda), torch.rand(2, 10, 3, device=cuda))
    assert empty.tolist() == [1, 1] and torch.isnan(pts).all() and (ch == -1).all()
    with pytest.raises(RuntimeError):
        metrics.sample_points(torch.zeros(1, 3, 3, device=cuda), torch.tensor([[0, 1, 2]], device=cuda), 10)


def _shapes(cuda, B=2, N=3000):
    uv_sphere, _ = _sphere(0)
    rng = np.random.default_rng(3)
    gv, gf = uv_sphere(4000)
    pv, pf = uv_sphere(1500, 0.37)
    Fg, Fp = len(gf), len(pf)
    gt = np.zeros((B, Fg, 3, 3), np.float32)
    pr = np.zeros((B, Fp, 3, 3), np.float32)
    ng, npf = [Fg, Fg - 40][:B], [Fp, Fp - 100][:B]
    for b in range(B):
        gt[b, :ng[b]] = gv[gf[:ng[b]]] * (1 + 0.1 * b)
        pr[b, :npf[b]] = pv[pf[:npf[b]]] * (1 + 0.1 * b)
    surf = np.stack([R.sample(gt[b, :ng[b]], rng.random((N, 3)).astype(np.float32))[0] for b in range(B)])
    u = rng.random((B, N, 3)).astype(np.float32)
    t = lambda x: _t(x, cuda)                                                    # noqa: E731
    return t(pr), torch.tensor(npf, dtype=torch.int32, device=cuda), t(gt), torch.tensor(ng, dtype=torch.int32, device=cuda), t(surf), t(u)


def test_surface_metrics_against_fp64_and_run_to_run(cuda):
    from deftet_amd import metrics
    pr, npf, gt, ng, surf, u = _shapes(cuda)
    with torch.no_grad():
        r1 = metrics.surface_metrics(pr, npf, gt, ng, surf, uniforms=u)
        r2 = metrics.surface_metrics(pr, npf, gt, ng, surf, uniforms=u)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    pts, _, _ = metrics.sample_faces(pr, npf, u)
    for b in range(2):
        da, _, _ = R.point_to_mesh(surf[b].cpu().numpy().astype(np.float64), pr[b, :npf[b]].cpu().numpy().astype(np.float64), np.float64)
        db, _, _ = R.point_to_mesh(pts[b].cpu().numpy().astype(np.float64), gt[b, :ng[b]].cpu().numpy().astype(np.float64), np.float64)
        ref = R.metric_block(surf[b].cpu().numpy(), pts[b].cpu().numpy(), da, db)
        for k, v in ref.items():
            assert abs(float(r1[k][b]) - v) <= 1e-5 * max(abs(v), 1e-3), (k, float(r1[k][b]), v)
    with pytest.raises(RuntimeError):
        metrics.surface_metrics(pr.requires_grad_(), npf, gt, ng, surf, uniforms=u)


def test_surface_metrics_batch_equals_per_shape(cuda):
    from deftet_amd import metrics
    pr, npf, gt, ng, surf, u = _shapes(cuda)
    with torch.no_grad():
        r = metrics.surface_metrics(pr, npf, gt, ng, surf, uniforms=u)
        for b in range(2):
            rb = metrics.surface_metrics(pr[b:b + 1, :int(npf[b])], None, gt[b:b + 1, :int(ng[b])], None, surf[b:b + 1], uniforms=u[b:b + 1])
            for k in r:
                assert torch.equal(r[k][b:b + 1], rb[k]), k


def _eval_style_caller(kal, mesh_v, mesh_f, gt_v, gt_f, surface_point, n):
    """eval's call sequence, written afresh: sample the prediction, three sided-distance metrics, two point-to-mesh queries"""
    pred, _ = kal.ops.mesh.sample_points(mesh_v[None], mesh_f, n)
    sd = kal.metrics.pointcloud.sided_distance
    d12, i12 = sd(surface_point, pred)
    d21, i21 = sd(pred, surface_point)
    a, b = torch.sqrt(d12 + 1e-15), torch.sqrt(d21 + 1e-15)
    chamfer = (a.mean() + b.mean()) / 2
    fa = kal.ops.mesh.index_vertices_by_faces(mesh_v[None], mesh_f)
    ha, _, _ = kal.metrics.trianglemesh.point_to_mesh_distance(surface_point, fa)
    fb = kal.ops.mesh.index_vertices_by_faces(gt_v[None], gt_f)
    hb, _, _ = kal.metrics.trianglemesh.point_to_mesh_distance(pred, fb)
    mean_h = ((torch.sqrt(ha + 1e-15) + torch.sqrt(hb + 1e-15)) / 2).mean()
    return pred, chamfer, mean_h


def test_through_the_overlay(cuda):
    from deftet_amd import metrics, overlay
    uv_sphere, _ = _sphere(0)
    saved = {k: v for k, v in sys.modules.items() if k == "kaolin" or k.startswith("kaolin.")}
    names = overlay.install(kaolin=True)
    try:
        kal = importlib.import_module("kaolin")
        gv, gf = uv_sphere(3000)
        pv, pf = uv_sphere(1000, 0.38)
        gv, gf, pv, pf = _t(gv, cuda), _t(gf, cuda), _t(pv, cuda), _t(pf, cuda)
        g = torch.Generator(device=cuda).manual_seed(5)
        surf, _ = metrics.sample_points(gv[None], gf, 4000, generator=g)
        with torch.no_grad():
            torch.manual_seed(6)
            pred, chamfer, mean_h = _eval_style_caller(kal, pv, pf, gv, gf, surf, 4000)
            torch.manual_seed(6)
            u = torch.rand(1, 4000, 3, device=cuda)
            r = metrics.surface_metrics(pv[pf][None], None, gv[gf][None], None, surf, uniforms=u)
        assert abs(float(chamfer) - float(r["chamfer"][0])) <= 1e-5 * float(chamfer)
        assert abs(float(mean_h) - float(r["mean_hausdorff"][0])) <= 1e-5 * float(mean_h)
    finally:
        overlay.uninstall(names)
        sys.modules.update(saved)
