"""The evaluation metrics without a GPU: the Kaolin shim resolves the four calls eval.py / point_cloud_utils.py / dataloader.py make
and its functions refuse CPU tensors; the new C entry points reject bad arguments with DEFTET_EINVAL and a message before any
device work; the fp32 Ericson restatement agrees with fp64 Ericson; the A/B tool builds its inputs up to its first GPU call."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
WS = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


@pytest.fixture()
def shim():
    from deftet_amd import overlay
    saved = {k: v for k, v in sys.modules.items() if k == "kaolin" or k.startswith("kaolin.")}
    names = overlay.install(kaolin=True)
    yield names
    overlay.uninstall(names)
    sys.modules.update(saved)


def test_kaolin_shim_resolves_the_metric_calls(shim):
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.render.deftet_sparse_render import deftet_sparse_render
    kal = importlib.import_module("kaolin")
    pc = importlib.import_module("kaolin.metrics.pointcloud")
    tm = importlib.import_module("kaolin.metrics.trianglemesh")
    assert kal.metrics.pointcloud is pc and kal.metrics.trianglemesh is tm
    v = torch.rand(1, 4, 3)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]])
    fv = kal.ops.mesh.index_vertices_by_faces(v, f)
    assert fv.shape == (1, 2, 3, 3) and torch.equal(fv[0, 1, 2], v[0, 3])
    calls = [lambda: pc.sided_distance(v, v), lambda: tm.point_to_mesh_distance(v, fv), lambda: kal.ops.mesh.sample_points(v, f, 8),
             lambda: kal.ops.mesh.check_sign(v, f, v)]
    for c in calls:
        with pytest.raises(DefTetHipError):
            c()
    from deftet_amd import metrics
    with pytest.raises(DefTetHipError):
        metrics.surface_metrics(fv, None, fv, None, v[:, :2], num_samples=2)
    from deftet_amd import overlay
    assert kal.ops.mesh.check_sign is overlay._kaolin_check_sign and kal.render.mesh.deftet_sparse_render is deftet_sparse_render


def test_sample_points_rejects_face_features(shim):
    kal = importlib.import_module("kaolin")
    with pytest.raises(NotImplementedError):
        kal.ops.mesh.sample_points(torch.rand(1, 3, 3), torch.tensor([[0, 1, 2]]), 4, face_features=torch.rand(1, 1, 3, 2))


def _buf(nbytes, align=256, offset=0):
    raw = ctypes.create_string_buffer(nbytes + align * 2)
    base = (ctypes.addressof(raw) + align - 1) // align * align + offset
    return raw, ctypes.c_void_p(base)


def _pm(lib, B=2, P=8, F=4, null=None, pts_off=0, idx_off=0, ws_off=0, wsb=None, scan=False):
    bufs = dict(pts=_buf(12 * B * P, offset=pts_off), face=_buf(36 * B * F), nf=_buf(4 * B), d=_buf(4 * B * P),
                fi=_buf(8 * B * P, offset=idx_off), dt=_buf(4 * B * P))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    if scan:
        return lib.deftet_point_mesh_distance_scan_f32(a["pts"], a["face"], a["nf"], B, P, F, a["d"], a["fi"], a["dt"], None)
    need = lib.deftet_point_mesh_distance_workspace_bytes(max(B, 0), max(P, 0), max(F, 0))
    ws = _buf(min(need, 1 << 26) if need else 256, offset=ws_off)
    return lib.deftet_point_mesh_distance_f32(a["pts"], a["face"], a["nf"], B, P, F, a["d"], a["fi"], a["dt"],
                                              None if null == "ws" else ws[1], need if wsb is None else wsb, None)


@pytest.mark.parametrize("scan", [False, True])
@pytest.mark.parametrize("bad", [dict(B=-1), dict(P=-1), dict(F=-1), dict(null="pts"), dict(null="face"), dict(null="d"),
                                 dict(null="fi"), dict(null="dt"), dict(pts_off=2), dict(idx_off=4)], ids=str)
def test_point_mesh_distance_rejects_bad_arguments(lib, bad, scan):
    assert _pm(lib, scan=scan, **bad) == EINVAL
    assert lib.deftet_last_error()


@pytest.mark.parametrize("bad", [dict(null="ws"), dict(ws_off=64), dict(wsb=256)], ids=str)
def test_point_mesh_distance_rejects_bad_workspace(lib, bad):
    assert _pm(lib, **bad) == EINVAL
    assert b"workspace" in lib.deftet_last_error()


def _samp(lib, B=2, F=4, N=8, null=None, u_off=0, ch_off=0, ws_off=0, wsb=WS):
    bufs = dict(face=_buf(36 * B * F), u=_buf(12 * B * N, offset=u_off), pts=_buf(12 * B * N), ch=_buf(8 * B * N, offset=ch_off),
                empty=_buf(4 * B), ws=_buf(WS, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_sample_points_f32(a["face"], None, None, a["u"], B, F, N, a["pts"], a["ch"], a["empty"], a["ws"], wsb, None)


@pytest.mark.parametrize("bad", [dict(B=-1), dict(F=-1), dict(N=-1), dict(null="face"), dict(null="u"), dict(null="pts"), dict(null="ch"),
                                 dict(null="empty"), dict(null="ws"), dict(u_off=2), dict(ch_off=4), dict(ws_off=64), dict(wsb=256)],
                         ids=str)
def test_sample_points_rejects_bad_arguments(lib, bad):
    assert _samp(lib, **bad) == EINVAL
    assert lib.deftet_last_error()


def _met(lib, B=2, N1=8, N2=8, Nh=8, null=None, p_off=0, ws_off=0, wsb=WS, radius=0.01):
    bufs = dict(p1=_buf(12 * B * N1, offset=p_off), p2=_buf(12 * B * N2), i12=_buf(4 * B * N1), i21=_buf(4 * B * N2), da=_buf(4 * B * Nh),
                db=_buf(4 * B * Nh), out=_buf(20 * B), ws=_buf(WS, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_surface_metrics_f32(a["p1"], a["p2"], a["i12"], a["i21"], a["da"], a["db"], B, N1, N2, Nh, radius, a["out"], a["ws"],
                                          wsb, None)


@pytest.mark.parametrize("bad", [dict(B=-1), dict(N1=0), dict(N2=-1), dict(Nh=-1), dict(null="p1"), dict(null="i21"), dict(null="out"),
                                 dict(null="da"), dict(null="ws"), dict(p_off=2), dict(ws_off=64), dict(wsb=16)], ids=str)
def test_surface_metrics_rejects_bad_arguments(lib, bad):
    assert _met(lib, **bad) == EINVAL
    assert lib.deftet_last_error()


def test_nn_distance_rejects_bad_arguments(lib):
    q, i, d = _buf(96), _buf(32), _buf(32)
    assert lib.deftet_nn_distance_f32(q[1], None, i[1], 1, 8, 4, d[1], None, None) == EINVAL
    assert lib.deftet_nn_distance_f32(q[1], q[1], i[1], -1, 8, 4, d[1], None, None) == EINVAL
    assert lib.deftet_nn_distance_f32(q[1], q[1], i[1], 1, 8, 4, d[1], _buf(64, offset=4)[1], None) == EINVAL


def test_version(lib):
    assert lib.deftet_version() >= 260


def _random_triangles(rng, n):
    tri = rng.normal(size=(n, 3, 3))
    k = n // 4
    tri[:k, 2] = tri[:k, 0] + rng.uniform(0, 1, (k, 1)) * (tri[:k, 1] - tri[:k, 0])       # collinear
    tri[k:2 * k, 1] = tri[k:2 * k, 0]                                                     # two equal corners
    tri[2 * k:2 * k + 4] = tri[2 * k:2 * k + 4, :1]                                       # a point
    tri[2 * k + 4:3 * k, :, 2] = tri[2 * k + 4:3 * k, :1, 2] + 1e-4 * rng.normal(size=(3 * k - 2 * k - 4, 3))   # near-flat in z
    return tri


def test_fp32_restatement_agrees_with_fp64():
    rng = np.random.default_rng(3)
    tri = _random_triangles(rng, 64)
    pts = rng.normal(size=(200, 3)) * 1.5
    d32, t32 = R.tri_dist(pts.astype(np.float32), tri.astype(np.float32), np.float32)
    d64, t64 = R.tri_dist(pts.astype(np.float32).astype(np.float64), tri.astype(np.float32).astype(np.float64), np.float64)
    assert np.isfinite(d32).all() and (d32 >= 0).all()
    # regular triangles: within 1e-6 L^2.  Near-collinear ones (the first quarter) are ill-conditioned for fp32 Ericson: its
    # interior branch divides by a rounding-level area, so only finiteness is asserted for them.
    L2 = 12.0 ** 2
    assert np.abs(d32 - d64)[:, 16:].max() <= 1e-6 * L2
    # away from region boundaries the region agrees: regular triangles, and points whose fp64 type is stable under a nudge
    reg = np.arange(48, 64)
    p2 = pts + 1e-4
    _, t_n = R.tri_dist(p2, tri[reg], np.float64)
    _, t_m = R.tri_dist(pts - 1e-4, tri[reg], np.float64)
    stable = (t_n == t64[:, reg]) & (t_m == t64[:, reg])
    assert stable.mean() > 0.9
    assert np.array_equal(t32[:, reg][stable], t64[:, reg][stable])


def test_point_to_mesh_restatement_rules():
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]]],
                   np.float32)
    pts = np.array([[0.2, 0.2, 1.0], [np.nan, 0, 0], [-1, -1, 0], [2, 0, 0], [0.5, -1, 0]], np.float32)
    d, f, t = R.point_to_mesh(pts, tri)
    assert d[0] == np.float32(1.0) and f[0] == 0 and t[0] == 0                   # tie between duplicates: the first
    assert np.isnan(d[1]) and f[1] == -1 and t[1] == -1
    assert t[2] == 1 and t[3] == 2 and t[4] == 4
    d, f, t = R.point_to_mesh(pts[:1], tri[:0])
    assert d[0] == np.inf and f[0] == -1 and t[0] == -1
    d, _, t = R.point_to_mesh(np.array([[0.5, 1, 0]], np.float32), np.array([[[0, 0, 0], [1, 0, 0], [2, 0, 0]]], np.float32))
    assert d[0] == np.float32(1.0) and t[0] == 4                                 # collinear: the segments


def test_sampling_restatement_never_picks_zero_area():
    rng = np.random.default_rng(0)
    tri = rng.normal(size=(50, 3, 3)).astype(np.float32)
    tri[::3, 2] = tri[::3, 1]
    pts, ch = R.sample(tri, rng.uniform(size=(4000, 3)).astype(np.float32))
    assert not np.isin(ch, np.arange(0, 50, 3)).any()
    assert R.sample(tri[::3], rng.uniform(size=(4, 3)).astype(np.float32)) is None


def test_ab_tool_builds_its_inputs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_metrics_ab.py"), "--dry-run", "--points", "2000",
                        "--gt-faces", "4000", "--res", "12"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "dry run" in r.stdout
