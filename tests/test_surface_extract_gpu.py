"""Surface extraction on the GPU against the numpy restatement (tests/surface_extract_ref.py) and the reference's fixtures
(tests/golden/gen_surface_extract.py): exact equality on every row of every output of every shape; nothing is compared against
the library itself.  Properties of the extracted surface are checked in float64."""
import os

import numpy as np
import pytest
import torch

from deftet_amd import grids
from tests import surface_extract_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
_tables = {}


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ref_table(key, tets):
    if key not in _tables:
        _tables[key] = R.neighbour_table(tets)
    return _tables[key]


def gpu_table(cuda, tets, n_point, want):
    from deftet_amd import hip_ops
    nbr = hip_ops.tet_face_neighbours(tets, n_point, cuda)
    assert nbr.table.dtype == torch.int64 and nbr.table32.dtype == torch.int32
    assert same(nbr.table, want) and same(nbr.table32, want.astype(np.int32))
    return nbr


def check(cuda, nbr, want_nbr, tets, tet_p, occ, mode, h=None, attr=None, weights=None, wrap=lambda t: t):
    """every output of hip_ops.surface_extract for the batch against the restatement, shape by shape; returns the counts"""
    from deftet_amd import hip_ops
    B = tet_p.shape[0]
    dev = lambda x: None if x is None else wrap(torch.from_numpy(np.ascontiguousarray(x)).to(cuda))
    soup = hip_ops.surface_extract(dev(tet_p), dev(occ), nbr, mode, thres=h, attr=dev(attr), vertex_weights=dev(weights),
                                   tet_idx=torch.from_numpy(tets.astype(np.int64)).to(cuda), return_index=True, return_faces=True)
    counts = []
    for b in range(B):
        o = R.occ_from_weights(weights[b], tets) if occ is None else occ[b].reshape(-1)
        want = R.extract(tet_p[b], o, want_nbr, mode, h, attr_tx4xc=None if attr is None else attr[b], tets=tets)
        assert same(soup.face[b], want["face"]), (mode, h, b)
        assert same(soup.index[b], want["index"]) and same(soup.faces[b], want["faces"]), (mode, h, b)
        if attr is not None:
            assert same(soup.face_attr[b], want["face_attr"]), (mode, h, b)
        else:
            assert soup.face_attr is None
        # index: tet[b, t][corner table][i] is the face
        t, i = soup.index[b][:, 0].cpu().numpy(), soup.index[b][:, 1].cpu().numpy()
        assert same(soup.face[b], tet_p[b][t[:, None], R.CORNER[i]])
        counts.append(want["face"].shape[0])
    return counts, soup


@pytest.mark.parametrize("grid", ["kuhn2", "kuhn4", "soup2"])
def test_fixtures(cuda, grid):
    from deftet_amd import hip_ops
    from deftet_amd.render import utils_tetsv
    from deftet_amd.utils import tet_utils
    g = np.load(os.path.join(GOLD, "surface_extract.npz"))
    tets = g[grid + "_tets"]
    t64 = tets.astype(np.int64)
    V = g[grid + "_pos"].shape[0]
    nbr = gpu_table(cuda, tets, V, g[grid + "_nbr"])
    tet_p, tet_c = g[grid + "_pos"][t64][None], g[grid + "_col"][t64][None]
    at = 0
    for k, occ in enumerate(g[grid + "_th_occ"]):
        for j, h in enumerate(R.THRESHOLDS):
            n = int(g[grid + "_th_count"][k, j])
            f, c = utils_tetsv.get_face_use_occ_color(tet_p, tet_c, occ.reshape(-1, 1), nbr, h)      # numpy in, numpy out
            assert isinstance(f[0], np.ndarray) and same(f[0], g[grid + "_th_face"][at:at + n]), (grid, k, h)
            assert same(c[0], g[grid + "_th_fcol"][at:at + n]), (grid, k, h)
            f = utils_tetsv.get_face_use_occ(torch.from_numpy(tet_p).to(cuda), torch.from_numpy(occ).to(cuda).reshape(-1, 1), nbr, h)
            assert f[0].is_cuda and same(f[0], g[grid + "_th_face"][at:at + n])
            at += n
    at = 0
    for k, occ2 in enumerate(g[grid + "_bin_occ"]):
        res = tet_utils.get_face_use_occ(torch.from_numpy(g[grid + "_bin_pos"][:, t64]).to(cuda), torch.from_numpy(occ2).to(cuda).reshape(2, -1, 1), nbr)
        for b in range(2):
            n = int(g[grid + "_bin_count"][k, b])
            assert same(res[b], g[grid + "_bin_face"][at:at + n]), (grid, k, b)
            at += n
    # the reference's own list of sparse matrices as tet_adj, and get_tet_adj
    from scipy.sparse import coo_matrix
    want = g[grid + "_nbr"]
    mats = []
    for i in range(4):
        rows = np.nonzero(want[:, i] >= 0)[0]
        mats.append(coo_matrix((np.ones(rows.size), (rows, want[rows, i])), shape=(want.shape[0],) * 2))
    occ = g[grid + "_th_occ"][0]
    f = utils_tetsv.get_face_use_occ(tet_p, occ.reshape(-1, 1), mats, 0.25)
    assert same(f[0], g[grid + "_th_face"][int(g[grid + "_th_count"][0, :3].sum()):int(g[grid + "_th_count"][0].sum())])
    once = hip_ops.neighbours_from_adj_list(mats, cuda)                                                        # converted once, then reused
    assert hip_ops.neighbours_from_adj_list(once, cuda) is once and same(once.table, want)
    assert same(utils_tetsv.get_face_use_occ(tet_p, occ.reshape(-1, 1), once, 0.25)[0], f[0])
    assert same(tet_utils.get_tet_adj(tets, V, cuda).table, want)


def test_saveobj_fixture(cuda, tmp_path):
    from deftet_amd import hip_ops
    from deftet_amd.render import export
    g = np.load(os.path.join(GOLD, "surface_extract.npz"))
    tets = g["kuhn2_tets"]
    nbr = hip_ops.tet_face_neighbours(tets, g["kuhn2_pos"].shape[0], cuda)
    paths = export.save_surface_objs(torch.from_numpy(g["kuhn2_pos"]).to(cuda), (torch.from_numpy(g["save_weights"]).to(cuda),
                                     torch.from_numpy(g["save_colours"]).to(cuda)), tets, nbr, str(tmp_path), "fx")
    assert [os.path.basename(p) for p in paths] == [n % h for h in ("0.005", "0.050", "0.150", "0.250")
                                                    for n in ("tet-geo-fx-thres-%s.obj", "tet-color-fx-thres-%s.obj")]
    for h in R.THRESHOLDS:
        assert open(tmp_path / ("tet-geo-fx-thres-%.3f.obj" % h), "rb").read() == g["save_geo_%.3f" % h].tobytes()
        assert open(tmp_path / ("tet-color-fx-thres-%.3f.obj" % h), "rb").read() == g["save_color_%.3f" % h].tobytes()


def sphere_occ(pos_bxvx3, tets, r=0.3):
    """1 where the tet's centroid lies within r of the origin"""
    c = pos_bxvx3[:, tets.astype(np.int64)].mean(2)
    return (np.linalg.norm(c, axis=-1) < r).astype(np.float32)


def test_cube40_grid(cuda):
    d = np.load(os.path.join(GOLD, "cube40_grid.npz"))
    tets, verts = d["tets"], d["verts"]
    want = ref_table("cube40", tets)
    nbr = gpu_table(cuda, tets, verts.shape[0], want)
    pos = (verts - verts.mean(0)).astype(np.float32)[None]
    pos = pos / np.abs(pos).max() * 0.5
    tet_p = grids.gather_tets(pos, tets)
    rng = np.random.default_rng(5)
    for occ in (sphere_occ(pos, tets), (rng.random((1, tets.shape[0])) < 0.5).astype(np.float32)):
        n, _ = check(cuda, nbr, want, tets, tet_p, occ, "binary")
        assert n[0] > 0
        check(cuda, nbr, want, tets, tet_p, occ, "threshold", 0.25)
    check(cuda, nbr, want, tets, tet_p, rng.random((1, tets.shape[0])).astype(np.float32), "threshold", 0.15)


@pytest.mark.parametrize("res", [8, 20])
@pytest.mark.parametrize("shuffle", [False, True], ids=["native", "shuffled"])
def test_jittered_kuhn_batches(cuda, res, shuffle):
    verts, tets = grids.kuhn_grid(res)
    if shuffle:
        tets = tets[np.random.default_rng(res).permutation(tets.shape[0])]
    want = ref_table(("kuhn", res, shuffle), tets)
    nbr = gpu_table(cuda, tets, verts.shape[0], want)
    pos = grids.jittered_positions(verts, res, 3)
    tet_p = grids.gather_tets(pos, tets)
    T = tets.shape[0]
    rng = np.random.default_rng(res + 1)
    occ = np.stack([sphere_occ(pos[:1], tets)[0], np.zeros(T, np.float32), np.ones(T, np.float32)])       # some, none, every tet
    n, _ = check(cuda, nbr, want, tets, tet_p, occ, "binary")
    assert n[0] > 0 and n[1] == 0 and n[2] == 0                                                        # (no grid-boundary faces)
    n, _ = check(cuda, nbr, want, tets, tet_p, occ, "threshold", 0.25)
    assert n[0] > 0 and n[1] == 0 and n[2] > n[0] and len(set(n)) == 3                                   # the full shape: the grid's hull
    occ = np.stack([rng.random(T).astype(np.float32), (rng.random(T) < 0.3).astype(np.float32), R.threshold_occupancies(T, want, 9)[3]])
    occ[0, 5] = np.nan
    for h in R.THRESHOLDS:
        check(cuda, nbr, want, tets, tet_p, occ, "threshold", h, attr=rng.random((3, T, 4, 3)).astype(np.float32))
    check(cuda, nbr, want, tets, tet_p, occ[:, :, None], "binary")
    if res == 20 and not shuffle:
        for C in (1, 8):
            check(cuda, nbr, want, tets, tet_p, occ, "threshold", 0.05, attr=rng.random((3, T, 4, C)).astype(np.float32))
        w = rng.random((3, verts.shape[0])).astype(np.float32)
        w[1, 7] = np.nan
        check(cuda, nbr, want, tets, tet_p, None, "threshold", 0.25, weights=w)
        # a non-default stream, and non-contiguous inputs
        s = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(s):
            check(cuda, nbr, want, tets, tet_p, occ, "threshold", 0.15, attr=rng.random((3, T, 4, 3)).astype(np.float32))
        s.synchronize()

        def strided(t):
            if t.dim() < 2:
                return t
            wide = torch.zeros(t.shape + (2,), dtype=t.dtype, device=t.device)
            wide[..., 1] = t
            v = wide[..., 1]
            assert not v.is_contiguous()
            return v
        check(cuda, nbr, want, tets, tet_p, occ, "threshold", 0.15, attr=rng.random((3, T, 4, 3)).astype(np.float32), wrap=strided)
        check(cuda, nbr, want, tets, tet_p, occ, "binary", wrap=strided)


def test_res70_batch8_full_size(cuda):
    res, B = 70, 8
    verts, tets = grids.kuhn_grid(res)
    want = ref_table(("kuhn", res, False), tets)
    nbr = gpu_table(cuda, tets, verts.shape[0], want)
    pos = grids.jittered_positions(verts, res, B)
    tet_p = grids.gather_tets(pos, tets)
    n, _ = check(cuda, nbr, want, tets, tet_p, sphere_occ(pos, tets), "binary")
    assert min(n) > 1000
    # smooth vertex weights through the fused maximum, colours with C = 3
    rng = np.random.default_rng(70)
    k = rng.uniform(2, 9, (B, 1, 3))
    w = (0.5 + 0.5 * np.sin((pos.astype(np.float64) * k).sum(-1) + rng.uniform(0, 6, (B, 1)))).astype(np.float32) * 0.6
    col = rng.random((B, verts.shape[0], 3)).astype(np.float32)
    attr = np.stack([col[b][tets.astype(np.int64)] for b in range(B)])
    n, _ = check(cuda, nbr, want, tets, tet_p, None, "threshold", 0.15, attr=attr, weights=w)
    assert min(n) > 1000


@pytest.mark.parametrize("res", [8, 20])
def test_closed_surface_properties_and_weld(cuda, res):
    """THRESHOLD with occupancy in {0,1} and htres 0.25 emits the whole boundary of the occupied union.  In float64: every directed
    edge of the indexed mesh occurs as often as its reverse, and the signed volume of the soup is MINUS the occupied volume (the
    soup's triangles face inward on a positively oriented grid).  Bound: both sides are sums of n <= 4e5 float64 terms of
    products of float32 inputs, so they agree to n u sum|term| with u = 2^-53 (< 5e-11 sum|term|); 1e-10 sum|term| is asserted."""
    from deftet_amd import hip_ops
    verts, tets = grids.kuhn_grid(res)
    want = ref_table(("kuhn", res, False), tets)
    nbr = hip_ops.tet_face_neighbours(tets, verts.shape[0], cuda)
    pos = grids.jittered_positions(verts, res, 2)
    tet_p = grids.gather_tets(pos, tets)
    rng = np.random.default_rng(res)
    occ = np.stack([sphere_occ(pos[:1], tets, 0.35)[0], (rng.random(tets.shape[0]) < 0.4).astype(np.float32)])
    _, soup = check(cuda, nbr, want, tets, tet_p, occ, "threshold", 0.25)
    for b in range(2):
        f = soup.face[b].cpu().numpy().astype(np.float64)
        terms = np.einsum("fi,fi->f", f[:, 0], np.cross(f[:, 1], f[:, 2])) / 6
        vol = (grids.tet_orientation(tet_p[b:b + 1])[0] / 6)[occ[b] == 1]
        assert vol.min() > 0
        assert abs(terms.sum() + vol.sum()) <= 1e-10 * (np.abs(terms).sum() + np.abs(vol).sum())
        ids = soup.faces[b].cpu().numpy()
        V = verts.shape[0]
        e = np.concatenate([ids[:, [0, 1]], ids[:, [1, 2]], ids[:, [2, 0]]])
        fwd, nf = np.unique(e[:, 0] * V + e[:, 1], return_counts=True)
        rev, nr = np.unique(e[:, 1] * V + e[:, 0], return_counts=True)
        assert np.array_equal(fwd, rev) and np.array_equal(nf, nr)
        # weld: verts[faces] is the soup bit for bit, old ids strictly ascending = the used ids
        col = rng.random((V, 3)).astype(np.float32)
        v, a, fnew, old = hip_ops.surface_weld(torch.from_numpy(pos[b]).to(cuda), soup.faces[b], torch.from_numpy(col).to(cuda))
        wv, wa, wf, wold = R.weld(ids, pos[b], col)
        assert same(old, wold) and (np.diff(old.cpu().numpy()) > 0).all() and same(old, np.unique(ids))
        assert same(v, wv) and same(a, wa) and same(fnew, wf)
        assert same(v[fnew], soup.face[b].cpu().numpy())
        v2, a2, _f2, _o2 = hip_ops.surface_weld(torch.from_numpy(pos[b]).to(cuda), soup.faces[b])
        assert a2 is None and same(v2, wv)
    with pytest.raises(RuntimeError, match="outside"):
        hip_ops.surface_weld(torch.from_numpy(pos[0]).to(cuda), torch.full((2, 3), verts.shape[0], dtype=torch.long, device=cuda))
    v, a, fnew, old = hip_ops.surface_weld(torch.from_numpy(pos[0]).to(cuda), torch.zeros(0, 3, dtype=torch.long, device=cuda))
    assert v.shape == (0, 3) and fnew.shape == (0, 3) and old.shape == (0,)


def test_save_surface_objs_end_to_end(cuda, tmp_path):
    from deftet_amd import hip_ops
    from deftet_amd.render import export
    res = 20
    verts, tets = grids.kuhn_grid(res)
    want = ref_table(("kuhn", res, False), tets)
    nbr = hip_ops.tet_face_neighbours(tets, verts.shape[0], cuda)
    pos = grids.jittered_positions(verts, res, 1)[0]
    rng = np.random.default_rng(3)
    w = (0.3 + 0.3 * np.sin(pos.astype(np.float64) @ np.array([5.0, 3.0, 7.0]))).astype(np.float32)[:, None]
    col = rng.random((verts.shape[0], 3)).astype(np.float32)
    feat = torch.from_numpy(np.concatenate([w, col], 1)).to(cuda)                                        # [P,4]: weights and colours side by side
    paths = export.save_surface_objs(torch.from_numpy(pos).to(cuda), feat, torch.from_numpy(tets).to(cuda), nbr, str(tmp_path), "e2e", welded=True)
    assert len(paths) == 12
    t64 = tets.astype(np.int64)
    rev = col[:, ::-1]
    occ = R.occ_from_weights(w, tets)
    for h in R.THRESHOLDS:
        got = R.extract(pos[t64], occ, want, "threshold", h, attr_tx4xc=rev[t64], tets=tets)
        assert got["face"].shape[0] > 100
        assert open(tmp_path / ("tet-geo-e2e-thres-%.3f.obj" % h)).read() == R.obj_text(got["face"])
        assert open(tmp_path / ("tet-color-e2e-thres-%.3f.obj" % h)).read() == R.obj_color_text(got["face"], got["face_attr"])
        wv, wa, wf, _ = R.weld(got["faces"], pos, np.ascontiguousarray(rev))
        text = "".join("v %f %f %f %f %f %f\n" % (p[0], p[1], p[2], c[0], c[1], c[2]) for p, c in zip(wv, wa))
        text += "".join("f %d %d %d\n" % (f[0] + 1, f[2] + 1, f[1] + 1) for f in wf)
        assert open(tmp_path / ("tet-mesh-e2e-thres-%.3f.obj" % h)).read() == text


def test_bad_channel_counts_and_mismatched_fill(cuda):
    """C outside 1..8 is refused; a fill pass asked for the fused occupancy after a count pass on a given one writes no row"""
    from deftet_amd import _lib, hip_ops
    verts, tets = grids.kuhn_grid(8)
    T = tets.shape[0]
    nbr = hip_ops.tet_face_neighbours(tets, verts.shape[0], cuda)
    tet_p = torch.from_numpy(grids.gather_tets(grids.jittered_positions(verts, 8, 1), tets)).to(cuda)
    occ = torch.ones(1, T, device=cuda)
    for C in (0, 9):
        with pytest.raises(_lib.DefTetHipError, match="1 <= C <= 8"):
            hip_ops.surface_extract(tet_p, occ, nbr, "threshold", thres=0.25, attr=torch.zeros(1, T, 4, C, device=cuda))
    lib = _lib.load()
    wsb = lib.deftet_surface_extract_workspace_bytes(1, T, 1)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=cuda)
    offs = torch.zeros(2, dtype=torch.int32, device=cuda)
    st = _lib.current_stream(cuda)
    _lib.check(lib.deftet_surface_extract_count_f32(occ.data_ptr(), None, None, 0, nbr.table32.data_ptr(), 1, T, 1, 0.25, offs.data_ptr(),
                                                    ws.data_ptr(), wsb, st), "count")
    F = int(offs[1])
    assert F == 6 * 2 * 16                                                                              # the grid's hull
    face = torch.full((F, 3, 3), -7.0, device=cuda)
    args = [None, 0, None, None, nbr.table32.data_ptr(), 1, T, 1, 0.25, F, face.data_ptr(), None, None, None, ws.data_ptr(), wsb, st]
    _lib.check(lib.deftet_surface_extract_fill_f32(tet_p.data_ptr(), *args), "fill")                     # occ NULL: the other occupancy
    assert bool((face == -7.0).all())
    args[2] = occ.data_ptr()
    _lib.check(lib.deftet_surface_extract_fill_f32(tet_p.data_ptr(), *args), "fill")
    want = R.extract(tet_p[0].cpu().numpy(), np.ones(T, np.float32), R.neighbour_table(tets), "threshold", 0.25)
    assert same(face, want["face"])
