"""Surface extraction without a GPU: the numpy restatement (tests/surface_extract_ref.py) reproduces every fixture the reference
wrote (tests/golden/gen_surface_extract.py) exactly, row order included; the whole-array OBJ writers reproduce the reference's
bytes; the library exports the six entry points and rejects bad arguments with DEFTET_EINVAL and a message before any device work;
the drop-in modules import on a CPU-only host and refuse CPU tensors; the sparse-list adapter yields the restatement's table."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import surface_extract_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
GRIDS = ("kuhn2", "kuhn4", "soup2")
SYMBOLS = ("deftet_tet_face_neighbours_i64", "deftet_surface_extract_workspace_bytes", "deftet_surface_extract_count_f32",
           "deftet_surface_extract_fill_f32", "deftet_surface_weld_workspace_bytes", "deftet_surface_weld_f32")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "surface_extract.npz"))


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("grid", GRIDS)
def test_restatement_neighbour_table_equals_the_reference(gold, grid):
    assert np.array_equal(R.neighbour_table(gold[grid + "_tets"]), gold[grid + "_nbr"])


@pytest.mark.parametrize("grid", GRIDS)
def test_restatement_equals_the_threshold_fixtures(gold, grid):
    tets = gold[grid + "_tets"].astype(np.int64)
    nbr = R.neighbour_table(tets)
    tet_p, tet_c = gold[grid + "_pos"][tets], gold[grid + "_col"][tets]
    occs, counts = gold[grid + "_th_occ"], gold[grid + "_th_count"]
    assert np.array_equal(occs, R.threshold_occupancies(tets.shape[0], nbr, 200 + GRIDS.index(grid)), equal_nan=True)
    at = 0
    for k, occ in enumerate(occs):
        for j, h in enumerate(R.THRESHOLDS):
            got = R.extract(tet_p, occ, nbr, "threshold", h, attr_tx4xc=tet_c)
            n = int(counts[k, j])
            assert got["face"].shape[0] == n, (grid, k, h)
            assert same(got["face"], gold[grid + "_th_face"][at:at + n]), (grid, k, h)
            assert same(got["face_attr"], gold[grid + "_th_fcol"][at:at + n]), (grid, k, h)
            at += n
    assert at == gold[grid + "_th_face"].shape[0]
    assert counts[-2].sum() == 0 and counts.max() > 0                  # a shape with no face is among them


@pytest.mark.parametrize("grid", GRIDS)
def test_restatement_equals_the_binary_fixtures(gold, grid):
    tets = gold[grid + "_tets"].astype(np.int64)
    nbr = R.neighbour_table(tets)
    at = 0
    for k, occ2 in enumerate(gold[grid + "_bin_occ"]):
        for b in range(2):
            got = R.extract(gold[grid + "_bin_pos"][b][tets], occ2[b], nbr, "binary")
            n = int(gold[grid + "_bin_count"][k, b])
            assert same(got["face"], gold[grid + "_bin_face"][at:at + n]), (grid, k, b)
            at += n
    assert at == gold[grid + "_bin_face"].shape[0]


def test_thresholds_are_pinned_on_both_comparisons(gold):
    """the fixtures hold occupancies ON the comparisons: evaluating either of them in the other precision changes the rows"""
    tets = gold["kuhn4_tets"].astype(np.int64)
    nbr = R.neighbour_table(tets)
    differs32 = differs64 = False
    for occ in gold["kuhn4_th_occ"][2:6]:
        for h in R.THRESHOLDS:
            o = occ[:, None]
            no = np.where(nbr >= 0, occ[np.where(nbr >= 0, nbr, 0)], np.float32(0))
            m = R.face_mask(occ, nbr, "threshold", h)
            differs32 |= not np.array_equal(m, (np.abs(no - o) > np.float32(h)) & (o > np.float32(h * 2)))
            differs64 |= not np.array_equal(m, (np.abs(no.astype(np.float64) - o) > h) & (o.astype(np.float64) > h * 2))
    assert differs32 and differs64


def _saveobj_inputs(gold):
    tets = gold["kuhn2_tets"].astype(np.int64)
    rev = gold["save_colours"][:, ::-1]
    return tets, gold["kuhn2_pos"][tets], rev[tets], R.occ_from_weights(gold["save_weights"], tets), R.neighbour_table(tets)


def test_writers_reproduce_the_reference_bytes(gold):
    from deftet_amd.render import export
    tets, tet_p, tet_c, occ, nbr = _saveobj_inputs(gold)
    for h in R.THRESHOLDS:
        got = R.extract(tet_p, occ, nbr, "threshold", h, attr_tx4xc=tet_c)
        geo, col = gold["save_geo_%.3f" % h].tobytes(), gold["save_color_%.3f" % h].tobytes()
        assert R.obj_text(got["face"]).encode() == geo and R.obj_color_text(got["face"], got["face_attr"]).encode() == col
        assert export.soup_obj_text(got["face"]).encode() == geo
        assert export.soup_color_obj_text(got["face"], got["face_attr"]).encode() == col
        assert export.soup_obj_text(torch.from_numpy(got["face"])).encode() == geo
    assert open(os.path.join(GOLD, "surface_extract_tet-geo-thres-0.050.obj"), "rb").read() == gold["save_geo_0.050"].tobytes()
    assert open(os.path.join(GOLD, "surface_extract_tet-color-thres-0.050.obj"), "rb").read() == gold["save_color_0.050"].tobytes()


def test_writers_format_blocks_specials_and_files(tmp_path, monkeypatch):
    from deftet_amd.render import export, utils_tetsv
    from deftet_amd.utils import tet_utils
    rng = np.random.default_rng(0)
    tri = (rng.normal(size=(700, 3, 3)) * 1e3).astype(np.float32)
    tri[3, 1, 2], tri[5, 0, 0], tri[6, 2, 1], tri[7, 0, 1] = np.nan, np.inf, -np.inf, -0.0
    col = rng.random((700, 3, 3)).astype(np.float32)
    monkeypatch.setattr(export, "_BLOCK", 64)                          # several blocks
    assert export.soup_obj_text(tri) == R.obj_text(tri)
    assert export.soup_color_obj_text(tri, col) == R.obj_color_text(tri, col)
    assert export.soup_obj_text(tri[:0]) == ""
    utils_tetsv.save_tet_face(tri, str(tmp_path / "a.obj"))
    tet_utils.save_tet_face(torch.from_numpy(tri), str(tmp_path / "b.obj"))
    utils_tetsv.save_tet_face_color(tri, col, str(tmp_path / "c.obj"))
    assert (tmp_path / "a.obj").read_text() == R.obj_text(tri) == (tmp_path / "b.obj").read_text()
    assert (tmp_path / "c.obj").read_text() == R.obj_color_text(tri, col)
    v = rng.normal(size=(5, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4]])
    assert export.mesh_obj_text(v, f) == "".join("v %f %f %f\n" % tuple(p) for p in v) + "f 1 3 2\nf 3 5 4\n"


def test_library_exports_the_entry_points(lib):
    raw = ctypes.CDLL(importlib.import_module("deftet_amd._lib").LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    assert lib.deftet_version() >= 270
    assert lib.deftet_surface_extract_workspace_bytes(8, 257250, 1) > 8 * 257250 * 4
    assert lib.deftet_surface_weld_workspace_bytes(46656) > 46656 * 4


def _buf(nbytes, align=256, offset=0):
    raw = ctypes.create_string_buffer(nbytes + align * 2)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + align - 1) // align * align + offset)


def _count(lib, B=2, T=8, V=9, mode=1, htres=0.25, null=None, wsb=None, ws_off=0, weights=False, both=False):
    bufs = dict(occ=_buf(4 * 2 * 8), w=_buf(4 * 2 * 9), idx=_buf(16 * 8), nbr=_buf(16 * 8), offs=_buf(4 * 3), ws=_buf(1 << 16, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    need = lib.deftet_surface_extract_workspace_bytes(2, 8, int(weights))
    return lib.deftet_surface_extract_count_f32(None if weights and not both else a["occ"], a["w"] if weights or both else None, a["idx"], V,
                                                a["nbr"], B, T, mode, htres, a["offs"], a["ws"], need if wsb is None else wsb, None)


@pytest.mark.parametrize("bad", [dict(T=0), dict(T=-3), dict(B=0), dict(mode=2), dict(mode=-1), dict(null="occ"), dict(null="nbr"),
                                 dict(null="offs"), dict(null="ws"), dict(wsb=64), dict(ws_off=64), dict(both=True),
                                 dict(weights=True, null="idx"), dict(weights=True, V=0), dict(htres=float("nan"))], ids=str)
def test_count_rejects_bad_arguments(lib, bad):
    assert _count(lib, **bad) == EINVAL
    assert lib.deftet_last_error()


def _fill(lib, B=2, T=8, C=3, mode=0, null=None, wsb=None, cap=4, attr=True, faces=True, occ=True):
    bufs = dict(tet=_buf(48 * 16), attr=_buf(4 * 16 * 4 * 8), occ=_buf(64), idx=_buf(128), nbr=_buf(128), face=_buf(36 * 4), fattr=_buf(96 * 4),
                index=_buf(64), faces=_buf(96), ws=_buf(1 << 16))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    need = lib.deftet_surface_extract_workspace_bytes(2, 8, int(not occ))
    return lib.deftet_surface_extract_fill_f32(a["tet"], a["attr"] if attr else None, C, a["occ"] if occ else None, a["idx"], a["nbr"], B, T, mode,
                                               0.25, cap, a["face"], a["fattr"] if attr else None, a["index"], a["faces"] if faces else None,
                                               a["ws"], need if wsb is None else wsb, None)


@pytest.mark.parametrize("bad", [dict(T=0), dict(B=-1), dict(C=0), dict(C=9), dict(mode=7), dict(null="tet"), dict(null="face"), dict(null="nbr"),
                                 dict(null="fattr"), dict(null="attr"), dict(null="idx"), dict(null="ws"), dict(wsb=16), dict(cap=-1),
                                 dict(occ=False, wsb=256)], ids=str)
def test_fill_rejects_bad_arguments(lib, bad):
    assert _fill(lib, **bad) == EINVAL
    assert lib.deftet_last_error()


def test_neighbours_and_weld_reject_bad_arguments(lib):
    t2, tf2, n64, n32 = _buf(64), _buf(64), _buf(32 * 8), _buf(16 * 8)
    call = lib.deftet_tet_face_neighbours_i64
    assert call(t2[1], tf2[1], 4, 0, n64[1], n32[1], None) == EINVAL
    assert call(t2[1], tf2[1], -1, 8, n64[1], n32[1], None) == EINVAL
    assert call(None, tf2[1], 4, 8, n64[1], n32[1], None) == EINVAL
    assert call(t2[1], tf2[1], 4, 8, None, None, None) == EINVAL and b"null" in lib.deftet_last_error()
    f, v, at, n, old, vo, ao, fo, ws = (_buf(1 << 12) for _ in range(9))
    need = lib.deftet_surface_weld_workspace_bytes(9)
    weld = lib.deftet_surface_weld_f32
    ok = [f[1], 4, v[1], at[1], 3, 9, 9, n[1], old[1], vo[1], ao[1], fo[1], ws[1], need, None]

    def bad(**kw):
        names = ["faces", "F", "verts", "attr", "C", "V", "cap", "n", "old", "vo", "ao", "fo", "ws", "wsb", "st"]
        args = list(ok)
        for k, val in kw.items():
            args[names.index(k)] = val
        return weld(*args)
    for kw in (dict(F=-1), dict(V=0), dict(C=0), dict(C=9), dict(n=None), dict(faces=None), dict(verts=None), dict(old=None), dict(fo=None),
               dict(ao=None), dict(attr=None), dict(ws=None), dict(wsb=8), dict(cap=3), dict(cap=-1)):
        assert bad(**kw) == EINVAL, kw
        assert lib.deftet_last_error()


def test_drop_ins_import_and_refuse_cpu_tensors(gold):
    from deftet_amd import hip_ops, overlay
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.render import export, utils_tetsv
    from deftet_amd.utils import tet_utils
    tets = gold["kuhn2_tets"].astype(np.int64)
    tet_p = torch.from_numpy(gold["kuhn2_pos"][tets][None])
    occ = torch.ones(1, tets.shape[0], 1)
    nbr = hip_ops.TetFaceNeighbours(torch.from_numpy(gold["kuhn2_nbr"]), torch.from_numpy(gold["kuhn2_nbr"]).int())
    calls = [lambda: tet_utils.get_face_use_occ(tet_p, occ, nbr),
             lambda: utils_tetsv.get_face_use_occ(tet_p, occ.reshape(-1, 1), nbr, 0.25),
             lambda: utils_tetsv.get_face_use_occ_color(tet_p, tet_p, occ.reshape(-1, 1), nbr),
             lambda: hip_ops.surface_extract(tet_p, occ, nbr, "binary"),
             lambda: hip_ops.surface_weld(tet_p[0, :, 0], torch.zeros(2, 3, dtype=torch.long)),
             lambda: export.save_surface_objs(tet_p[0, :, 0], (occ.reshape(-1, 1), tet_p[0, :, 0]), tets, nbr, "/nonexistent", "x")]
    if not torch.cuda.is_available():
        calls += [lambda: tet_utils.get_tet_adj(tets, 8), lambda: utils_tetsv.get_face_use_occ(tet_p.numpy(), occ.numpy().reshape(-1, 1), nbr)]
    for c in calls:
        with pytest.raises(DefTetHipError):
            c()
    with pytest.raises(ValueError):
        hip_ops.surface_extract(tet_p, occ, nbr, "nearest")
    saved = sys.modules.get("utils_tetsv")
    names = overlay.install(kaolin=False, stub_cv2=False, render_model=True)
    try:
        assert "utils_tetsv" in names and importlib.import_module("utils_tetsv") is utils_tetsv
    finally:
        overlay.uninstall(names)
        if saved is not None:
            sys.modules["utils_tetsv"] = saved
    saved = sys.modules.pop("utils_tetsv", None)
    names = overlay.install(kaolin=False, stub_cv2=False)              # the default install does not register it
    try:
        assert "utils_tetsv" not in names and "utils_tetsv" not in sys.modules
    finally:
        overlay.uninstall(names)
        if saved is not None:
            sys.modules["utils_tetsv"] = saved
    with pytest.raises(DefTetHipError, match="1 <= C <= 8"):
        hip_ops.surface_extract(tet_p, occ, nbr, "threshold", thres=0.25, attr=torch.zeros(1, tets.shape[0], 4, 0))


@pytest.mark.parametrize("kind", ["scipy", "torch"])
def test_sparse_list_adapter_yields_the_restatement_table(gold, kind):
    from scipy.sparse import coo_matrix
    from deftet_amd import hip_ops
    tets = gold["kuhn4_tets"]
    nbr = R.neighbour_table(tets)
    T = nbr.shape[0]
    mats = []
    for i in range(4):
        rows = np.nonzero(nbr[:, i] >= 0)[0]
        m = coo_matrix((np.ones(rows.size), (rows, nbr[rows, i])), shape=(T, T))
        mats.append(m if kind == "scipy" else torch.sparse_coo_tensor(torch.from_numpy(np.stack([m.row, m.col])).long(),
                                                                      torch.from_numpy(m.data).float(), (T, T)))
    assert np.array_equal(hip_ops.adj_list_table(mats), nbr)
    assert np.array_equal(hip_ops.adj_list_table([m.tocsr() for m in mats] if kind == "scipy" else mats), nbr)
    if kind == "scipy":
        two = mats[0].tolil()
        two[0, :3] = 1
        with pytest.raises(ValueError, match="more than one"):
            hip_ops.adj_list_table([two] + mats[1:])
        half = mats[1] * 0.5
        with pytest.raises(ValueError, match="other than 1"):
            hip_ops.adj_list_table([mats[0], half] + mats[2:])
        with pytest.raises(ValueError, match="four"):
            hip_ops.adj_list_table(mats[:3])
    with pytest.raises(_cpu_error()):
        hip_ops.neighbours_from_adj_list(mats, "cpu")


def _cpu_error():
    from deftet_amd._lib import DefTetHipError
    return DefTetHipError
