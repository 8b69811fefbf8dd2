"""The wide-channel vertex aggregation without a GPU (hip_ops.vertex_aggregate, deftet_amd.utils.matrix_utils, DESIGN.md section
6j): the header, the ctypes table and the built library agree on deftet_vertex_aggregate_f32; bad arguments come back as
DEFTET_EINVAL with a message before anything touches a device; the Python front ends refuse CPU tensors; the overlay registers
utils.matrix_utils only when asked; det_m and cross_dot_torch are the triple and the cross product."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


def _buf(nbytes, align=256, offset=0):
    raw = ctypes.create_string_buffer(nbytes + align * 2)
    base = (ctypes.addressof(raw) + align - 1) // align * align + offset
    return raw, ctypes.c_void_p(base)


def _call(lib, B=2, V=4, C=8, nnz=6, null=(), x_off=0, out_off=0):
    bufs = dict(x=_buf(4 * B * V * max(C, 1), offset=x_off), off=_buf(4 * (V + 1)), idx=_buf(4 * nnz), vals=_buf(4 * nnz),
                out=_buf(4 * B * V * max(C, 1), offset=out_off))
    a = {k: (None if k in null else v[1]) for k, v in bufs.items()}
    return lib.deftet_vertex_aggregate_f32(a["x"], a["off"], a["idx"], a["vals"], B, V, C, nnz, a["out"], None)


def test_header_ctypes_table_and_library_agree(lib):
    from deftet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"int\s+deftet_vertex_aggregate_f32\s*\(([^)]*)\)\s*;", code)
    assert m, "the header does not declare deftet_vertex_aggregate_f32"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float *x", "const int32_t *offsets", "const int32_t *idx", "const float *vals", "int n_batch",
                      "int n_vertex", "int n_channel", "int nnz", "float *out", "void *stream"]
    res, args = _lib.SIGNATURES["deftet_vertex_aggregate_f32"]
    want = [ctypes.c_int if p.startswith("int ") else ctypes.c_void_p for p in params]
    assert res is ctypes.c_int and args == want
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "deftet_vertex_aggregate_f32")
    assert lib.deftet_version() >= 300
    assert re.search(r"\b300: .*deftet_vertex_aggregate_f32", txt), "the header's version note is missing"


@pytest.mark.parametrize("bad", [dict(B=-1), dict(B=65536), dict(V=-1), dict(nnz=-1), dict(C=0), dict(C=-4), dict(null=("x",)),
                                 dict(null=("out",)), dict(null=("off",)), dict(null=("idx",)), dict(null=("vals",)), dict(x_off=2),
                                 dict(out_off=2), dict(B=0, C=0), dict(V=0, null=("off",))], ids=str)
def test_bad_arguments_are_refused_before_any_device_work(lib, bad):
    # the buffers are host memory and no device exists here: a call that got as far as a launch would not return EINVAL
    assert _call(lib, **bad) == EINVAL
    assert lib.deftet_last_error().decode(), "no message"


def test_empty_problems_launch_nothing(lib):
    # valid arguments with B·V == 0 return at once, also with the pointers an empty tensor has (null)
    assert _call(lib, B=0) == 0
    assert _call(lib, V=0, nnz=0) == 0
    assert _call(lib, B=0, null=("x", "out")) == 0
    assert _call(lib, V=0, nnz=0, null=("x", "out", "idx", "vals")) == 0


def test_python_front_ends_refuse_cpu_tensors():
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.hip_ops import VertexAdjacency, vertex_aggregate
    from deftet_amd.utils.matrix_utils import sparse_batch_matmul
    fake = VertexAdjacency.__new__(VertexAdjacency)
    with pytest.raises(DefTetHipError):
        vertex_aggregate(torch.zeros(1, 4, 8), fake)
    with pytest.raises(DefTetHipError):
        sparse_batch_matmul(fake, torch.zeros(1, 4, 8))
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.ones(2), (4, 4))
    with pytest.raises(DefTetHipError):
        sparse_batch_matmul(adj, torch.zeros(1, 4, 8))


def _clean_overlay_names():
    for k in [k for k in sys.modules if k.split(".")[0] in ("layers", "utils", "kaolin", "cv2")]:
        del sys.modules[k]


def test_overlay_registers_matrix_utils_only_when_asked():
    import deftet_amd.overlay as overlay
    import deftet_amd.utils.matrix_utils as ours
    saved = dict(sys.modules)
    _clean_overlay_names()
    try:
        names = overlay.install(kaolin=False)
        assert "utils.matrix_utils" not in names and "utils.matrix_utils" not in sys.modules
        overlay.uninstall(names)
        names = overlay.install(kaolin=False, graph_conv=True)
        assert "utils.matrix_utils" in names and set(overlay.L1_MODULES) <= set(names)
        mod = sys.modules["utils.matrix_utils"]
        assert mod is ours
        for name in ("convert_torch_sparse", "sparse_batch_matmul", "cross_dot_torch", "det_m", "MySparse"):
            assert hasattr(mod, name), name
        from deftet_amd.utils import tet_utils
        assert mod.convert_torch_sparse is tet_utils.convert_torch_sparse            # imported, not restated twice
        overlay.uninstall(names)
        assert "utils.matrix_utils" not in sys.modules
    finally:
        _clean_overlay_names()
        sys.modules.update({k: v for k, v in saved.items() if k not in sys.modules})


def test_my_sparse_round_trip():
    from deftet_amd.utils.matrix_utils import MySparse
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1, 3], [1, 0, 2]]), torch.tensor([0.5, 0.25, 2.0]), (4, 4))
    back = MySparse(adj).construct()
    assert back.is_sparse and tuple(back.shape) == (4, 4)
    assert torch.equal(back.to_dense(), adj.to_dense())


def test_det_and_cross_are_the_triple_product():
    from deftet_amd.utils.matrix_utils import cross_dot_torch, det_m
    rng = np.random.default_rng(7)
    m = rng.standard_normal((64, 3, 3))
    a, b, c = m[:, 0], m[:, 1], m[:, 2]
    cross = cross_dot_torch(torch.from_numpy(b), torch.from_numpy(c))
    assert cross.dtype == torch.float64
    np.testing.assert_allclose(cross.numpy(), np.cross(b, c), rtol=1e-12, atol=1e-14)
    det = det_m(torch.from_numpy(m))
    want = np.einsum("ni,ni->n", a, np.cross(b, c))
    np.testing.assert_allclose(det.numpy(), want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(det.numpy(), np.linalg.det(m), rtol=1e-9, atol=1e-12)


def test_ab_tool_check_mode_runs_without_a_gpu():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vertex_aggregate_ab.py"), "--check"], cwd=ROOT,
                       env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"check": "ok"' in r.stdout
