"""The vertex Laplacian's argument checks, without a GPU: the adjacency build and the forward / backward entry points reject bad
sizes, C outside 1..16, an unknown order, weighting or reduction, null pointers, misalignment and an undersized workspace with
DEFTET_EINVAL and a message before anything touches a device; the Python wrappers refuse CPU tensors; the A/B tool's argument
parsing and input generation run up to its first GPU call."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
WS = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


def _buf(nbytes, align=256, offset=0):
    raw = ctypes.create_string_buffer(nbytes + align * 2)
    base = (ctypes.addressof(raw) + align - 1) // align * align + offset
    return raw, ctypes.c_void_p(base)


def _adj(lib, nnz=6, V=4, ib=8, order=0, null=None, rows_off=0, out_off=0, ws_off=0, wsb=WS):
    bufs = dict(rows=_buf(8 * nnz, offset=rows_off), cols=_buf(8 * nnz), vals=_buf(4 * nnz), off=_buf(4 * (V + 1), offset=out_off),
                ocols=_buf(4 * nnz), ovals=_buf(4 * nnz), toff=_buf(4 * (V + 1)), trows=_buf(4 * nnz), tvals=_buf(4 * nnz),
                bad=_buf(4), ws=_buf(WS, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_vertex_adjacency_csr_i32(a["rows"], a["cols"], ib, a["vals"], nnz, V, order, a["off"], a["ocols"], a["ovals"],
                                               a["toff"], a["trows"], a["tvals"], a["bad"], a["ws"], wsb, None)


def _fwd(lib, B=2, V=4, C=3, nnz=6, weighting=0, reduction=1, null=None, x_off=0, ws_off=0, wsb=WS):
    bufs = dict(x=_buf(4 * B * V * C, offset=x_off), off=_buf(4 * (V + 1)), cols=_buf(4 * nnz), vals=_buf(4 * nnz), w=_buf(4 * V),
                r=_buf(4 * B * V * C), out=_buf(4 * B * V * C), ws=_buf(WS, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_vertex_laplacian_fwd_f32(a["x"], a["off"], a["cols"], a["vals"], a["w"], weighting, reduction, B, V, C, nnz,
                                               a["r"], a["out"], a["ws"], wsb, None)


def _bwd(lib, B=2, V=4, C=3, nnz=6, weighting=0, reduction=1, null=None, x_off=0):
    bufs = dict(r=_buf(4 * B * V * C, offset=x_off), g=_buf(4 * B * V * C), toff=_buf(4 * (V + 1)), trows=_buf(4 * nnz),
                tvals=_buf(4 * nnz), w=_buf(4 * V), dx=_buf(4 * B * V * C))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_vertex_laplacian_bwd_f32(a["r"], a["g"], a["toff"], a["trows"], a["tvals"], a["w"], weighting, reduction, B, V,
                                               C, nnz, a["dx"], None)


@pytest.mark.parametrize("bad", [dict(nnz=-1), dict(V=-1), dict(ib=2), dict(ib=0), dict(order=2), dict(order=-1), dict(null="rows"),
                                 dict(null="cols"), dict(null="off"), dict(null="toff"), dict(null="ocols"), dict(null="trows"),
                                 dict(null="bad"), dict(rows_off=4), dict(out_off=2), dict(null="ws"), dict(ws_off=64), dict(wsb=256)],
                         ids=str)
def test_adjacency_rejects_bad_arguments(lib, bad):
    assert _adj(lib, **bad) == EINVAL
    assert lib.deftet_last_error().decode(), "no message"


BAD_BOTH = [dict(B=-1), dict(B=65536), dict(V=-1), dict(nnz=-1), dict(C=0), dict(C=17), dict(weighting=2), dict(weighting=-1),
            dict(reduction=2), dict(reduction=-1), dict(null="cols"), dict(null="vals"), dict(null="w", weighting=1), dict(x_off=2)]


@pytest.mark.parametrize("bad", BAD_BOTH + [dict(null="off"), dict(null="x"), dict(null="r"), dict(null="out"), dict(null="ws"),
                                            dict(ws_off=64), dict(wsb=0)], ids=str)
def test_forward_rejects_bad_arguments(lib, bad):
    assert _fwd(lib, **bad) == EINVAL
    assert lib.deftet_last_error().decode(), "no message"


@pytest.mark.parametrize("bad", BAD_BOTH + [dict(null="toff"), dict(null="trows"), dict(null="tvals"), dict(null="r"), dict(null="g"),
                                            dict(null="dx")], ids=str)
def test_backward_rejects_bad_arguments(lib, bad):
    if "null" in bad and bad["null"] in ("cols", "vals"):
        bad = dict(bad, null={"cols": "trows", "vals": "tvals"}[bad["null"]])
    if "null" in bad and bad["null"] == "x":
        bad = dict(bad, null="r")
    assert _bwd(lib, **{k: v for k, v in bad.items() if k not in ("ws_off", "wsb")}) == EINVAL
    assert lib.deftet_last_error().decode(), "no message"


def test_version_and_workspace_sizes(lib):
    assert lib.deftet_version() >= 250
    assert lib.deftet_vertex_adjacency_workspace_bytes(1000, 100) >= 1000 * (8 + 8 + 4)
    assert lib.deftet_vertex_adjacency_workspace_bytes(-1, 100) == 0
    # one partial per (shape, workgroup of 256 vertices), the grid rounded up to a multiple of 8 workgroups
    assert lib.deftet_vertex_laplacian_workspace_bytes(8, 46656) >= 8 * 184 * 4
    assert lib.deftet_vertex_laplacian_workspace_bytes(-1, 10) == 0


def test_none_reduction_needs_no_workspace_and_empty_batches_are_fine(lib):
    # valid arguments that launch nothing: B = 0 (the checks still run first)
    assert _fwd(lib, B=0, reduction=0, null="ws", wsb=0) == 0
    assert _bwd(lib, B=0) == 0
    assert _fwd(lib, B=0, C=17) == EINVAL


def test_python_wrappers_refuse_cpu_tensors():
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.hip_ops import VertexAdjacency, vertex_laplacian
    from deftet_amd.render import get_featlap
    tets = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32)
    with pytest.raises(DefTetHipError):
        VertexAdjacency.from_tets(tets, 4)
    with pytest.raises(DefTetHipError):
        VertexAdjacency.from_table(torch.zeros(4, 3, dtype=torch.int64), torch.ones(4, 1), index_base=1)
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.ones(2), (4, 4))
    with pytest.raises(DefTetHipError):
        VertexAdjacency.from_sparse(adj)
    fake = VertexAdjacency.__new__(VertexAdjacency)
    with pytest.raises(DefTetHipError):
        vertex_laplacian(torch.zeros(1, 4, 3), fake)
    with pytest.raises(DefTetHipError):
        get_featlap(torch.zeros(4, 3), fake)


def test_ab_tool_check_mode_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vertex_laplacian_ab.py"), "--check"], cwd=ROOT,
                       env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"check": "ok"' in r.stdout
