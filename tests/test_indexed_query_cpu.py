"""The indexed occupancy query's argument checks, without a GPU: the C entry points reject bad sizes, batches and alignment
with DEFTET_EINVAL and a message before anything touches a device; the Python wrappers refuse CPU tensors; the A/B tool's
argument parsing runs up to its first GPU call."""
import ctypes
import os
import subprocess
import sys

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


def _fwd(lib, B=2, V=8, T=4, Q=5, idx_batch=1, idx_off=0):
    keep, pos = _buf(4 * 3 * max(B * V, 1))
    keep2, idx = _buf(16 * max(idx_batch * T, 1), offset=idx_off)
    keep3, pts = _buf(12 * max(B * Q, 1))
    keep4, cond = _buf(4 * max(B * Q, 1))
    keep5, ws = _buf(1 << 16)
    return lib.deftet_point_in_tet_indexed_f32(pos, idx, idx_batch, pts, cond, None, None, None, None, B, V, T, Q, 0, None, None, None,
                                               None, None, ws, 1 << 16, None)


def _scan(lib, B=2, V=8, T=4, Q=5, idx_batch=1, idx_off=0):
    keep, pos = _buf(4 * 3 * max(B * V, 1))
    keep2, idx = _buf(16 * max(idx_batch * T, 1), offset=idx_off)
    keep3, pts = _buf(12 * max(B * Q, 1))
    keep4, cond = _buf(4 * max(B * Q, 1))
    keep5, ws = _buf(1 << 16)
    return lib.deftet_point_in_tet_indexed_scan_f32(pos, idx, idx_batch, pts, cond, None, None, None, None, B, V, T, Q, 0, None, None, ws,
                                                    1 << 16, None)


def _bwd(lib, B=2, V=8, T=4, Q=5, idx_batch=1, idx_off=0):
    keep, pos = _buf(4 * 3 * max(B * V, 1))
    keep2, idx = _buf(16 * max(idx_batch * T, 1), offset=idx_off)
    keep3, pts = _buf(12 * max(B * Q, 1))
    keep4, cond = _buf(4 * max(B * Q, 1))
    keep5, gw = _buf(16 * max(B * Q, 1))
    keep6, off = _buf(4 * (idx_batch * V + 1))
    keep7, slots = _buf(16 * max(idx_batch * T, 1))
    keep8, gpos = _buf(12 * max(B * V, 1))
    keep9, ws = _buf(1 << 16)
    return lib.deftet_point_in_tet_indexed_bwd_to_vertices_f32(pos, idx, idx_batch, pts, cond, gw, None, None, off, slots, gpos, None, None,
                                                               B, V, T, Q, 0, ws, 1 << 16, None)


@pytest.mark.parametrize("call", [_fwd, _scan, _bwd])
@pytest.mark.parametrize("bad", [dict(B=-1), dict(V=-1), dict(T=-2), dict(idx_batch=3), dict(idx_batch=0), dict(idx_off=4)])
def test_entry_points_reject_bad_arguments(lib, call, bad):
    assert call(lib, **bad) == EINVAL
    msg = lib.deftet_last_error().decode()
    assert msg, "no message"


def test_version_and_symbols(lib):
    assert lib.deftet_version() >= 230
    for name in ("deftet_point_in_tet_indexed_f32", "deftet_point_in_tet_indexed_scan_f32",
                 "deftet_point_in_tet_indexed_bwd_to_vertices_f32"):
        assert hasattr(lib, name)


def test_python_wrappers_refuse_cpu_tensors():
    from deftet_amd import hip_ops
    from deftet_amd._lib import DefTetHipError
    pos = torch.zeros(1, 8, 3)
    idx = torch.zeros(2, 4, dtype=torch.int64)
    pts = torch.zeros(1, 5, 3)
    with pytest.raises(DefTetHipError):
        hip_ops.point_in_tet_indexed(pos, idx, pts)
    with pytest.raises(DefTetHipError):
        hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, idx, pts, torch.zeros(1, 5, 1), torch.zeros(1, 5, 4),
                                                     (torch.zeros(9, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), 1))


def test_ab_tool_check_mode_runs_without_a_gpu():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "occupancy_indexed_ab.py"), "--check"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
