"""The fused rasterize-and-composite operator's argument checks, without a GPU: the C entry points reject bad sizes, a feature
width too small for the depth flag, an unknown policy, null pointers, misalignment and an undersized workspace with
DEFTET_EINVAL and a message before anything touches a device; the Python wrapper refuses CPU tensors; render_mesh_color refuses
fused=True with a custom rasterizer; the A/B tool's argument parsing and input generation run up to its first GPU call."""
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


def _fwd(lib, B=1, P=4, F=2, D=4, knum=3, policy=0, depth=0, null=None, xy_off=0, ws_off=0, wsb=WS):
    bufs = dict(pix=_buf(8 * B * P), rng=_buf(8 * B * P), fz=_buf(12 * B * F), fxy=_buf(24 * B * F, offset=xy_off),
                feat=_buf(12 * D * B * F), col=_buf(4 * B * P * max(D, 1)), cov=_buf(4 * B * P), dep=_buf(4 * B * P),
                face=_buf(4 * B * P * max(knum, 1)), ws=_buf(WS, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_sparse_render_composite_fwd_f32(a["pix"], a["rng"], a["fz"], a["fxy"], a["feat"], B, P, F, D, knum, 1e-8,
                                                      policy, depth, 1.0, -6.0, a["col"], a["cov"], a["dep"], a["face"], a["ws"],
                                                      wsb, None)


def _bwd(lib, B=1, P=4, F=2, D=4, knum=3, policy=0, depth=0, null=None, xy_off=0, ws_off=0, wsb=WS):
    bufs = dict(pix=_buf(8 * B * P), fxy=_buf(24 * B * F, offset=xy_off), feat=_buf(12 * D * B * F), face=_buf(4 * B * P * max(knum, 1)),
                gcol=_buf(4 * B * P * max(D, 1)), gcov=_buf(4 * B * P), gdep=_buf(4 * B * P), gxy=_buf(24 * B * F),
                gfeat=_buf(12 * D * B * F), ws=_buf(WS, offset=ws_off))
    a = {k: (None if k == null else v[1]) for k, v in bufs.items()}
    return lib.deftet_sparse_render_composite_bwd_f32(a["pix"], a["fxy"], a["feat"], a["face"], a["gcol"], a["gcov"], a["gdep"], B, P, F,
                                                      D, knum, 1e-8, depth, 1.0, -6.0, a["gxy"], a["gfeat"], a["ws"], wsb, None)


BAD_BOTH = [dict(B=-1), dict(P=-1), dict(F=-2), dict(knum=-1), dict(D=-1), dict(D=1), dict(D=2, depth=1), dict(null="fxy"),
            dict(null="feat"), dict(null="pix"), dict(null="face"), dict(xy_off=4),
            dict(ws_off=64), dict(null="ws"), dict(wsb=256)]


@pytest.mark.parametrize("bad", BAD_BOTH + [dict(policy=2), dict(policy=-1), dict(null="rng"), dict(null="col"), dict(null="cov"),
                                            dict(null="dep", depth=1)], ids=str)
def test_forward_rejects_bad_arguments(lib, bad):
    assert _fwd(lib, **bad) == EINVAL
    assert lib.deftet_last_error().decode(), "no message"


@pytest.mark.parametrize("bad", BAD_BOTH + [dict(null="gxy"), dict(null="gfeat")], ids=str)
def test_backward_rejects_bad_arguments(lib, bad):
    assert _bwd(lib, **bad) == EINVAL
    assert lib.deftet_last_error().decode(), "no message"


def test_workspace_sizes_and_version(lib):
    assert lib.deftet_version() >= 240
    assert lib.deftet_sparse_render_composite_workspace_bytes(1, 64, 10, 4, 8) > 0
    # the backward keeps one batch entry's P * knum * D layer gradients in its workspace, on top of the hit sort
    assert (lib.deftet_sparse_render_composite_bwd_workspace_bytes(1, 64, 10, 4, 8)
            >= 64 * 8 * 4 * 4 + lib.deftet_sparse_render_bwd_workspace_bytes(1, 64, 10, 8))
    assert lib.deftet_sparse_render_composite_workspace_bytes(1, -1, 10, 4, 8) == 0


def test_python_wrapper_refuses_cpu_tensors():
    from deftet_amd._lib import DefTetHipError
    from deftet_amd.render import deftet_sparse_render_composite
    with pytest.raises(DefTetHipError):
        deftet_sparse_render_composite(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), torch.zeros(1, 2, 3), torch.zeros(1, 2, 3, 2),
                                       torch.zeros(1, 2, 3, 4), knum=3)


def test_render_mesh_color_refuses_fused_with_a_rasterizer():
    from deftet_amd.render import render_mesh_color
    with pytest.raises(ValueError):
        render_mesh_color(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), torch.zeros(1, 3, 3), torch.zeros(1, 3, 2),
                          torch.zeros(1, 3, 4), torch.zeros(1, 3, dtype=torch.int64), knum=3, rasterizer=lambda *a: None, fused=True)


def test_ab_tool_check_mode_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_composite_ab.py"), "--check"], cwd=ROOT,
                       env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
