"""The winding-number entry points without a GPU: the header, the ctypes table and the library agree on the symbols, the workspace
size is the layout the entry point carves (one byte short is refused before any device call), bad arguments are refused by name in
C and in Python, and the depth chooser of the library is the one tests/winding_ref.py restates."""
import ctypes
import os
import re

import pytest
import torch

from tests import winding_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["deftet_winding_number_f32", "deftet_winding_number_workspace_bytes", "deftet_winding_number_levels",
           "deftet_winding_number_resolve_algo"]
EINVAL = -1
AUTO, EXACT, FAST, FAST_UNSORTED = 0, 1, 2, 3
P = ctypes.c_void_p(1 << 20)                                          # a non-null, 256-byte aligned pointer that is never followed


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


def _call(lib, B=2, V=100, F=300, N=1000, algo=FAST, beta=0.0, ws=P, ws_bytes=1 << 40, verts=P, faces=P, points=P, out=P, bad=P,
          v_off=None, f_off=None, n_rec=None):
    return lib.deftet_winding_number_f32(verts, v_off, faces, f_off, points, out, bad, B, V, B * F if n_rec is None else n_rec, F, N, algo,
                                         beta, ws, ws_bytes, None)


def test_header_ctypes_table_and_library_agree_on_the_symbols(lib):
    from deftet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    for name, value in (("AUTO", AUTO), ("EXACT", EXACT), ("FAST", FAST), ("FAST_UNSORTED", FAST_UNSORTED)):
        assert re.search(r"#define DEFTET_WN_%s %d\b" % (name, value), txt), name
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", txt))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 370


def test_depth_chooser_is_the_restated_one(lib):
    for F in list(range(0, 70)) + [223, 224, 255, 256, 1023, 1024, 4056, 4095, 4096, 99999, 1 << 20, (1 << 31) - 1]:
        assert lib.deftet_winding_number_levels(F) == T.levels(F), F
    assert lib.deftet_winding_number_levels(-5) == 0


def test_auto_resolves_to_one_of_the_two_paths(lib):
    r = lib.deftet_winding_number_resolve_algo
    assert [r(a, 4056, 1000) for a in (EXACT, FAST, FAST_UNSORTED)] == [EXACT, FAST, FAST_UNSORTED]
    # the measured sizes: 48 faces exact at either point count, 120 faces fast at 2 M points only, 224 up fast
    assert r(AUTO, 0, 1) == EXACT and r(AUTO, 12, 1 << 21) == EXACT
    assert [r(AUTO, F, 4096) for F in (48, 120, 224, 528, 960, 2208)] == [EXACT, EXACT, FAST, FAST, FAST, FAST]
    assert [r(AUTO, F, 8 * 257250) for F in (48, 120, 224, 528, 960, 2208, 4056, 101760)] == [EXACT, FAST, FAST, FAST, FAST, FAST, FAST, FAST]
    assert r(7, 10, 10) == EINVAL and r(-1, 10, 10) == EINVAL


@pytest.mark.parametrize("B,F,N", [(1, 1, 1), (3, 224, 4000), (8, 4056, 257250)])
def test_workspace_is_the_layout_and_one_byte_short_is_refused(lib, B, F, N):
    size = lib.deftet_winding_number_workspace_bytes
    want = {a: size(B, B * F, F, N, a) for a in (EXACT, FAST, FAST_UNSORTED)}
    assert all(w > 0 and w % 256 == 0 for w in want.values())
    assert want[EXACT] >= 48 * B * F and want[EXACT] < want[FAST_UNSORTED] < want[FAST]
    L = T.levels(F)
    assert want[FAST_UNSORTED] >= 96 * B * F + 32 * B * T.level_offset(L + 1) + 4 * B * (1 << (3 * L))    # records twice, nodes, leaf runs
    assert want[FAST] - want[FAST_UNSORTED] >= 12 * B * N                                               # the point sort: keys, sorted keys, order
    assert size(B, B * F, F, 2 * N + 4096, FAST) > want[FAST] and size(B, B * F, F, 2 * N + 4096, EXACT) == want[EXACT]
    assert size(B, B * F, F, N, AUTO) == want[lib.deftet_winding_number_resolve_algo(AUTO, F, B * N)]
    for a, w in want.items():
        assert _call(lib, B=B, F=F, N=N, algo=a, ws_bytes=w - 1) == EINVAL and b"workspace null, misaligned or too small: need %d bytes" % w in lib.deftet_last_error()
        assert _call(lib, B=B, F=F, N=N, algo=a, ws_bytes=w, verts=None) == EINVAL and b"null mesh" in lib.deftet_last_error()
        assert _call(lib, B=B, F=F, N=N, algo=a, ws_bytes=w, ws=None) == EINVAL and b"workspace" in lib.deftet_last_error()
        assert _call(lib, B=B, F=F, N=N, algo=a, ws_bytes=w, ws=ctypes.c_void_p(P.value + 16)) == EINVAL and b"misaligned" in lib.deftet_last_error()


def test_ragged_workspace_follows_the_largest_mesh(lib):
    size = lib.deftet_winding_number_workspace_bytes
    assert size(3, 5000, 4096, 100, FAST) > size(3, 5000, 4000, 100, FAST)        # L = 5 against L = 4: eight times the nodes
    assert size(3, 5000, 4000, 100, EXACT) == size(3, 5000, 100, 100, EXACT)


def test_bad_arguments_are_refused_by_name(lib):
    size = lib.deftet_winding_number_workspace_bytes
    assert size(0, 0, 0, 5, FAST) == 0 and size(2, -1, 3, 5, FAST) == 0 and size(2, 6, 3, -5, FAST) == 0 and size(2, 6, 3, 5, 4) == 0
    assert _call(lib, N=-1) == EINVAL and b"negative size" in lib.deftet_last_error()
    assert _call(lib, algo=4) == EINVAL and b"unknown algo" in lib.deftet_last_error()
    assert _call(lib, B=70000) == EINVAL and b"65535" in lib.deftet_last_error()
    assert _call(lib, f_off=P) == EINVAL and b"offsets come together" in lib.deftet_last_error()
    assert _call(lib, n_rec=7) == EINVAL and b"n_batch * n_face" in lib.deftet_last_error()
    for beta in (0.5, -3.0, float("nan"), 1e7):
        assert _call(lib, beta=beta) == EINVAL and b"beta" in lib.deftet_last_error(), beta
    assert _call(lib, points=None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert _call(lib, out=None) == EINVAL and _call(lib, bad=None) == EINVAL
    # nothing to do: accepted without a device call
    assert _call(lib, B=0) == 0 and _call(lib, N=0) == 0


def test_front_end_refuses_cpu_tensors_and_bad_arguments():
    from deftet_amd import dataprep, hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    v, f, p = torch.zeros(1, 4, 3), torch.zeros(2, 3, dtype=torch.long), torch.zeros(1, 5, 3)
    for call in (lambda: hip_ops.winding_number(v, f, p), lambda: hip_ops.winding_number_ragged([v[0]], [f], p)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="sign"):
        dataprep.mesh_to_sdf(v, f, p, sign="rays")
    with pytest.raises(ValueError, match="method"):
        DefTet().check_tet_inside_sdfs(torch.zeros(1, 2, 4, 3), [[v[0]], [[f]]], method="rays")
    w = torch.tensor([-1.2, -0.9, -0.4, 0.0, 0.4, 0.6, 1.0, 1.6, 2.0, 2.4, 2.6])
    assert hip_ops.winding_inside(w).tolist() == [False, False, False, False, False, True, True, True, True, True, True]
    assert hip_ops.winding_inside(w, "parity").tolist() == [True, True, False, False, False, True, True, False, False, False, True]
    with pytest.raises(ValueError, match="rule"):
        hip_ops.winding_inside(w, "majority")
    assert "no backward" in hip_ops.winding_number.__doc__
