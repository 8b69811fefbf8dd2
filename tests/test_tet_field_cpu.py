"""CPU tests of per-vertex field sampling at query points: the order logic of the fp32 restatements of
tests/tet_field_ref.py, their distance from the fp64 chain on the GPU tests' own inputs, the four symbols of the C ABI, its
workspace size and its argument checks (all refused by name before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from deftet_amd import grids
from tests import tet_field_ref as ref
from tests.tol import check_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5
EINVAL = -1
SYMBOLS = ["deftet_tet_field_sample_fwd_f32", "deftet_tet_field_sample_bwd_w_f32", "deftet_tet_field_sample_bwd_field_f32",
           "deftet_tet_field_sample_workspace_bytes"]

_raw = ctypes.create_string_buffer(1 << 12)
P = ctypes.c_void_p((ctypes.addressof(_raw) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib, build
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------- the restatements
def test_grad_field_restatement_equals_a_dense_sum_on_integers():
    """integer-valued weights and gradients: every partial sum is exact, so any order gives the same bits, and the ordered walk
    over incidences and per-tet query lists must find every (query, corner) term exactly once"""
    g = np.random.default_rng(0)
    for B, per_shape in ((1, False), (3, False), (3, True)):
        pos, tets = ref.mesh(4, B, per_shape)
        V, T, Q, C = pos.shape[1], tets.shape[-2], 400, 3
        cond = g.integers(-1, T, (B, Q, 1)).astype(np.float32)
        bary = g.integers(-8, 9, (B, Q, 4)).astype(np.float32)
        gout = g.integers(-8, 9, (B, Q, C)).astype(np.float32)
        got = ref.grad_field(gout, cond, bary, tets, V)
        want = ref.grad_field_dense(gout, cond, bary, tets, V)
        assert got.dtype == np.float32 and (cond == -1).any() and np.abs(want).max() > 50
        assert np.array_equal(got.astype(np.float64), want)
        base = g.integers(-8, 9, (B, V, C)).astype(np.float32)
        assert np.array_equal(ref.grad_field(gout, cond, bary, tets, V, base=base), base + got)
    # a tet that lists a vertex twice counts twice
    tets = np.array([[0, 1, 1, 2]])
    got = ref.grad_field(np.ones((1, 1, 1), np.float32), np.zeros((1, 1, 1), np.float32), np.array([[[1, 2, 4, 8]]], np.float32), tets, 4)
    assert got.reshape(-1).tolist() == [1, 6, 8, 0]


@pytest.mark.parametrize("R,B,C", [(6, 1, 1), (6, 1, 4), (4, 3, 4), (4, 3, 33)])
def test_fp32_restatements_lie_within_the_bound_of_the_fp64_chain(R, B, C):
    """the GPU tests' meshes, queries, fields and output gradients, located here by brute force: values, grad_w and grad_field in
    the library's fp32 orders against fp64 autograd"""
    Q = 1000
    pos, tets = ref.mesh(R, B)
    V = pos.shape[1]
    pts = grids.random_queries(B, Q)
    cond, bary = ref.cpu_location(pos, tets, pts)
    miss = float((cond < 0).mean())
    assert 0.05 < miss < 0.25, miss                                    # random_queries reaches past the grid: about 14 % miss
    field, gout = ref.field_of(B, V, C), ref.gout_of(B, Q, C)
    f64 = torch.from_numpy(field).double().requires_grad_(True)
    p64 = torch.from_numpy(pos).double()
    want = ref.chain64(f64, p64, torch.from_numpy(pts).double(), tets, cond)
    want.backward(torch.from_numpy(gout).double())
    check_close("tfs.cpu.R%d.B%d.C%d.values" % (R, B, C), ref.values(field, tets, cond, bary), want, BOUND)
    check_close("tfs.cpu.R%d.B%d.C%d.grad_field" % (R, B, C), ref.grad_field(gout, cond, bary, tets, V), f64.grad, BOUND)
    tt, t = ref.tets_of(tets, B), ref.located(cond)
    rows = np.stack([field[b].astype(np.float64)[tt[b][np.maximum(t[b], 0)]] for b in range(B)])              # [B,Q,4,C]
    gw64 = np.einsum("bqc,bqkc->bqk", gout.astype(np.float64), rows) * (t >= 0)[..., None]
    check_close("tfs.cpu.R%d.B%d.C%d.grad_w" % (R, B, C), ref.grad_w(field, tets, cond, gout), gw64, BOUND)


def test_restated_values_fill_misses_and_refuse_bad_indices():
    pos, tets = ref.mesh(4, 1)
    V = pos.shape[1]
    pts = grids.random_queries(1, 200)
    cond, bary = ref.cpu_location(pos, tets, pts)
    field = ref.field_of(1, V, 2)
    out = ref.values(field, tets, cond, bary, fill=-7.0)
    assert np.all(out[cond[..., 0] < 0] == -7.0) and np.all(bary[cond[..., 0] < 0] == 0)
    hit = int(np.nonzero(cond[0, :, 0] >= 0)[0][0])
    dirty = tets.copy()
    dirty[int(cond[0, hit, 0]), 2] = V
    out = ref.values(field, dirty, cond, bary)
    assert np.isnan(out[0, hit]).all() and np.isfinite(np.delete(out[0], np.nonzero(cond[0, :, 0] == cond[0, hit, 0])[0], 0)).all()
    assert np.all(ref.grad_w(field, dirty, cond, np.ones((1, 200, 2), np.float32))[0, hit] == 0)


# ---------------------------------------------------------------------------- the C ABI
def test_header_ctypes_table_and_library_agree_on_the_four_symbols(lib):
    from deftet_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deftet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", txt))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 340


def align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("B,T,Q", [(1, 162, 1000), (3, 48, 1), (8, 257250, 100000)])
def test_workspace_is_the_total_of_the_layout(lib, B, T, Q):
    """keys, sorted keys, the radix sort's own scratch, the queries in (shape, tet) order, seg[B (T + 1) + 1]: each on its own
    256-byte line"""
    size = lib.deftet_tet_field_sample_workspace_bytes
    n = B * Q
    want = 3 * align(4 * n) + align(lib.deftet_radix_sort_workspace_bytes(n, 4, 4)) + align(4 * (B * (T + 1) + 1))
    got = size(B, T, Q)
    assert got > 0 and got % 256 == 0 and got == want
    assert size(B, T, 4 * Q + 256) > got and size(B, 2 * T + 256, Q) > got and size(B + 1, T + 64, Q + 64) > got
    # the entry point carves with the same layout: one byte short is refused, the exact size passes on to the pointer checks
    args = lambda nbytes: (P, P, P, None, P, P, B, 50, T, 1, Q, 4, 0, P, nbytes, None)
    assert lib.deftet_tet_field_sample_bwd_field_f32(*args(got - 1)) == EINVAL and b"workspace" in lib.deftet_last_error()
    assert lib.deftet_tet_field_sample_bwd_field_f32(*args(got)) == EINVAL and b"null pointer" in lib.deftet_last_error()


def test_bad_arguments_are_refused_by_name(lib):
    fwd, bw, bf = lib.deftet_tet_field_sample_fwd_f32, lib.deftet_tet_field_sample_bwd_w_f32, lib.deftet_tet_field_sample_bwd_field_f32
    # a field without a channel, a negative size, a tet list batch that is neither 1 nor B
    for C, V, Bi, msg in ((0, 10, 1, b"at least one channel"), (4, -1, 1, b"negative size"), (4, 10, 2, b"batch must be 1 or")):
        assert fwd(P, P, P, P, P, None, 0.0, 3, V, 20, Bi, 5, C, None) == EINVAL and msg in lib.deftet_last_error()
        assert b"tet_field_sample:" in lib.deftet_last_error()
        assert bw(P, P, P, P, P, 3, V, 20, Bi, 5, C, None) == EINVAL and msg in lib.deftet_last_error()
        assert b"tet_field_sample_bwd_w:" in lib.deftet_last_error()
        assert bf(P, P, P, P, P, P, 3, V, 20, Bi, 5, C, 0, P, 1 << 30, None) == EINVAL and msg in lib.deftet_last_error()
        assert b"tet_field_sample_bwd_field:" in lib.deftet_last_error()
    # null and misaligned pointers
    assert fwd(P, P, None, P, P, None, 0.0, 1, 10, 20, 1, 5, 4, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    off = ctypes.c_void_p(P.value + 4)
    assert fwd(P, off, P, P, P, None, 0.0, 1, 10, 20, 1, 5, 4, None) == EINVAL and b"16-byte aligned" in lib.deftet_last_error()
    assert fwd(P, P, P, off, P, None, 0.0, 1, 10, 20, 1, 5, 4, None) == EINVAL and b"16-byte aligned" in lib.deftet_last_error()
    assert bw(P, off, P, P, P, 1, 10, 20, 1, 5, 4, None) == EINVAL and b"16-byte aligned" in lib.deftet_last_error()
    assert bw(P, P, P, None, P, 1, 10, 20, 1, 5, 4, None) == EINVAL and b"null pointer" in lib.deftet_last_error()
    # the workspace: missing, one byte short, misaligned
    need = lib.deftet_tet_field_sample_workspace_bytes(1, 20, 5)
    for ws, nbytes in ((None, need), (P, need - 1), (ctypes.c_void_p(P.value + 16), need)):
        assert bf(P, P, P, P, P, P, 1, 10, 20, 1, 5, 4, 0, ws, nbytes, None) == EINVAL
        assert b"workspace null, misaligned or too small: need %d bytes" % need in lib.deftet_last_error()
    # sizes past what the indices hold
    assert fwd(P, P, P, P, P, None, 0.0, 1, 10, 1 << 24, 1, 5, 4, None) == -4 and b"2^24" in lib.deftet_last_error()
    assert fwd(P, P, P, P, P, None, 0.0, 70000, 10, 20, 1, 5, 4, None) == -4 and b"65535" in lib.deftet_last_error()
    # nothing to do is not an error: no shape, or no query (the empty result is the caller's)
    assert fwd(None, None, None, None, None, None, 0.0, 0, 10, 20, 1, 5, 4, None) == 0
    assert fwd(None, None, None, None, None, None, 0.0, 2, 10, 20, 1, 0, 4, None) == 0
    assert bw(None, None, None, None, None, 2, 10, 20, 1, 0, 4, None) == 0
    assert lib.deftet_tet_field_sample_workspace_bytes(-1, 20, 5) == 0


def test_front_end_refuses_cpu_tensors():
    from deftet_amd import hip_ops
    field, pos, tets, pts = torch.zeros(1, 5, 2), torch.zeros(1, 5, 3), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(1, 7, 3)
    with pytest.raises(RuntimeError):
        hip_ops.tet_field_sample(field, pos, tets, pts)
    for name in ("tet_field_sample_fwd", "tet_field_sample_bwd_w", "tet_field_sample_bwd_field"):
        assert callable(getattr(hip_ops, name))
