"""CPU tests of tet-centroid feature sampling: the C ABI carries the four symbols and refuses bad arguments by
name before any device call, the workspace size is the layout's own total, and the restatements of tests/tet_centroid_ref.py
agree with the reference's literal decode_occ composition and with fp64 autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tet_centroid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5
EINVAL = -1
SYMBOLS = ["deftet_tet_centroid_sample_fwd_f32", "deftet_tet_centroid_sample_bwd_pos_f32", "deftet_tet_centroid_sample_bwd_vertices_f32",
           "deftet_tet_centroid_sample_workspace_bytes"]

_raw = ctypes.create_string_buffer(1 << 12)
P = ctypes.c_void_p((ctypes.addressof(_raw) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def ptrs(n):
    return (ctypes.c_void_p * max(n, 1))(*([P.value] * n))


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib, build
    build.build()
    return _lib.load()


def test_header_ctypes_table_and_library_agree_on_the_four_symbols(lib):
    from deftet_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deftet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", txt))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 330


def align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("T,K", [(1500, 257), (1500, 1), (300, 600), (257250, 10000)])
def test_workspace_is_the_total_of_the_layout(lib, T, K):
    """keys, sorted keys, the radix sort's own scratch, the slots in tet order, seg[T + 1]: each on its own 256-byte line"""
    size = lib.deftet_tet_centroid_sample_workspace_bytes
    want = 3 * align(4 * K) + align(lib.deftet_radix_sort_workspace_bytes(K, 4, 4)) + align(4 * (T + 1))
    got = size(8, T, K)
    assert got > 0 and got % 256 == 0 and got == want
    assert size(8, T, 4 * K + 256) > got and size(8, 2 * T + 256, K) > got and size(1, T, K) == got      # grows with K and with T
    # the entry point carves with the same layout: one byte short is refused, the exact size passes on to the pointer checks
    args = lambda nbytes: (P, None, P, P, 0, P, 1, 50, T, 1, K, 0, P, nbytes, None)
    assert lib.deftet_tet_centroid_sample_bwd_vertices_f32(*args(got - 1)) == EINVAL and b"workspace" in lib.deftet_last_error()
    assert lib.deftet_tet_centroid_sample_bwd_vertices_f32(*args(got)) == EINVAL and b"null pointer" in lib.deftet_last_error()


def test_bad_arguments_are_refused_by_name(lib):
    fwd, bpos, bvert = (lib.deftet_tet_centroid_sample_fwd_f32, lib.deftet_tet_centroid_sample_bwd_pos_f32,
                        lib.deftet_tet_centroid_sample_bwd_vertices_f32)
    c9, r9 = ints(*[1] * 9), ints(*[4] * 9)
    # the number of volumes outside [0, 8]
    for n in (-1, 9):
        assert fwd(ptrs(9), c9, r9, n, None, None, None, 0, None, None, None, 1, 10, 20, 1, 5, 1, None) == EINVAL
        assert b"between 0 and 8 volumes" in lib.deftet_last_error()
        assert bpos(ptrs(9), c9, r9, n, None, None, None, 1, 5, 1, None) == EINVAL and b"between 0 and 8 volumes" in lib.deftet_last_error()
    # a resolution below 1
    assert fwd(ptrs(2), ints(3, 2), ints(8, 0), 2, None, None, None, 0, None, None, None, 1, 10, 20, 1, 5, 1, None) == EINVAL
    assert b"resolution below 1" in lib.deftet_last_error()
    assert bpos(ptrs(2), ints(3, 2), ints(8, 0), 2, None, None, None, 1, 5, 1, None) == EINVAL and b"resolution below 1" in lib.deftet_last_error()
    # a range past the end of the tet list, without a selection
    assert fwd(ptrs(1), ints(3), ints(8), 1, None, None, None, 16, None, None, None, 1, 10, 20, 1, 5, 1, None) == EINVAL
    assert b"exceeds the 20 tets" in lib.deftet_last_error()
    assert bvert(None, None, None, None, 16, None, 1, 10, 20, 1, 5, 0, None, 0, None) == EINVAL and b"exceeds the 20 tets" in lib.deftet_last_error()
    assert fwd(ptrs(1), ints(3), ints(8), 1, None, None, None, -1, None, None, None, 1, 10, 20, 1, 5, 1, None) == EINVAL
    # the workspace: missing, one byte short, misaligned
    need = lib.deftet_tet_centroid_sample_workspace_bytes(1, 20, 5)
    for ws, nbytes in ((None, need), (P, need - 1), (ctypes.c_void_p(P.value + 16), need)):
        assert bvert(P, P, P, P, 0, P, 1, 10, 20, 1, 5, 0, ws, nbytes, None) == EINVAL
        assert b"workspace null, misaligned or too small: need %d bytes" % need in lib.deftet_last_error()
    # null pointers and a tet list batch that is neither 1 nor B
    assert fwd(ptrs(1), ints(3), ints(8), 1, None, None, None, 0, None, None, None, 1, 10, 20, 1, 5, 1, None) == EINVAL
    assert b"null" in lib.deftet_last_error()
    assert fwd(ptrs(1), ints(3), ints(8), 1, P, P, None, 0, P, P, None, 3, 10, 20, 2, 5, 1, None) == EINVAL and b"batch must be 1 or" in lib.deftet_last_error()
    # nothing to do is not an error: no shape, or no slot (the empty result is the caller's)
    assert fwd(None, None, None, 0, None, None, None, 0, None, None, None, 0, 10, 20, 1, 5, 1, None) == 0
    assert fwd(ptrs(1), ints(3), ints(8), 1, None, None, None, 0, None, None, None, 2, 10, 20, 1, 0, 1, None) == 0
    assert bpos(None, None, None, 0, None, None, None, 2, 0, 1, None) == 0


def test_front_end_refuses_cpu_tensors():
    from deftet_amd import hip_ops, pointvoxel
    vol, pos, tets = torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 5, 3), torch.zeros(3, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        hip_ops.tet_centroid_sample([vol], pos, tets)
    with pytest.raises(RuntimeError):
        pointvoxel.decode_occ_features(pos, tets[None], [vol])


def _small_case(seed=0, B=2, V=50, T=120, K=40, lattice=False):
    g = torch.Generator().manual_seed(seed)
    vols = [torch.randn(B, c, r, r, r, generator=g) for c, r in ((5, 32), (3, 16), (4, 8))]
    pos = ref.lattice_vertices(B, V, seed + 1) if lattice else ref.uniform_vertices(B, V, seed + 1)
    tets = torch.from_numpy(ref.random_tets(T, V, seed + 2))
    select = torch.randperm(T, generator=g)[:K]
    return vols, pos, tets, select


def test_fp64_restatement_agrees_with_the_literal_decode_occ_composition():
    """gather, mean, gather of center_idx, sample_f (grid_sample), cat in fp32 against restatement (a): 2.7e-6 measured"""
    vols, pos, tets, select = _small_case()
    want = ref.occ_feature(vols, pos, tets, select=select)
    got = ref.decode_occ_composition(pos, tets[None].expand(2, -1, -1), vols, center_idx=select)
    assert got.shape == want.shape == (2, 15, 40)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("literal decode_occ composition against the fp64 restatement: max-norm error %.3g" % err)
    assert err <= BOUND
    # and the range form against the same composition on a slice of the tet list
    want = ref.occ_feature(vols, pos, tets, first=37, count=50)
    got = ref.decode_occ_composition(pos, tets[None, 37:87].expand(2, -1, -1), vols)
    assert float((got.double() - want).abs().max() / want.abs().max()) <= BOUND


def test_fp32_centroid_restatement_is_the_rounded_mean():
    vols, pos, tets, select = _small_case(3)
    got = ref.centroids(pos, tets, select=select)
    want = ref.centroids64(pos, tets, select=select)
    assert got.dtype == np.float32 and got.shape == (2, 40, 3)
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()
    per_shape = tets[None].expand(2, -1, -1).contiguous()
    assert np.array_equal(ref.centroids(pos, per_shape, select=select), got)
    assert np.array_equal(ref.centroids(pos, tets, first=5, count=7), ref.centroids(pos, tets, select=torch.arange(5, 12)))


@pytest.mark.parametrize("mode", ["select", "repeats", "range"])
def test_vertex_reduction_restatement_agrees_with_fp64_autograd(mode):
    """(b) against the backward of mean + index in fp64: the reduction is linear, so any gcent serves"""
    B, V, T = 2, 50, 120
    tets = ref.random_tets(T, V, 7)
    g = np.random.default_rng(8)
    if mode == "range":
        select, first, K = None, 11, 60
        chosen = np.arange(first, first + K)
    else:
        first = 0
        chosen = g.permutation(T)[:40]
        if mode == "repeats":
            chosen = g.permutation(np.concatenate([chosen, chosen, chosen]))
        select, K = chosen, len(chosen)
    gcent = g.standard_normal((B, K, 3)).astype(np.float32)
    got = ref.vertex_reduction(gcent, tets, V, select=select, first=first)
    pos = torch.zeros(B, V, 3, dtype=torch.float64, requires_grad=True)
    pos[:, torch.from_numpy(tets)].mean(2)[:, torch.from_numpy(chosen)].backward(torch.from_numpy(gcent).double())
    want = pos.grad.numpy()
    assert got.dtype == np.float32 and np.abs(got - want).max() / np.abs(want).max() <= BOUND
    untouched = np.setdiff1d(np.arange(V), tets[chosen].reshape(-1))
    assert np.all(got[:, untouched] == 0.0)
    base = g.standard_normal((B, V, 3)).astype(np.float32)
    assert np.array_equal(ref.vertex_reduction(gcent, tets, V, select=select, first=first, base=base), base + got)


def test_lattice_vertices_keep_their_margin():
    """the inputs on which the GPU test checks the position gradient: no chosen centroid within 0.01 of an integer voxel
    coordinate, all strictly inside (0, R - 1), at the three resolutions"""
    for seed in range(20):
        pos = ref.lattice_vertices(3, 300, seed)
        cent = ref.centroids64(pos, ref.random_tets(1500, 300, seed + 100))
        for R, least in ((32, 0.05), (16, 0.025), (8, 0.0125)):
            margin, inside = ref.lattice_margin(cent, R)
            assert inside and margin >= 0.01 and margin >= least - 1e-4, (seed, R, margin)
