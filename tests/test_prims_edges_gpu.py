"""The device sort and scans (deftet_amd/csrc/prims.hpp) past every size switch and at the edges of their arguments: pass counts and
digit widths with the top key bit set, key patterns that load one digit or all of them, the column scan of the unfused pass at
every quarter layout and with a second batch of chunks, the device-side count at its clamps, values moved as bits, the entry
checks; scans around the one-workgroup switch, in place, with wrapping sums, identities in the data and step inputs.  Every
comparison is integer or bit equality against numpy on the host."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# restated from prims.hpp: 2,048 keys per tile; up to 512 tiles the scatter sums the digit table itself (fused), above that the
# table is scanned by columns in chunks of 64 tiles, four quarters of the chunks in one workgroup, 16 chunks per batch; scans of
# up to 8,192 elements run in one workgroup
TILE = 2048
FUSED_TILES = 512
SCAN_SMALL = 8192


def _unsigned(keys):
    return keys.view(np.uint32 if keys.dtype.itemsize == 4 else np.uint64)


def _order(keys, bits):
    """stable argsort of (keys as unsigned) & mask; the masked keys in the narrowest unsigned type (numpy radix-sorts 8 and 16 bits)"""
    u = _unsigned(keys)
    m = u & u.dtype.type((1 << bits) - 1)
    if bits <= 8:
        m = m.astype(np.uint8)
    elif bits <= 16:
        m = m.astype(np.uint16)
    return np.argsort(m, kind="stable")


def _bits_of(a):
    """integer view of an array (float values are compared as bit patterns)"""
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_sort(cuda, keys, vals, bits, order=None):
    from deftet_amd import hip_ops
    k = torch.from_numpy(keys).to(cuda)
    v = torch.from_numpy(vals).to(cuda) if vals is not None else None
    ko, vo = hip_ops.radix_sort(k, v, bits=bits)
    order = _order(keys, bits) if order is None else order
    assert np.array_equal(ko.cpu().numpy(), keys[order])
    assert np.array_equal(k.cpu().numpy(), keys)                                     # the inputs are not modified
    if vals is not None:
        assert np.array_equal(_bits_of(vo.cpu().numpy()), _bits_of(vals[order]))
        assert np.array_equal(_bits_of(v.cpu().numpy()), _bits_of(vals))
    else:
        assert vo is None


# ----------------------------------------------------------------------------------------- 1a. pass counts and digit widths
def _wide_keys(rng, n, kdt):
    """keys over the whole word with the top bit set in half of them (a negative key sorts as unsigned), long runs of equal low
    digits (random >> random) and bits above any requested width that must not count"""
    w = np.dtype(kdt).itemsize * 8
    r = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)   # 64 uniform bits
    if w == 32:
        r &= np.uint64(0xFFFFFFFF)
    u = (r >> rng.integers(0, w, n).astype(np.uint64)) ^ (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(w - 1))
    return u.astype(np.uint32 if w == 32 else np.uint64).view(kdt)


@pytest.mark.parametrize("with_values", [False, True])
@pytest.mark.parametrize("n", [65, 2049, 100_003])
@pytest.mark.parametrize("kdt,bits", [(np.int32, b) for b in (1, 7, 8, 16, 24, 32)] + [(np.int64, b) for b in (8, 32, 33, 56, 64)])
def test_sort_pass_counts_and_digit_widths(cuda, kdt, bits, n, with_values):
    """one pass (bits <= 8: the first pass writes the output), last digits of 1, 7 and 8 bits, odd and even pass counts, the full
    word: hip_ops.radix_sort hands negative keys through unchanged and they sort as their unsigned view"""
    rng = np.random.default_rng(1000 * bits + n)
    keys = _wide_keys(rng, n, kdt)
    if bits == np.dtype(kdt).itemsize * 8:
        neg = int((keys < 0).sum())
        assert n // 4 < neg < 3 * n // 4                                              # half the keys are negative
    _check_sort(cuda, keys, np.arange(n, dtype=np.int32) if with_values else None, bits)


# ----------------------------------------------------------------------------------------- 1b. key patterns
def _ramp(i, n):
    return i.astype(np.int64) * 65535 // max(n - 1, 1)


PATTERNS = {
    "all_equal": lambda i, n: np.full(n, 0x1234),                    # one digit owns whole tiles: ranks reach 2,047
    "ascending": _ramp,
    "descending": lambda i, n: 65535 - _ramp(i, n),
    "digit_is_lane": lambda i, n: i % 256,                           # every round of the match-any ballots sees 64 distinct digits
    "one_digit_per_round": lambda i, n: (i // 64) % 256,
    "last_pass_only": lambda i, n: (i % 2) << 15,
    "two_values_by_tile": lambda i, n: np.where((i // TILE) % 2 == 0, 0x01FF, 0x0200),
}


@pytest.mark.parametrize("n", [2048, 2049, 6000, 100_003])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_sort_key_patterns(cuda, pattern, n):
    i = np.arange(n)
    keys = np.asarray(PATTERNS[pattern](i, n)).astype(np.int32)
    assert keys.min() >= 0 and keys.max() < 65536
    _check_sort(cuda, keys, np.arange(n, dtype=np.int32), 16)


# ----------------------------------------------------------------------------------------- 1c. column scan of the unfused pass
# tiles -> chunks of 64 -> chunks per quarter: 576 -> 9 (3,3,3,0), 577 -> 10 (3,3,3,1), 641 -> 11 (3,3,3,2), 769 -> 13 (4,4,4,1),
# 4,096 -> 64 (16 per quarter: one full batch), 4,097 -> 65 (17,17,17,14: a second batch)
COLUMN_SIZES = [576 * TILE, 577 * TILE, 640 * TILE + 1, 769 * TILE, 4096 * TILE, 4096 * TILE + 1]


def _uniform_keys(n, bits, seed):
    """keys uniform over all `bits` (every digit column populated), as the narrow unsigned array the host sorts"""
    return np.random.default_rng(seed).integers(0, 1 << bits, n, dtype=np.uint8 if bits <= 8 else np.uint16)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("n", COLUMN_SIZES)
def test_sort_column_scan_layouts(cuda, n, bits):
    assert n > FUSED_TILES * TILE
    narrow = _uniform_keys(n, bits, n + bits)
    _check_sort(cuda, narrow.astype(np.int32), np.arange(n, dtype=np.int32), bits, order=np.argsort(narrow, kind="stable"))


@pytest.mark.parametrize("n", COLUMN_SIZES[-2:])
def test_sort_column_scan_layouts_wide_words(cuda, n):
    narrow = _uniform_keys(n, 8, n + 64)
    vals = np.arange(n, dtype=np.int64) + (1 << 40)
    _check_sort(cuda, narrow.astype(np.int64), vals, 8, order=np.argsort(narrow, kind="stable"))


# ----------------------------------------------------------------------------------------- 1d. the device-side count
@functools.lru_cache(maxsize=None)
def _count_case(n, bits):
    keys = np.random.default_rng(n).integers(0, 1 << bits, n, dtype=np.int64).astype(np.int32)
    keys.setflags(write=False)
    return keys, torch.from_numpy(keys.copy()).cuda(), torch.arange(n, device="cuda", dtype=torch.int32)


def _check_count(cuda, n, bits, count):
    from deftet_amd import hip_ops
    keys, k, v = _count_case(n, bits)
    ko, vo = hip_ops.radix_sort(k, v, bits=bits, n_valid=torch.tensor([count], device=cuda, dtype=torch.int32))
    torch.cuda.synchronize()
    m = min(n, max(count, 0))                                         # the kernels clamp the count to [0, capacity]
    order = np.argsort(keys[:m], kind="stable")
    assert np.array_equal(ko.cpu().numpy()[:m], keys[:m][order])      # (nothing is said about the tail: undefined by contract)
    assert np.array_equal(vo.cpu().numpy()[:m], order.astype(np.int32))
    assert np.array_equal(k.cpu().numpy(), keys)


@pytest.mark.parametrize("count", [0, 1, 2048, 4096, 49_999, 50_000, 50_001, 2**31 - 1, -5])
def test_sort_device_count_fused(cuda, count):
    _check_count(cuda, 50_000, 30, count)


@pytest.mark.parametrize("count", [0, TILE * FUSED_TILES, TILE * FUSED_TILES + 1, 1_200_000, 1_300_000, 1_300_001])
def test_sort_device_count_unfused(cuda, count):
    _check_count(cuda, 1_300_000, 19, count)


# ----------------------------------------------------------------------------------------- 1e. values as bits
SPECIAL_F32 = [0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7FFFFFFF,        # quiet NaNs with payloads, both signs
               0x7F800001, 0x7FA00000, 0xFF800001, 0xFFBFFFFF,        # signalling NaNs
               0x00000000, 0x80000000, 0x7F800000, 0xFF800000,        # +-0, +-inf
               0x00000001, 0x807FFFFF, 0x007FFFFF, 0x80000001]        # denormals


@pytest.mark.parametrize("kdt", [np.int32, np.int64])
@pytest.mark.parametrize("n", [6000, 100_003])
def test_sort_moves_values_as_bits(cuda, kdt, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 12, n).astype(kdt)
    f = np.asarray(SPECIAL_F32, np.uint32)[rng.integers(0, len(SPECIAL_F32), n)]
    f[::3] = rng.integers(0, 1 << 32, len(f[::3]), dtype=np.uint64).astype(np.uint32)      # any pattern at all, NaN payloads included
    _check_sort(cuda, keys, f.view(np.float32), 12)
    wide = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    assert (np.abs(wide.astype(np.float64)) > 2.0**32).mean() > 0.99
    _check_sort(cuda, keys, wide, 12)


# ----------------------------------------------------------------------------------------- 1f. entry checks
def test_sort_entry_checks(cuda):
    """refused before anything is launched (the outputs keep their sentinel); a workspace of exactly the stated size works"""
    from deftet_amd import _lib
    lib = _lib.load()
    n = 5000
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 16, n).astype(np.int32)
    k, v = torch.from_numpy(keys).to(cuda), torch.arange(n, device=cuda, dtype=torch.int32)
    ko, vo = torch.full_like(k, -7), torch.full_like(v, -7)
    need = lib.deftet_radix_sort_workspace_bytes(n, 4, 4)
    assert need > 0
    exact = torch.empty(need, device=cuda, dtype=torch.uint8)
    assert exact.data_ptr() % 256 == 0
    shifted = torch.empty(need + 256, device=cuda, dtype=torch.uint8)[16:16 + need]
    assert shifted.data_ptr() % 256 == 16 and shifted.numel() == need

    def sort(k_in, k_out, v_in, v_out, bits, ws):
        _lib.call("deftet_radix_sort", cuda, k_in, k_out, v_in, v_out, n, 4, 4, bits, None, ws=ws)

    for args in ((k, k, v, vo, 16, exact),                             # keys_out aliases keys_in
                 (k, ko, v, v, 16, exact),                             # values_out aliases values_in
                 (k, ko, v, vo, 16, exact[:need - 1]),                 # one byte short
                 (k, ko, v, vo, 16, shifted),                          # large enough, not 256-aligned
                 (k, ko, v, vo, 0, exact)):                            # no key bits
        with pytest.raises(_lib.DefTetHipError):
            sort(*args)
        torch.cuda.synchronize()
        assert bool((ko == -7).all()) and bool((vo == -7).all())
        assert np.array_equal(k.cpu().numpy(), keys) and torch.equal(v, torch.arange(n, device=cuda, dtype=torch.int32))
    sort(k, ko, v, vo, 16, exact)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(ko.cpu().numpy(), keys[order]) and np.array_equal(vo.cpu().numpy(), order.astype(np.int32))


# ----------------------------------------------------------------------------------------- 2. scans
KINDS = {"exclusive": 0, "inclusive": 1, "max": 2}


def _scan_reference(x, kind):
    with np.errstate(over="ignore"):
        if kind == "max":
            return np.maximum.accumulate(x)
        incl = np.cumsum(x, dtype=x.dtype)
        return incl if kind == "inclusive" else (incl - x).astype(x.dtype)


def _check_scans(cuda, x, kinds=("exclusive", "inclusive", "max")):
    from deftet_amd import hip_ops
    t = torch.from_numpy(x).to(cuda)
    for kind in kinds:
        assert np.array_equal(hip_ops.scan(t, kind).cpu().numpy(), _scan_reference(x, kind)), kind
    assert np.array_equal(t.cpu().numpy(), x)


@pytest.mark.parametrize("n", [1, 64, 8192, 8193, 100_003])
@pytest.mark.parametrize("dt", [np.int32, np.int64])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_scan_in_place(cuda, kind, dt, n):
    """the same tensor as input and output of deftet_scan: the bits of the out-of-place call (and numpy's)"""
    from deftet_amd import _lib, hip_ops
    x = np.random.default_rng(n + KINDS[kind]).integers(-50, 1000, n).astype(dt)
    t = torch.from_numpy(x).to(cuda)
    apart = hip_ops.scan(t, kind)
    _lib.call("deftet_scan", cuda, t, t, n, t.element_size(), KINDS[kind], ws=_lib.load().deftet_scan_workspace_bytes(n, t.element_size()))
    assert torch.equal(t, apart)
    assert np.array_equal(t.cpu().numpy(), _scan_reference(x, kind))


@pytest.mark.parametrize("n", [SCAN_SMALL - 1, SCAN_SMALL, SCAN_SMALL + 1, 100_003])
def test_scan_sums_that_wrap_and_sums_past_32_bits(cuda, n):
    rng = np.random.default_rng(n)
    x32 = rng.integers(2**31 // 1000 - 100_000, 2**31 // 1000 + 100_000, n).astype(np.int32)
    assert int(x32.astype(np.int64).sum()) > 3 * 2**32                    # the int32 sums wrap several times
    _check_scans(cuda, x32, ("exclusive", "inclusive"))
    x64 = rng.integers(2**40 - 1000, 2**40 + 1000, n).astype(np.int64)
    _check_scans(cuda, x64, ("exclusive", "inclusive"))
    _check_scans(cuda, -x64, ("exclusive", "inclusive"))


@pytest.mark.parametrize("n", [SCAN_SMALL - 1, SCAN_SMALL, SCAN_SMALL + 1, 100_003])
@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_scan_running_max_edges(cuda, dt, n):
    lowest = np.iinfo(dt).min                                             # the identity of the running maximum
    rng = np.random.default_rng(n + 3)
    x = rng.integers(-10**9, -1, n).astype(dt)                            # all negative, the identity at position 0 and elsewhere
    x[[0, 5, 63, 64, n // 2, n - 1]] = lowest
    _check_scans(cuda, x, ("max",))
    x[:3 * 2048 + 7] = lowest                                             # whole tiles of the identity before the first real value
    _check_scans(cuda, x, ("max",))
    _check_scans(cuda, np.full(n, lowest, dt), ("max",))
    x = (5 - np.arange(n)).astype(dt)                                     # strictly descending: the output is constant
    from deftet_amd import hip_ops
    assert bool((hip_ops.scan(torch.from_numpy(x).to(cuda), "max") == 5).all())
    base = rng.integers(-1000, 1000, n).astype(dt)
    for p in (63, 64, 2047, 2048, 8191, 8192, n - 1):                     # one maximum above everything else, at p
        if p < n:
            x = base.copy()
            x[p] = 5000
            _check_scans(cuda, x, ("max",))


STEP_AT = [0, 7, 8, 63, 64, 511, 512, 2047, 2048, 8191, 8192, "last"]


@pytest.mark.parametrize("n,p", [(n, p) for n in (SCAN_SMALL - 1, SCAN_SMALL, SCAN_SMALL + 1, 100_003) for p in STEP_AT if p == "last" or p < n - 1])
def test_scan_of_a_single_one_is_a_step(cuda, n, p):
    """(into an output filled with -1, so that an element left unwritten shows whatever the allocator hands out)"""
    from deftet_amd import _lib
    p = n - 1 if p == "last" else p
    at = np.arange(n)
    for dt in (torch.int32, torch.int64):
        t = torch.zeros(n, device=cuda, dtype=dt)
        t[p] = 1
        for kind, step_at in (("exclusive", p + 1), ("inclusive", p)):
            out = torch.full_like(t, -1)
            _lib.call("deftet_scan", cuda, t, out, n, t.element_size(), KINDS[kind], ws=_lib.load().deftet_scan_workspace_bytes(n, t.element_size()))
            assert np.array_equal(out.cpu().numpy(), (at >= step_at).astype(np.int64)), kind
