"""Row sums (deftet_amd/csrc/reduce.hip) on data whose sums are exact in float32 in any order, so that one dropped or doubled element
shows: small integers for `rowdot`, perfect squares for `sqrt_rowsum`.  Widths on both sides of every trip count of the
four-loads-in-flight loop, misaligned bases, the two-launch form, the ticket form across calls and streams, captured launches,
and (in a child process) more streams than there are ticket slots.  Every comparison is equality against int64 sums in numpy."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# restated from reduce.hip: 128 workgroups of 256 threads per row; a thread of the 16-byte path strides 128 * 256 float4 =
# 131,072 columns and enters the batch loop (four loads in flight) with at least four items: n_cols >= 3 * 131,072 + 4 = 393,220
# for thread 0; a second batch trip from 7 * 131,072 + 4 = 917,508.  Up to 1,024 rows take the one-launch ticket form.
STRIDE = 128 * 256 * 4
TICKET_ROWS = 1024
WIDTHS = [1, 2, 3, 4, 5, 8, 131_071, 131_072, 131_073, 393_216, 393_220, 393_221, 917_504, 917_508, 917_512, 917_513, 1_048_580]
# the second term's width: a 16-byte term (width % 4 == 0) meets a 4-byte one both ways round
SECOND = {1: 4, 2: 8, 3: 131_072, 5: 393_216, 131_071: 917_508, 131_073: 393_220, 393_221: 917_504, 917_513: 917_512,
          4: 5, 8: 3, 131_072: 131_073, 393_216: 393_221, 393_220: 131_071, 917_504: 917_513, 917_508: 1, 917_512: 131_073, 1_048_580: 2}
assert sorted(SECOND) == WIDTHS and all((w % 4 == 0) != (SECOND[w] % 4 == 0) for w in WIDTHS)
# at most this many distinct rows are drawn (and summed on the host); a case with more rows repeats them in a random order,
# every row still compared with the host sum of its own data
DISTINCT = 41
EXACT = 2**24


class Rows:
    """[rows, width] of small integers: `host` int32 [distinct, width], `index` [rows] into it, `dev` float32 [rows, width]"""

    def __init__(self, cuda, rng, rows, width, lo, hi, index=None):
        u = min(rows, DISTINCT)
        self.host = rng.integers(lo, hi + 1, (u, width)).astype(np.int32)
        if index is None:
            index = np.arange(rows) if rows == u else np.concatenate([np.arange(u), rng.integers(0, u, rows - u)])
        self.index = index
        d = torch.from_numpy(self.host.astype(np.float32)).to(cuda)
        self.dev = d if rows == u else d[torch.from_numpy(index).to(cuda)].contiguous()


def _dot(a, b=None):
    """(int64 sum_c a*b, int64 sum_c |a*b|) per row of the case"""
    p = a.host * b.host if b is not None else a.host
    return p.sum(1, dtype=np.int64)[a.index], np.abs(p).sum(1, dtype=np.int64)[a.index]


def _exactly(got, want):
    assert got.dtype == torch.float32 and got.shape == want.shape
    return np.array_equal(got.double().cpu().numpy(), want.astype(np.float64))


def _dot_case(cuda, seed, rows, width, width2):
    rng = np.random.default_rng(seed)
    a = Rows(cuda, rng, rows, width, -3, 3)
    b, a2, b2 = (Rows(cuda, rng, rows, w, -3, 3, a.index) for w in (width, width2, width2))
    (s1, m1), (s2, m2), (s0, m0) = _dot(a, b), _dot(a2, b2), _dot(a)
    assert (m1 + m2).max() < EXACT and m0.max() < EXACT        # every product and partial sum is an integer below 2^24: exact in any order
    return (a, b, a2, b2), (s1, s1 + s2, s0)


# ----------------------------------------------------------------------------------------- 3a. every element exactly once
@pytest.mark.parametrize("rows,width", [(r, w) for w in WIDTHS for r in (1, 3)] + [(TICKET_ROWS + 1, 917_512)])
def test_rowdot_is_exact_on_small_integers(cuda, rows, width):
    from deftet_amd import hip_ops
    (a, b, a2, b2), (one, two, plain) = _dot_case(cuda, 100 * width + rows, rows, width, SECOND[width])
    assert _exactly(hip_ops.rowdot(a.dev, b.dev), one)
    assert _exactly(hip_ops.rowdot(a.dev, b.dev, a2.dev, b2.dev), two)
    assert _exactly(hip_ops.rowdot(a.dev), plain)


# ----------------------------------------------------------------------------------------- 3b. one element per row
@pytest.mark.parametrize("width", [917_512, 917_513])
def test_rowdot_sees_every_column(cuda, width):
    """row r is zero but for a[r, p] = b[r, p] = 1, p over every thread-stride boundary of the 16-byte path and the row's ends"""
    from deftet_amd import hip_ops
    at = {0, 3, 4} | set(range(width - 5, width))
    for m in range(0, width, STRIDE):
        at |= {p for p in (m - 1, m, m + 1) if 0 <= p < width}
    at = torch.tensor(sorted(at), device=cuda)
    rows = torch.arange(len(at), device=cuda)
    a = torch.zeros(len(at), width, device=cuda)
    a[rows, at] = 1.0
    b = a.clone()
    assert bool((hip_ops.rowdot(a, b) == 1.0).all())
    assert bool((hip_ops.rowdot(a) == 1.0).all())
    assert bool((hip_ops.rowdot(a, b, b, a) == 2.0).all())


# ----------------------------------------------------------------------------------------- 3c. misaligned bases
def _one_float_in(t):
    """the same values as a contiguous view that starts one float into a larger buffer: 4 bytes off a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("which", ["a", "b", "a2", "b2"])
def test_rowdot_with_a_misaligned_base(cuda, which):
    """widths that are multiples of four, one operand off the 16-byte boundary: that term takes the 4-byte path"""
    from deftet_amd import hip_ops
    rows, width, width2 = 3, 917_512, 393_220
    assert width % 4 == 0 and width2 % 4 == 0
    case, (one, two, plain) = _dot_case(cuda, 77, rows, width, width2)
    t = {k: c.dev for k, c in zip(("a", "b", "a2", "b2"), case)}
    aligned = hip_ops.rowdot(t["a"], t["b"], t["a2"], t["b2"])
    t[which] = _one_float_in(t[which])
    got = hip_ops.rowdot(t["a"], t["b"], t["a2"], t["b2"])
    assert _exactly(got, two) and torch.equal(got, aligned)
    if which in ("a", "b"):
        assert _exactly(hip_ops.rowdot(t["a"], t["b"]), one)
    if which == "a":
        assert _exactly(hip_ops.rowdot(t["a"]), plain)


# ----------------------------------------------------------------------------------------- 3d, 3e. sqrt_rowsum
def _sqrt_case(cuda, seed, rows, width, roots=(0, 5)):
    rng = np.random.default_rng(seed)
    r = Rows(cuda, rng, rows, width, *roots)
    want, _ = _dot(r)
    assert want.max() < EXACT
    return r.dev * r.dev, want                                   # x: perfect squares (exact in float32), the sum of their roots


@pytest.mark.parametrize("rows,width", [(r, w) for w in WIDTHS if w >= 131_071 for r in (1, 8)] + [(TICKET_ROWS, 131_073)])
def test_sqrt_rowsum_forward_is_exact_on_perfect_squares(cuda, rows, width):
    from deftet_amd import hip_ops
    x, want = _sqrt_case(cuda, 100 * width + rows, rows, width)
    assert _exactly(hip_ops.sqrt_rowsum(x, 0.0), want)


@pytest.mark.parametrize("rows,width", [(3, 1001), (8, 131_073), (TICKET_ROWS, 5)])
def test_sqrt_rowsum_backward_is_exact_on_powers_of_two(cuda, rows, width):
    from deftet_amd import hip_ops
    rng = np.random.default_rng(rows + width)
    e = rng.integers(0, 4, (rows, width))                        # x = 4^e in {1, 4, 16, 64}: sqrt(x) = 2^e
    g = rng.integers(-3, 4, rows)                                # upstream gradients 2^g
    x = torch.from_numpy((4.0**e).astype(np.float32)).to(cuda).requires_grad_(True)
    out = hip_ops.sqrt_rowsum(x, 0.0)
    out.backward(torch.from_numpy((2.0**g).astype(np.float32)).to(cuda))
    assert np.array_equal(x.grad.double().cpu().numpy(), 2.0**g[:, None] / (2.0 * 2.0**e))
    assert _exactly(out.detach(), (2**e).sum(1, dtype=np.int64))


def test_sqrt_rowsum_refuses_more_than_the_ticket_rows(cuda):
    from deftet_amd import hip_ops
    with pytest.raises(RuntimeError, match="sqrt_rowsum: at most 1024 rows, got 1025"):
        hip_ops.sqrt_rowsum(torch.ones(TICKET_ROWS + 1, 4, device=cuda), 0.0)


# ----------------------------------------------------------------------------------------- 3f. tickets across calls and streams
@pytest.fixture(scope="module")
def side_streams(cuda):
    """two side streams for the whole module: every distinct stream that runs a row sum takes one of the 32 ticket slots of the
    process for good"""
    return torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)


def _both(hip_ops, case, x):
    a, b, a2, b2 = case
    return hip_ops.rowdot(a.dev, b.dev, a2.dev, b2.dev), hip_ops.sqrt_rowsum(x, 0.0)


def _ticket_case(cuda, seed, rows, width):
    case, (_, two, _) = _dot_case(cuda, seed, rows, width, width // 2 + 1)
    x, roots = _sqrt_case(cuda, seed + 1, rows, width)
    return case, x, two, roots


def test_tickets_across_calls_on_one_stream(cuda):
    """every launch leaves its slot's counters at zero: calls of different shapes back to back are each exact, the last repeats
    the first"""
    from deftet_amd import hip_ops
    got = []
    for rows, width in ((3, 5), (TICKET_ROWS, 131_073), (7, 64), (3, 5)):
        case, x, two, roots = _ticket_case(cuda, 1000 * rows + width, rows, width)
        d, s = _both(hip_ops, case, x)
        assert _exactly(d, two) and _exactly(s, roots), (rows, width)
        got.append((d, s))
    assert torch.equal(got[0][0], got[3][0]) and torch.equal(got[0][1], got[3][1])


@pytest.mark.parametrize("rows,width", [(3, 5), (8, 917_512)])
def test_tickets_on_a_side_stream(cuda, side_streams, rows, width):
    from deftet_amd import hip_ops
    case, x, two, roots = _ticket_case(cuda, 1000 * rows + width, rows, width)
    d0, s0 = _both(hip_ops, case, x)
    side = side_streams[0]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d1, s1 = _both(hip_ops, case, x)
    torch.cuda.current_stream().wait_stream(side)
    assert _exactly(d0, two) and _exactly(s0, roots)
    assert torch.equal(d0, d1) and torch.equal(s0, s1)


def test_tickets_on_two_side_streams_at_once(cuda, side_streams):
    from deftet_amd import hip_ops
    cases = [_ticket_case(cuda, seed, 8, 917_512) for seed in (5, 6)]
    got = []
    for side, (case, x, _, _) in zip(side_streams, cases):       # no synchronisation between the two streams' launches
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got.append(_both(hip_ops, case, x))
    for side in side_streams:
        torch.cuda.current_stream().wait_stream(side)
    for (d, s), (_, _, two, roots) in zip(got, cases):
        assert _exactly(d, two) and _exactly(s, roots)


# ----------------------------------------------------------------------------------------- 3g. captured launches
@pytest.mark.parametrize("rows,width", [(3, 1001), (8, 131_073)])
def test_captured_row_sums_equal_eager(cuda, side_streams, rows, width):
    """a captured launch takes the two-launch form (no counters): replayed twice, the bits of the eager ticket call — the two
    forms share one summation tree"""
    from deftet_amd import hip_ops
    rng = np.random.default_rng(rows)
    (a, b, a2, b2), (_, two, _) = _dot_case(cuda, 9 * rows + width, rows, width, 4 * (width // 8) + 4)
    e = rng.integers(0, 4, (rows, width))
    g = torch.from_numpy((2.0**rng.integers(-3, 4, rows)).astype(np.float32)).to(cuda)
    x = torch.from_numpy((4.0**e).astype(np.float32)).to(cuda).requires_grad_(True)

    def run():
        d = hip_ops.rowdot(a.dev, b.dev, a2.dev, b2.dev)
        s = hip_ops.sqrt_rowsum(x, 0.0)
        (gx,) = torch.autograd.grad(s, x, g)
        return d, s, gx

    eager = [t.detach().clone() for t in run()]
    assert _exactly(eager[0], two) and _exactly(eager[1], (2**e).sum(1, dtype=np.int64))
    s = side_streams[1]
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            out = run()
        del out
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        with torch.no_grad():
            for t in captured:
                t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for c, want in zip(captured, eager):
            assert torch.equal(c.detach().view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------------------- 3h. more streams than ticket slots
def test_row_sums_past_the_last_ticket_slot(cuda):
    """in a fresh process: the slot table is process-wide and never recycled, filling it here would move every later side-stream
    test of this process off the ticket form"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rowdot_slots_child.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("ok: ")]
    assert len(lines) == 1 and lines[0].endswith(" streams") and int(lines[0].split()[1]) >= 33, out.stdout[-500:]
