"""Row sums (reduce.hip) over every width class of the 16-byte and the 4-byte path, the one-launch ticket form (<= 1,024 rows)
and the two-launch form, both terms, against float64 numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 1023, 100_000, 400_000]
ROWS = [1, 8, 1025]
# the second term's width for each first width: another member of the same set, so that every pairing of a 16-byte and a
# 4-byte term occurs
SECOND = {1: 4, 3: 100_000, 4: 1023, 1023: 400_000, 100_000: 3, 400_000: 100_000}


def _dot64(a, b, block=64):
    """sum_c a[r, c] * b[r, c] in float64 numpy, a few rows at a time (1,025 x 400,000 doubles are 3.3 GB a copy)"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    out = np.empty(a.shape[0], np.float64)
    for r in range(0, a.shape[0], block):
        out[r:r + block] = (a[r:r + block].astype(np.float64) * b[r:r + block].astype(np.float64)).sum(1)
    return out


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("width", WIDTHS)
def test_rowdot_slices(cuda, width, rows):
    from deftet_amd import hip_ops
    g = torch.Generator(device=cuda).manual_seed(1000 * rows + width % 997)
    w2 = SECOND[width]
    a = torch.randn(rows, width, device=cuda, generator=g)
    b = torch.randn(rows, width, device=cuda, generator=g)
    a2 = torch.randn(rows, w2, device=cuda, generator=g)
    b2 = torch.randn(rows, w2, device=cuda, generator=g)
    want1 = _dot64(a, b)
    want = want1 + _dot64(a2, b2)
    got = hip_ops.rowdot(a, b, a2, b2)
    again = hip_ops.rowdot(a, b, a2, b2)
    one = hip_ops.rowdot(a, b)
    torch.cuda.synchronize()
    err = np.abs(got.double().cpu().numpy() - want)
    print("rowdot rows=%d width=%d+%d: max |err| %.3g, max |err| / (1e-3 + 1e-5 |want|) %.3g"
          % (rows, width, w2, err.max(), (err / (1e-3 + 1e-5 * np.abs(want))).max()))
    assert got.shape == (rows,) and got.dtype == torch.float32
    assert np.allclose(got.double().cpu().numpy(), want, rtol=1e-5, atol=1e-3)       # the tolerance of test_rowdot
    assert np.allclose(one.double().cpu().numpy(), want1, rtol=1e-5, atol=1e-3)
    assert torch.equal(got, again)                                                    # deterministic: bit-equal runs
    assert torch.equal(one, hip_ops.rowdot(a, b))
