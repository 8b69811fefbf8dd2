"""CPU checks of tests/surface_ref.py: the sheet builder's face counts and adjacency, and the two fp64 loss references
against central finite differences (fp64 against fp64: step 1e-6, agreement 1e-6 of the largest gradient entry; the
truncation error of a central difference is h^2 f'''/6 ~ 1e-12 f''' and its rounding error eps f / h ~ 1e-10)."""
import numpy as np
import torch

from tests import surface_ref as R


def test_sheet_face_counts_and_shared_vertices():
    assert R.sheet(2, 3, 0).shape == (12, 3, 3)
    big = R.sheet(64, 33, 1)
    assert big.shape == (4224, 3, 3) and big.dtype == np.float32
    for n in (4096, 4097, 0, 1):
        cut = R.sheet(64, 33, 1, n=n)
        assert cut.shape == (n, 3, 3) and np.array_equal(cut, big[:n])           # a prefix of the same sheet
    assert R.sheet(256, 257, 2).shape[0] == 131584 >= 131073
    assert not np.array_equal(R.sheet(4, 4, 0), R.sheet(4, 4, 1))                # the seed moves z
    t = R.sheet(3, 2, 5)
    assert np.array_equal(t[0, 0], t[1, 0]) and np.array_equal(t[0, 2], t[1, 1])  # the diagonal of a quad, bit-equal
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert (n[:, 2] > 0).all()                                                    # one winding
    pad, counts = R.pad_shapes([t, t[:0], t[:5]])
    assert counts == [12, 0, 5] and pad.shape == (3, 12, 3, 3) and (pad[2, 5:] == 0).all() and np.array_equal(pad[2, :5], t[:5])


def test_sheet_adjacency_by_the_oracle(oracle):
    t = R.sheet(5, 4, 3)
    far = (t[:1] + np.float32(50.0)).astype(np.float32)                           # an isolated triangle
    tab = oracle.face_edge_adj(np.concatenate([t, far], 0), 30)
    deg = (tab >= 0).sum(1)
    assert deg[:-1].min() == 1 and deg[:-1].max() == 3 and deg[-1] == 0
    assert deg[:-1].sum() == 3 * (2 * 5 * 4) - 2 * (5 + 4)                        # every boundary edge costs one neighbour
    # symmetric, ascending rows
    for f in range(t.shape[0]):
        row = tab[f][tab[f] >= 0].astype(int)
        assert list(row) == sorted(row) and all(f in tab[g][tab[g] >= 0] for g in row)
    # the 4,097-face prefix of the 64 x 33 sheet ends on a face that still has a neighbour (the row below)
    cut = R.sheet(64, 33, 1, n=4097)
    assert (oracle.face_edge_adj(cut, 30)[-1] >= 0).sum() == 1


def _central_differences(fn, x, h=1e-6):
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        keep = flat[i].item()
        flat[i] = keep + h
        up = fn(x).item()
        flat[i] = keep - h
        dn = fn(x).item()
        flat[i] = keep
        gf[i] = (up - dn) / (2 * h)
    return g


def _small_case(oracle):
    a, b = R.sheet(2, 3, 7), R.sheet(2, 3, 8, n=7)
    tri, counts = R.pad_shapes([a, b])
    tab = np.full((2, 12, 3), -1.0, np.float32)
    for s, (t, c) in enumerate(zip((a, b), counts)):
        tab[s, :c] = oracle.face_edge_adj(t, 3)
    return torch.from_numpy(tri).double(), torch.from_numpy(tab), counts


def test_normal_consistency64_gradient_vs_finite_differences(oracle):
    tri, tab, counts = _small_case(oracle)
    tab[0, 3, 1] = float("nan")                                                   # entries the validity rule drops ...
    tab[0, 4, 0] = 12.0
    tab[1, 2, 2] = 7.0                                                            # (== n_face of shape 1)
    tab[1, 0, 1] = -7.0
    tab[0, 5, 2] = 2.5                                                            # ... and one it truncates to face 2
    w = torch.tensor([0.7, -1.3], dtype=torch.float64)
    fn = lambda t: (R.normal_consistency64(t, tab, counts) * w).sum()
    x = tri.clone().requires_grad_(True)
    val = R.normal_consistency64(x, tab, counts)
    (val * w).sum().backward()
    assert val.dtype == torch.float64 and (val > 0).all() and (val < 1).all()
    assert (x.grad[1, 7:] == 0).all()                                             # beyond the count: no influence
    fd = _central_differences(fn, tri.clone())
    assert (x.grad - fd).abs().max().item() <= 1e-6 * x.grad.abs().max().item()
    # by hand on two faces: coplanar gives 0, a right angle 1
    flat = torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 0, 0], [0, 1, 0], [0, 0, 1]]],
                        dtype=torch.float64)[None]
    t2 = torch.tensor([[[1.0, -1.0], [0.0, -1.0], [-1.0, -1.0]]])
    assert abs(R.normal_consistency64(flat, t2, [3]).item()) < 1e-9               # faces 0 and 1 are coplanar
    t3 = torch.tensor([[[2.0, -1.0], [-1.0, -1.0], [0.0, -1.0]]])
    assert abs(R.normal_consistency64(flat, t3, [3]).item() - 1.0) < 1e-9         # faces 0 and 2 are perpendicular
    assert R.normal_consistency64(flat, torch.full((1, 3, 2), -1.0), [3]).item() == 0.0
    assert R.normal_consistency64(flat, t3, [0]).item() == 0.0


def test_chamfer64_gradient_vs_finite_differences(oracle):
    tri, _, counts = _small_case(oracle)
    K = 3
    rng = np.random.default_rng(4)
    uv = torch.from_numpy(rng.uniform(0.05, 0.95, (2, 2, 12, K)))
    gt = torch.from_numpy(np.stack([rng.uniform(0, 1, (40, 3)) + [0, 0, 0.2], rng.uniform(0, 1, (40, 3)) - [0, 0, 0.25]]))
    first = R.chamfer64(tri, gt, torch.zeros(2, 12 * K, dtype=torch.long), uv, [12, 12], K)
    assert first.shape == (2,)
    # nearest ground-truth point of every sample, by brute force in fp64, then held fixed
    s = torch.sqrt(uv[0])
    smp = ((1 - s)[..., None] * tri[:, :, None, 0] + (s * (1 - uv[1]))[..., None] * tri[:, :, None, 1]
           + (s * uv[1])[..., None] * tri[:, :, None, 2]).reshape(2, -1, 3)
    idx = torch.cdist(smp, gt).argmin(-1)
    w = torch.tensor([1.1, 0.6], dtype=torch.float64)
    fn = lambda t: (R.chamfer64(t, gt, idx, uv, counts, K) * w).sum()
    x = tri.clone().requires_grad_(True)
    val = R.chamfer64(x, gt, idx, uv, counts, K)
    (val * w).sum().backward()
    want = torch.sqrt(((smp - torch.gather(gt, 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1) + 1e-10)
    assert abs(val[0].item() - want[0].sum().item()) < 1e-12 and abs(val[1].item() - want[1, :7 * K].sum().item()) < 1e-12
    assert (x.grad[1, 7:] == 0).all() and x.grad.abs().max() > 0
    fd = _central_differences(fn, tri.clone())
    assert (x.grad - fd).abs().max().item() <= 1e-6 * x.grad.abs().max().item()
    # a sample on corner a (r0 = 0) that coincides with a cloud point: d = sqrt(1e-10), gradient contribution 0, not NaN
    uv0 = uv.clone()
    uv0[0, 0, 0, 0] = 0.0
    gt0 = gt.clone()
    gt0[0, 5] = tri[0, 0, 0]
    idx0 = idx.clone()
    idx0[0, 0] = 5
    x = tri.clone().requires_grad_(True)
    R.chamfer64(x, gt0, idx0, uv0, [1, 0], 1 * K)[0].backward()
    assert torch.isfinite(x.grad).all()
    y = tri.clone().requires_grad_(True)
    uv1, idx1 = uv0[:, :, :, 1:].contiguous(), idx0.reshape(2, 12, K)[:, :, 1:].reshape(2, -1)
    R.chamfer64(y, gt0, idx1, uv1, [1, 0], K - 1)[0].backward()
    assert torch.allclose(x.grad, y.grad, rtol=0, atol=1e-12)                     # the coinciding sample added nothing
