"""fp64 references and a mesh builder for the surface-operator tests (A8 / A9 / A10, normal consistency, chamfer term).

Nothing here touches the GPU or the library under test: `sheet` builds triangle soups whose shared edges have bit-equal
endpoints, `normal_consistency64` and `chamfer64` are the plain torch expressions of the two loss terms in double
precision with autograd (checked against central finite differences in tests/test_surface_ref_cpu.py).
"""
import numpy as np
import torch


def sheet(nx, ny, seed, n=None):
    """float32 [F,3,3]: the corners of a height-field sheet of nx x ny quads, two triangles per quad (F = 2 nx ny), quads
    row by row (x fastest), both triangles of a quad next to each other, all wound the same way.  The corners are taken
    from ONE float32 vertex array, so the endpoints of a shared edge are bit-equal (A8 matches by position).  z is
    jittered by up to 0.3 cell widths.  n: keep the first n faces only (any face count up to 2 nx ny)."""
    rng = np.random.default_rng(seed)
    h = 1.0 / max(nx, ny)
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))             # [ny+1, nx+1], x fastest
    z = rng.uniform(-0.3 * h, 0.3 * h, gx.shape)
    verts = np.stack([gx * h, gy * h, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    v00 = (j * (nx + 1) + i).reshape(-1)
    v10, v01, v11 = v00 + 1, v00 + nx + 1, v00 + nx + 2
    faces = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], 1).reshape(-1, 3)
    tri = verts[faces]
    assert tri.shape == (2 * nx * ny, 3, 3) and tri.dtype == np.float32
    if n is not None:
        assert 0 <= n <= tri.shape[0], (n, tri.shape[0])
        tri = tri[:n]
    return np.ascontiguousarray(tri)


def pad_shapes(shapes, f_max=None):
    """float32 [B, F_max, 3, 3] (zero padded) and the list of face counts of a list of [F_b,3,3] arrays."""
    counts = [int(s.shape[0]) for s in shapes]
    f_max = max(counts) if f_max is None else f_max
    out = np.zeros((len(shapes), f_max, 3, 3), np.float32)
    for b, s in enumerate(shapes):
        out[b, :counts[b]] = s
    return out, counts


def normal_consistency64(tri, adj, n_face):
    """float64 [B]: mean over the valid table entries of 1 - <n_i, n_j>, n = c / sqrt(|c|^2 + 1e-12), c = (v1 - v0) x
    (v2 - v0); 0 for a shape without a valid entry.  tri [B,F_max,3,3] (converted to float64; pass a float64 leaf to
    get its gradient), adj [B,F_max,K] float table, n_face B integers.  The operator's validity rule, made explicit:
    with F = n_face[b], row i counts iff i < F, an entry a counts iff a >= 0 and a < F (NaN fails both), and the
    neighbour is trunc(a)."""
    t = tri.double()
    B, Fm, K = adj.shape
    nf = torch.as_tensor([int(x) for x in n_face], device=t.device).clamp(max=Fm)
    c = torch.linalg.cross(t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 0], dim=-1)
    n = c / torch.sqrt((c * c).sum(-1, keepdim=True) + 1e-12)
    a = adj.double()
    fcol = nf.double()[:, None, None]
    ok = (a >= 0) & (a < fcol) & (torch.arange(Fm, device=t.device)[None, :, None] < nf[:, None, None])
    j = torch.where(ok, torch.trunc(a), torch.zeros_like(a)).long()
    nj = torch.gather(n, 1, j.reshape(B, Fm * K, 1).expand(-1, -1, 3)).reshape(B, Fm, K, 3)
    term = (1 - (n[:, :, None] * nj).sum(-1)) * ok
    return term.sum((1, 2)) / ok.sum((1, 2)).clamp(min=1)


def chamfer64(tri, gt, idx, uv, counts, K):
    """float64 [B]: sum over shape b's first counts[b] * K samples of sqrt(|s - gt[idx]|^2 + 1e-10).  Sample j of face f
    (row f K + j) = (1 - s) a + s (1 - r1) b + s r1 c with s = sqrt(r0): the square-root warp of the two uniform numbers
    uv[0] = r0, uv[1] = r1 ([2,B,F,K]).  idx [B, F K] is GIVEN (the operator's own nearest-neighbour result, verified on
    its own), so that a near-tie of the nearest neighbour cannot enter.  tri [B,F,3,3]; pass a float64 leaf for its
    gradient."""
    t = tri.double()
    B, F = t.shape[0], t.shape[1]
    r = uv.double().reshape(2, B, F, K)
    s = torch.sqrt(r[0])
    wa, wb, wc = 1 - s, s * (1 - r[1]), s * r[1]
    smp = (wa[..., None] * t[:, :, None, 0] + wb[..., None] * t[:, :, None, 1] + wc[..., None] * t[:, :, None, 2]).reshape(B, F * K, 3)
    near = torch.gather(gt.double(), 1, idx.long().reshape(B, F * K, 1).expand(-1, -1, 3))
    d = torch.sqrt(((smp - near) ** 2).sum(-1) + 1e-10)
    nv = torch.as_tensor([int(x) * K for x in counts], device=t.device)
    ok = torch.arange(F * K, device=t.device)[None, :] < nv[:, None]
    return (d * ok).sum(-1)
