"""Plain torch restatement of the reference's per-tet energies (layers/DefTet/deftet.py:239-338, det_m of
utils/matrix_utils.py:42-47) and the well-conditioned tets the energy tests run on.

`energies` works in the dtype of `tet`: in float64 it is the reference of the GPU tests, in float32 it is what
tests/test_tet_energies_cpu.py pins against the reference's own recorded outputs (tests/golden/deftet_module.npz and
deftet_energies_pows.npz), so that it is known to be the reference's reading of the formulas and not the kernel's.
"""
import numpy as np
import torch

EPS = 1e-10                                                     # deftet.py:18


def _det_m(m):                                                  # matrix_utils.py:42-47 (rows a, b, c: a . (b x c))
    a, b, c = m[..., 0, :], m[..., 1, :], m[..., 2, :]
    n = torch.stack([b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1],
                     b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2],
                     b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]], -1)
    return (a * n).sum(-1)


def volumes(tet):
    """V [B,T], deftet.py:242-254 (scale = 1)."""
    A, B, C, D = (tet[:, :, k, :] for k in range(4))
    m = torch.stack([A - D, B - D, C - D], 2)                   # :248-251
    return -_det_m(m) / 6.0                                     # :253


def amips_per_tet(tet, inv, scale, masked=True):
    """(energy [B,T], det J [B,T]), deftet.py:269-284; masked=False leaves out `* pos_det`."""
    A, B, C, D = (tet[:, :, k, :].unsqueeze(2) * scale for k in range(4))      # :269-272
    off = torch.cat([B - A, C - A, D - A], dim=2)               # :274
    J = off @ inv.to(tet.dtype)[None]                           # :275-278
    trace = (J ** 2).sum(-1).sum(-1)                            # :279
    det = _det_m(J)                                             # :281
    e = trace * torch.pow(torch.pow(det, 2) + EPS, -1.0 / 3.0)  # :283-284
    if masked:
        e = e * (det >= 0.0).to(tet.dtype)                      # :282
    return e, det


def energies(tet, inv, pow_v, pow_e, scale):
    """-> (out [B,3], vol_scale [B], edge_scale [B]).

    out = (volume_variance(pow=pow_v), amips_energy(inv, scale) or 0 without inv, edge_length(pow=pow_e)) with the edge scale
    of the fused operator (the reference's is the constant 20, :321-324).  The two scales say how large the terms are that each
    sum was made of: sum |V - mean|^pow_v and the edge mean with |.|^pow_e — odd exponents cancel, and an error relative to
    the result itself means nothing then.
    """
    V = volumes(tet)
    d = V - V.mean(-1, keepdim=True)                            # :258
    if pow_v == 1:
        vv = d.abs().sum(-1)                                    # :260
    else:
        vv = (d ** pow_v).sum(-1)                               # :262
    vol_scale = (d.abs() ** pow_v).sum(-1)
    if inv is not None:
        am = amips_per_tet(tet, inv, scale)[0].mean(-1)         # :298
    else:
        am = torch.zeros_like(vv)
    A, B, C, D = (tet[:, :, k, :] * scale for k in range(4))    # :326-329
    pairs = ((A, D), (B, D), (C, D), (A, B), (A, C), (B, C))    # :330-335
    n = 6 * tet.shape[1]
    el = sum(((p - q) ** pow_e).sum(-1).sum(-1) for p, q in pairs) / n          # :337-338
    edge_scale = sum(((p - q).abs() ** pow_e).sum(-1).sum(-1) for p, q in pairs) / n
    return torch.stack([vv, am, el], -1), vol_scale.detach(), edge_scale.detach()


INVERT_EVERY, INVERT_AT = 7, 3                                  # tets t % 7 == 3 are inverted
VOLUME_GAP = 5e-6                                               # no |V - mean V| below this (fp32 volumes are off by up to 2e-7)


def make_tets(B, T, seed, scale=20.0, invert="some"):
    """(tet f32 [B,T,4,3], inverse_v f32 [T,3,3], inverted bool [T]) with a controlled Jacobian.

    rest tet = unit corner tet + 0.1 randn; deformed = rest @ M^T + t, M = Q diag(s), Q a random rotation, s uniform in
    [0.6, 1.6]; s_x < 0 for every 7th tet ("some"), for all ("all") or for none ("none").  inverse_v inverts the scaled rest
    offsets (B-A, C-A, D-A), so J = (deformed offsets) inverse_v is similar to M^T: |det J| = s_x s_y s_z >= 0.216, and the
    fp32 evaluation of every term is well conditioned (edges of order 1, no det near 0).

    At pow_v == 1 the energy has a kink at V == mean V: a tet whose fp32 volume falls on the other side of the mean than its
    fp64 volume flips a sign, and through the mean of the signs moves every gradient row of its shape by 2/T.  Among 70,001
    random tets some come within the 2e-7 that fp32 volumes are off by, so such tets (T > 1) are enlarged by 1 % about their
    first vertex until no |V - mean V| of the fp32 coordinates is below VOLUME_GAP.
    """
    rng = np.random.default_rng(seed)
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    rest = corner[None] + 0.1 * rng.standard_normal((T, 4, 3))
    Q, _ = np.linalg.qr(rng.standard_normal((B, T, 3, 3)))
    Q[..., :, 0] *= np.sign(np.linalg.det(Q))[..., None]        # proper rotations
    s = rng.uniform(0.6, 1.6, (B, T, 3))
    inverted = {"some": np.arange(T) % INVERT_EVERY == INVERT_AT, "all": np.ones(T, bool), "none": np.zeros(T, bool)}[invert]
    s[:, inverted, 0] *= -1.0
    M = Q * s[..., None, :]                                     # Q diag(s)
    t = 0.5 * rng.standard_normal((B, T, 1, 3))
    tet = (rest[None] @ np.swapaxes(M, -1, -2) + t).astype(np.float32)
    for _ in range(16 if T > 1 else 0):
        t64 = tet.astype(np.float64)
        V = -np.linalg.det(t64[:, :, :3] - t64[:, :, 3:]) / 6.0
        near = np.abs(V - V.mean(-1, keepdims=True)) < VOLUME_GAP
        if not near.any():
            break
        t64[near] = t64[near][:, :1] + (t64[near] - t64[near][:, :1]) * 1.01
        tet = t64.astype(np.float32)
    else:
        assert T == 1, "make_tets: volumes still within VOLUME_GAP of their mean"
    off = np.stack([rest[:, 1] - rest[:, 0], rest[:, 2] - rest[:, 0], rest[:, 3] - rest[:, 0]], 1) * scale
    inv = np.linalg.inv(off)
    return (torch.from_numpy(tet), torch.from_numpy(inv.astype(np.float32)), torch.from_numpy(inverted))
