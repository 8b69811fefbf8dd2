"""References of the fused composite (k_pix_composite / k_pix_composite_bwd in csrc/raster.hip; DESIGN.md "Fused
rasterize-and-composite") for one shape: pix [P,2], fxy [F,3,2], feat [F,3,D], the ranked face [P,knum] (-1 behind the n used
slots), the incoming gradients g = (g_colour [P,Dc], g_coverage [P], g_depth [P]) or None each.

analytic      what the GPU is compared with: fp64 torch autograd of oracle.sparse_render_torch followed by
              deftet_amd.render.alpha_composite, on the fp32 inputs.  alpha_composite clamps to [1e-10, 1 - 1e-10]; in fp32, where
              the operator lives, the upper limit IS 1.0f, an opacity of exactly 1.0 is inside the clamp and its gradient passes.
              In fp64 it would be clamped and masked.  So where a used slot's opacity exceeds 1 - 1e-10 the composition is
              alpha_composite's expression, line by line, with the limits as fp32 has them (composite_fp32_limits;
              test_composite_ref_cpu.py holds it to alpha_composite itself on every case that needs no such limit).
exact         the same numbers in closed form, numpy fp64 — layers, T_i, w_i = alpha_i T_i, v_i, Rseed, Q_i, the layer gradient
              G [P,knum,D] of every used slot, the forward outputs — and next to every value its own expression with every term in
              absolute value (M).  A layer enters M as sum_k what_k |f_k|, what_1 = (|s q| + |n t|) / |den|, what_2 alike,
              what_0 = 1 + what_1 + what_2: the barycentric expression in absolute values, so the conditioning of the weights is
              in M and not in K.  T_i and alpha_i enter as they are (products of positive factors).
              opacity channel   M = T_i sum_{j>=i} (V_j + V_{j+1}) prod_{i<k<=j} (1 - alpha_k),  the last used slot with
                                V_{n-1} + (knum - n) 1e-10 V_empty;  V_j = |g_cov| + sum_c |g_c| (chat_jc + |bg|) + |g_d| (dhat_j + |far|)
              colour, depth     M = w_i |g_c|,  w_i |g_d|
              coverage          M = sum_i w_i + (knum - n) 1e-10 T_n;  colour  sum_i w_i chat_ic + |bg| (1 + M_cov);  depth alike
restatement   numpy fp32, the two kernels' arithmetic from the comments above them: the clamp, T_i as running products, w_i, v_i
              (coverage, then depth, then the colours in channel order), Rseed, Q_i = (v_i - v_{i+1}) + (1 - alpha_{i+1}) Q_{i+1},
              the clamp mask, the colour and depth layer gradients; sequential over the slots where the kernels scan 64 at a time.
              It is there to learn what fp32 needs (K), not to match bits.  `defect` plants one deliberate error (DEFECTS).
bounds        per entry:  layer gradient  k u n M + n 2^-126 S;  forward output  k u (n + 1) M + (n + 1) 2^-126 S  (the empty
              slots' term is one more summand; n = 0 leaves a coverage of knum 1e-10, two roundings).  n the pixel's used slots,
              u = 2^-24, S the largest V of the pixel (the fp32 underflow floor: T_i leaves the normal range after about 45 slots
              of the opaque profile).  To gfeat and gxy in two steps: the fp64 face reduction evaluated on the entry-wise bounds
              with every coefficient in absolute value (carried), plus the face-reduction bound of tests/raster_bwd_ref.py for the
              fp64 layer gradients.
"""
import numpy as np

from tests import raster_bwd_cases as RB
from tests import raster_bwd_ref as R
from tests.composite_cases import ALPHA_HI, ALPHA_LO, EPS, FAR_DEPTH, K, TINY, U, WINDOW

DEFECTS = ("T restarts at 1 at slot 64", "Q is not carried into the window before", "vNext and aNext are 0 at lane 63",
           "Rseed is omitted", "the last used slot has a successor")


def _layers(pix, fxy, feat, face, dtype, eps):
    """-> L [P,K,D] the layers in `dtype`, operation by operation as Slot::layer; Lhat [P,K,D] their absolute-value expression"""
    t = dtype
    pix, fxy, feat = np.asarray(pix, t), np.asarray(fxy, t), np.asarray(feat, t)
    f = np.maximum(face, 0)
    with np.errstate(all="ignore"):
        a, b, c = fxy[f, 0], fxy[f, 1], fxy[f, 2]                      # [P,K,2]
        m, pp, nn, q = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], c[..., 0] - a[..., 0], c[..., 1] - a[..., 1]
        s, tt = pix[:, None, 0] - a[..., 0], pix[:, None, 1] - a[..., 1]
        k1, k2, k3 = s * q - nn * tt, m * tt - s * pp, m * q - nn * pp
        den = k3 + t(eps)
        w1, w2 = k1 / den, k2 / den
        w0 = t(1) - w1 - w2
        ff = feat[f]                                                   # [P,K,3,D]
        L = (w0[..., None] * ff[:, :, 0] + w1[..., None] * ff[:, :, 1]) + w2[..., None] * ff[:, :, 2]
        h1 = (np.abs(s * q) + np.abs(nn * tt)) / np.abs(den)
        h2 = (np.abs(m * tt) + np.abs(s * pp)) / np.abs(den)
        Lhat = (1 + h1 + h2)[..., None] * np.abs(ff[:, :, 0]) + h1[..., None] * np.abs(ff[:, :, 1]) + h2[..., None] * np.abs(ff[:, :, 2])
    assert L.dtype == t
    return L, Lhat


def _grads(g, P, Dc, dtype):
    gc, gv, gd = g
    z = np.zeros
    return (z((P, Dc), dtype) if gc is None else np.asarray(gc, dtype), z(P, dtype) if gv is None else np.asarray(gv, dtype),
            z(P, dtype) if gd is None else np.asarray(gd, dtype))


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))              # NaN stays NaN, as clamp_alpha and torch.clamp


def exact(pix, fxy, feat, face, g, depth, bg, far=FAR_DEPTH, eps=EPS):
    """fp64 closed form -> dict(n, colour, cov, dep, G, M, S, M_colour, M_cov, M_dep, S_fwd, T_end, alpha, T)"""
    face = np.asarray(face, np.int64)
    P, Kn = face.shape
    D = feat.shape[2]
    a, c0 = (1, 2) if depth else (0, 1)
    Dc = D - c0
    used = face >= 0
    n = used.sum(1)
    assert (used == (np.arange(Kn)[None] < n[:, None])).all()         # the used slots come first
    L, Lhat = _layers(pix, fxy, feat, face, np.float64, eps)
    gc, gv, gd = _grads(g, P, Dc, np.float64)
    with np.errstate(all="ignore"):
        araw = L[..., a]
        alpha = np.where(used, _clamp(araw, ALPHA_LO, ALPHA_HI), 0.0)
        om = 1.0 - alpha
        through = np.cumprod(om, 1)
        T = np.concatenate([np.ones((P, 1)), through[:, :-1]], 1)
        T_end = through[:, -1] if Kn else np.ones(P)
        w = np.where(used, alpha * T, 0.0)
        seed = (Kn - n) * ALPHA_LO * T_end
        cov = w.sum(1) + seed
        M_cov = w.sum(1) + seed
        colour = (w[..., None] * L[..., c0:]).sum(1) + bg * (1.0 - cov)[:, None]
        M_colour = (w[..., None] * Lhat[..., c0:]).sum(1) + abs(bg) * (1.0 + M_cov)[:, None]
        dep = (w * L[..., 0]).sum(1) + far * (1.0 - cov) if depth else None
        M_dep = (w * Lhat[..., 0]).sum(1) + abs(far) * (1.0 + M_cov) if depth else None
        v = gv[:, None] + (gc[:, None, :] * (L[..., c0:] - bg)).sum(2)
        V = np.abs(gv)[:, None] + (np.abs(gc)[:, None, :] * (Lhat[..., c0:] + abs(bg))).sum(2)
        vE, VE = gv - bg * gc.sum(1), np.abs(gv) + abs(bg) * np.abs(gc).sum(1)
        if depth:
            v, V = v + gd[:, None] * (L[..., 0] - far), V + np.abs(gd)[:, None] * (Lhat[..., 0] + abs(far))
            vE, VE = vE - far * gd, VE + abs(far) * np.abs(gd)
        Rseed, Rabs = (Kn - n) * ALPHA_LO * vE, (Kn - n) * ALPHA_LO * VE
        Q, MQ = np.zeros((P, Kn)), np.zeros((P, Kn))
        for i in range(Kn - 1, -1, -1):
            last, mid = i == n - 1, i < n - 1
            if i + 1 < Kn:
                q_mid = (v[:, i] - v[:, i + 1]) + om[:, i + 1] * Q[:, i + 1]
                m_mid = (V[:, i] + V[:, i + 1]) + om[:, i + 1] * MQ[:, i + 1]
            else:
                q_mid = m_mid = np.zeros(P)
            Q[:, i] = np.where(last, v[:, i] - Rseed, np.where(mid, q_mid, 0.0))
            MQ[:, i] = np.where(last, V[:, i] + Rabs, np.where(mid, m_mid, 0.0))
        passes = used & (araw >= ALPHA_LO) & (araw <= ALPHA_HI)
        G, M = np.zeros((P, Kn, D)), np.zeros((P, Kn, D))
        G[..., a], M[..., a] = np.where(passes, T * Q, 0.0), np.where(passes, T * MQ, 0.0)
        if depth:
            G[..., 0], M[..., 0] = w * gd[:, None], w * np.abs(gd)[:, None]
        G[..., c0:], M[..., c0:] = w[..., None] * gc[:, None, :], w[..., None] * np.abs(gc)[:, None, :]
        S = np.maximum(np.where(used, V, 0.0).max(1) if Kn else 0.0, VE)
        S = np.maximum(S, np.maximum(np.abs(gc).max(1) if Dc else 0.0, np.abs(gd)))
        S_fwd = np.maximum(np.where(used[..., None], Lhat, 0.0).max((1, 2)) if Kn else 0.0, max(abs(bg), abs(far), 1.0))
    return dict(n=n, used=used, passes=passes, colour=colour, cov=cov, dep=dep, G=G, M=M, S=S, M_colour=M_colour, M_cov=M_cov, M_dep=M_dep,
                S_fwd=S_fwd, alpha=alpha, T=T, T_end=T_end)


def restatement(pix, fxy, feat, face, g, depth, bg, far=FAR_DEPTH, eps=EPS, defect=None):
    """fp32 -> dict(colour [P,Dc], cov [P], dep [P] or None, G [P,knum,D]); zero rows for the unused slots"""
    assert defect is None or defect in DEFECTS
    f32 = np.float32
    face = np.asarray(face, np.int64)
    P, Kn = face.shape
    D = feat.shape[2]
    a, c0 = (1, 2) if depth else (0, 1)
    Dc = D - c0
    used = face >= 0
    n = used.sum(1)
    L, _ = _layers(pix, fxy, feat, face, f32, eps)
    gc, gv, gd = _grads(g, P, Dc, f32)
    have_gc = g[0] is not None
    lo, hi, bg, far, one, zero = f32(ALPHA_LO), f32(ALPHA_HI), f32(bg), f32(far), f32(1), f32(0)
    with np.errstate(all="ignore"):
        araw = L[..., a]
        alpha = np.where(used, _clamp(araw, lo, hi), zero)
        # forward: T_i as running products, the sums slot by slot
        T = np.ones(P, f32)
        Ti, w = np.zeros((P, Kn), f32), np.zeros((P, Kn), f32)
        cov, dep, col = np.zeros(P, f32), np.zeros(P, f32), np.zeros((P, Dc), f32)
        for i in range(Kn):
            u = used[:, i]
            if defect == DEFECTS[0] and i == WINDOW:
                T = np.ones(P, f32)
            Ti[:, i] = T
            w[:, i] = np.where(u, alpha[:, i] * T, zero)
            cov = cov + w[:, i]
            if depth:
                dep = dep + np.where(u, w[:, i] * L[:, i, 0], zero)
            col = col + np.where(u[:, None], w[:, i, None] * L[:, i, c0:], zero)
            T = np.where(u, T * (one - alpha[:, i]), T)
        left = (Kn - n).astype(f32)
        if defect != DEFECTS[3]:
            cov = cov + left * (lo * T)
        colour = col + bg * (one - cov)[:, None]
        depth_out = dep + far * (one - cov) if depth else None
        # backward
        v = np.broadcast_to(gv[:, None], (P, Kn)).astype(f32)
        vE = gv.copy()
        if depth:
            v = v + gd[:, None] * (L[..., 0] - far)
            vE = vE + gd * (zero - far)
        if have_gc:
            for c in range(Dc):
                v = v + gc[:, None, c] * (L[..., c0 + c] - bg)
                vE = vE + gc[:, c] * (zero - bg)
        Rseed = left * (lo * vE)
        if defect == DEFECTS[3]:
            Rseed = np.zeros(P, f32)
        Q = np.zeros((P, Kn), f32)
        for i in range(Kn - 1, -1, -1):
            last, mid = i == n - 1, i < n - 1
            if i + 1 < Kn:
                v1, a1, Q1 = v[:, i + 1], alpha[:, i + 1], Q[:, i + 1]
                if i % WINDOW == WINDOW - 1:
                    if defect == DEFECTS[1]:
                        Q1 = np.zeros(P, f32)
                    if defect == DEFECTS[2]:
                        v1, a1 = np.zeros(P, f32), np.zeros(P, f32)
                q_mid = (v[:, i] - v1) + (one - a1) * Q1
            else:
                q_mid = np.zeros(P, f32)
            q_last = v[:, i] - Rseed
            if defect == DEFECTS[4]:                                  # slot n taken for the zero layer at opacity 1e-10 it is, nothing behind it
                q_last = (v[:, i] - vE) + (one - lo) * zero
            Q[:, i] = np.where(last, q_last, np.where(mid, q_mid, zero))
        passes = used & (araw >= lo) & (araw <= hi)
        G = np.zeros((P, Kn, D), f32)
        G[..., a] = np.where(passes, Ti * Q, zero)
        if depth:
            G[..., 0] = np.where(used, w * gd[:, None], zero)
        if have_gc:
            G[..., c0:] = np.where(used[..., None], w[..., None] * gc[:, None, :], zero)
    for x in (colour, cov, G, Q, v, Ti):
        assert x.dtype == f32
    return dict(colour=colour, cov=cov, dep=depth_out, G=G)


# ---- the bounds ------------------------------------------------------------------------------------------------------------

def layer_bound(ex, k=K):
    """[P,knum,D]: k u n M + n 2^-126 S on the used slots (0 on the others: nothing is written there)"""
    n = ex["n"][:, None, None].astype(np.float64)
    return np.where(ex["used"][..., None], k * U * n * ex["M"] + n * TINY * ex["S"][:, None, None], 0.0)


def forward_bounds(ex, k=K):
    """(colour [P,Dc], coverage [P], depth [P] or None): k u (n + 1) M + (n + 1) 2^-126 S"""
    n1 = ex["n"] + 1.0
    floor = n1 * TINY * ex["S_fwd"]
    return (k * U * n1[:, None] * ex["M_colour"] + floor[:, None], k * U * n1 * ex["M_cov"] + floor,
            None if ex["M_dep"] is None else k * U * n1 * ex["M_dep"] + floor)


def k_needed(err, M, count, floor):
    """the k at which an error meets k u count M + floor (what K is derived from); where M is 0 the entries must be equal"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(M > 0, (err - floor) / (U * count * M), np.where(err > 0, np.inf, -np.inf))


def k_needed_layers(G, ex):
    n = ex["n"][:, None, None].astype(np.float64)
    k = k_needed(np.abs(np.asarray(G, np.float64) - ex["G"]), ex["M"], n, n * TINY * ex["S"][:, None, None])
    return np.where(ex["used"][..., None], k, -np.inf)


def k_needed_forward(res, ex):
    n1 = ex["n"] + 1.0
    floor = n1 * TINY * ex["S_fwd"]
    out = [k_needed(np.abs(res["colour"].astype(np.float64) - ex["colour"]), ex["M_colour"], n1[:, None], floor[:, None]).max(1),
           k_needed(np.abs(res["cov"].astype(np.float64) - ex["cov"]), ex["M_cov"], n1, floor)]
    if ex["dep"] is not None:
        out.append(k_needed(np.abs(res["dep"].astype(np.float64) - ex["dep"]), ex["M_dep"], n1, floor))
    return np.max(out, 0)


def carried(pix, fxy, feat, face, E, eps=EPS):
    """(bxy [F,3,2], bfeat [F,3,D]): the fp64 face reduction (raster_bwd_ref.analytic's formulas) on the entry-wise bounds
    E [P,knum,D] with every coefficient in absolute value"""
    pix, fxy, feat = (np.asarray(x, np.float64) for x in (pix, fxy, feat))
    F, D = fxy.shape[0], feat.shape[2]
    p, slot, f = R._slots(face)
    A = np.abs
    a, b, c = fxy[f, 0], fxy[f, 1], fxy[f, 2]
    m, pp, nn, q = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    s, t = pix[p, 0] - a[:, 0], pix[p, 1] - a[:, 1]
    den = (m * q - nn * pp) + eps
    w1, w2 = (s * q - nn * t) / den, (m * t - s * pp) / den
    w = np.stack([1 - w1 - w2, w1, w2], 1)
    e = E[p, slot]
    e1, e2 = (e * A(feat[f, 1] - feat[f, 0])).sum(1), (e * A(feat[f, 2] - feat[f, 0])).sum(1)
    k1, k2, k3 = e1 / A(den), e2 / A(den), (e1 * A(w1) + e2 * A(w2)) / A(den)
    gm, gp_, gn, gq = k2 * A(t) + k3 * A(q), k2 * A(s) + k3 * A(nn), k1 * A(t) + k3 * A(pp), k1 * A(s) + k3 * A(m)
    gs, gt = k1 * A(q) + k2 * A(pp), k1 * A(nn) + k2 * A(m)
    bxy, bfeat = np.zeros((F, 6)), np.zeros((F, 3, D))
    np.add.at(bxy, f, np.stack([gm + gn + gs, gp_ + gq + gt, gm, gp_, gn, gq], 1))
    np.add.at(bfeat, f, A(w)[:, :, None] * e[:, None, :])
    return bxy.reshape(F, 3, 2), bfeat


def face_bounds(pix, fxy, feat, face, ex, eps=EPS, k=K):
    """(bound_xy [F,3,2], bound_feat [F,3,D], n_f [F], the raster_bwd_ref.analytic dict): carried(layer_bound) + the face-reduction
    bound of raster_bwd_ref"""
    F = fxy.shape[0]
    face = np.asarray(face, np.int64)
    bxy, bfeat = carried(pix, fxy, feat, face, layer_bound(ex, k), eps)
    with np.errstate(all="ignore"):
        ref = R.analytic(pix, fxy, feat, face, ex["G"], eps)
        kappa = RB.kappa(fxy, RB.pixel_reach(pix, face, F), eps)
        return bxy + R.bound_xy(ref, kappa)[:, None, None], bfeat + R.bound_feat(ref, kappa)[:, None, None], ref["n"], ref


# ---- fp64 autograd -----------------------------------------------------------------------------------------------------------

def composite_fp32_limits(layers, depth_layer, background, far_depth):
    """alpha_composite (deftet_amd/render/compositing.py) line by line with the clamp limits as fp32 has them: [1e-10f, 1.0f]"""
    import torch
    alpha = layers[..., :1].clamp(ALPHA_LO, ALPHA_HI)
    through = torch.cumprod(1.0 - alpha, dim=2)
    reach = torch.cat([torch.ones_like(through[:, :, :1]), through[:, :, :-1]], dim=2)
    weight = alpha * reach
    coverage = weight.sum(2)
    colour = (weight * layers[..., 1:]).sum(2) + background * (1.0 - coverage)
    depth = None
    if depth_layer is not None:
        depth = (weight * depth_layer).sum(2) + far_depth * (1.0 - coverage)
    return colour, coverage, depth


def needs_fp32_limits(feat, face, depth):
    """a used slot's face has a corner opacity above 1 - 1e-10: alpha_composite's fp64 clamp would act where the fp32 one does not"""
    f = np.asarray(face)
    return bool((np.asarray(feat, np.float64)[f[f >= 0]][:, :, 1 if depth else 0] > 1.0 - 1e-10).any())


def analytic(pix, fxy, feat, face, g, depth, bg, far=FAR_DEPTH, eps=EPS, composite=None):
    """fp64 autograd -> dict(colour [P,Dc], cov [P], dep [P] or None, gxy [F,3,2], gfeat [F,3,D]) as numpy"""
    import torch
    from deftet_amd.render import alpha_composite
    from oracle import oracle as O
    if composite is None:
        composite = composite_fp32_limits if needs_fp32_limits(feat, face, depth) else alpha_composite
    t = lambda x: torch.from_numpy(np.array(x, np.float64))[None]
    xy, ff = t(fxy).requires_grad_(True), t(feat).requires_grad_(True)
    idx = torch.from_numpy(np.array(face, np.int64))[None]
    layers = O.sparse_render_torch(t(pix), xy, ff, idx, eps=eps)
    # sparse_render_torch reads face 0 at an empty slot and multiplies by 0: behind a NaN layer that sends 0 * NaN back to face 0.
    # The empty slots are zero layers; taken through where() they stay zero layers and pass exactly nothing back.
    layers = torch.where((idx >= 0)[..., None], layers, torch.zeros_like(layers))
    c, v, d = composite(layers[..., 1:], layers[..., :1], bg, far) if depth else composite(layers, None, bg, far)
    gc, gv, gd = g
    loss = 0.0
    if gc is not None:
        loss = loss + (c * t(gc)).sum()
    if gv is not None:
        loss = loss + (v[..., 0] * t(gv)).sum()
    if gd is not None and depth:
        loss = loss + (d[..., 0] * t(gd)).sum()
    gxy, gfeat = torch.autograd.grad(loss, (xy, ff))
    return dict(colour=c[0].detach().numpy(), cov=v[0, :, 0].detach().numpy(), dep=d[0, :, 0].detach().numpy() if depth else None,
                gxy=gxy[0].numpy(), gfeat=gfeat[0].numpy())
