"""Reference of the rasterizer backward (k_bwd_sorted / k_bwd_runs in csrc/raster.hip) for one shape, in numpy.

analytic      fp64, per used slot (a hit): w0, w1, w2 with den = k3 + eps as the contract has it; gw1, gw2, gk1, gk2, gk3; the hit's
              six-entry contribution to gxy[f] and its 3 D entries to gfeat[f] (the formulas of k_bwd_sorted); their per-face sums,
              the hit counts n_f, S_xy[f] = sum over the face's hits of max|contribution| and S_feat[f] alike.  Two scales that do
              not rest on a cancelled sum: scale_xy[f], the sum over the hits of max(max|contribution|, (|gk1| + |gk2|) reach), reach
              the largest |edge component or pixel offset| of the hit; and T_xy[f], the sum over the hits of the TERM scale
              sum_d |g_d| (|f1 - f0|_d + |f2 - f0|_d) / |den| times reach (1 + |w1| + |w2|), which does not shrink where the D products
              of gw1 or gw2 cancel.
restatement   fp32: the per-hit arithmetic of k_bwd_sorted operation by operation — every product and difference rounded once, the
              channel sums of gw1 / gw2 from 0 in ascending channel order, correctly rounded division — added up in ascending
              sorted-hit order (by face, ascending slot index p * knum + slot inside a face: the order of the stable sort).
              What the build does, checked before relying on this: deftet_amd/build.py compiles every source with
              -ffp-contract=off -fno-fast-math (no -ffast-math, no -munsafe-fp-atomics, no reciprocal flags), raster.hip opens with
              `#pragma clang fp contract(off)` and has no other floating-point pragma (the rest are `#pragma unroll`), and hipcc's
              default keeps the fp32 `/` correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt); so a lane computes what numpy
              computes here.  The kernels add the same terms in another order (a segmented scan; k_bwd_runs four hits per lane
              first), which the bound's n_f covers.
bounds        gfeat (K kappa_f + n_f) u S_feat[f];  gxy (K kappa_f + n_f) u scale_xy[f] + K D u T_xy[f]  (tests/raster_bwd_cases.py: U,
              K, kappa).  K u kappa per hit for the weights and what is built on them, n_f u for a sum of n_f terms in any order.
              This is the shape (K + n_f) u kappa S of bary_ref.bound_tet with two changes, both found on the CPU before any GPU run:
              * n_f multiplies u, not u kappa.  Adding n_f fp32 terms costs n_f u S whatever the conditioning of a term, and with
                kappa on it the bound is above S itself from n_f u kappa >= 1 on — every wave and block case at flat 2^-13 — where no
                defect can leave it (dropping a hit moves a sum by at most S): the sensitivity cases of test_raster_bwd_ref_cpu.py
                could not hold.  For gfeat the bound used is never above the other shape.
              * for gxy the per-hit scale is scale_xy, and the rounding of the D products enters through T_xy.  On a sliver the two
                edges are nearly parallel, gs = gk1 q - gk2 pp and gt = -gk1 nn + gk2 m cancel TOGETHER when gw1 : gw2 meets the
                edges' ratio, and gm = -w1 gs, gn, ... shrink with them, while the error that w1, w2 carry into gk3 stays at
                (|gk1| + |gk2|) reach u kappa.  At image / 2^-13 one face of 576 has a contribution 4,000 times below its terms and
                the restatement stands at 6.5 u kappa max|contribution|: a bound on S_xy alone has a 1 / x tail.
"""
import numpy as np

from tests.raster_bwd_cases import K, U

DEFECTS = ("gk3 without w2", "gn with pp and q swapped", "last hit missing")


def _slots(face):
    """the used slots in sorted-hit order: (p, slot, f) of every hit, by face and ascending slot index inside a face"""
    face = np.asarray(face)
    P, knum = face.shape
    h = np.nonzero(face.reshape(-1) >= 0)[0]
    h = h[np.argsort(face.reshape(-1)[h], kind="stable")]
    return h // knum, h % knum, face.reshape(-1)[h]


def analytic(pix, fxy, feat, face, gout, eps):
    """pix [P,2], fxy [F,3,2], feat [F,3,D], face i64 [P,knum], gout [P,knum,D] -> dict, everything fp64 (hits in sorted order)"""
    pix, fxy, feat, gout = (np.asarray(x, np.float64) for x in (pix, fxy, feat, gout))
    eps = np.float64(np.float32(eps))                                # the kernels receive eps as a float
    F, D = fxy.shape[0], feat.shape[2]
    p, slot, f = _slots(face)
    a, b, c = fxy[f, 0], fxy[f, 1], fxy[f, 2]
    m, pp, nn, q = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    s, t = pix[p, 0] - a[:, 0], pix[p, 1] - a[:, 1]
    k1, k2, k3 = s * q - nn * t, m * t - s * pp, m * q - nn * pp
    den = k3 + eps
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w1, w2 = k1 / den, k2 / den
        w0 = 1 - w1 - w2
        g = gout[p, slot]
        d1, d2 = feat[f, 1] - feat[f, 0], feat[f, 2] - feat[f, 0]
        gw1, gw2 = (g * d1).sum(1), (g * d2).sum(1)
        gk1, gk2, gk3 = gw1 / den, gw2 / den, -(gw1 * w1 + gw2 * w2) / den
        gm, gp_, gn, gq = gk2 * t + gk3 * q, -gk2 * s - gk3 * nn, -gk1 * t - gk3 * pp, gk1 * s + gk3 * m
        gs, gt = gk1 * q - gk2 * pp, -gk1 * nn + gk2 * m
        cxy = np.stack([-(gm + gn + gs), -(gp_ + gq + gt), gm, gp_, gn, gq], 1)                  # [H,6]: a, b, c of gxy[f]
        w = np.stack([w0, w1, w2], 1)
        cfeat = w[:, :, None] * g[:, None, :]                                                     # [H,3,D]
        terms = (np.abs(g) * (np.abs(d1) + np.abs(d2))).sum(1) / np.abs(den)
        reach = np.abs(np.stack([m, pp, nn, q, s, t], 1)).max(1)
        txy = terms * reach * (1 + np.abs(w1) + np.abs(w2))
    out = {"p": p, "slot": slot, "f": f, "w": w, "gw": np.stack([gw1, gw2], 1), "gk": np.stack([gk1, gk2, gk3], 1), "cxy": cxy, "cfeat": cfeat,
           "terms": terms, "txy": txy, "n": np.bincount(f, minlength=F)}
    out["gxy"], out["gfeat"] = np.zeros((F, 6)), np.zeros((F, 3, D))
    out["S_xy"], out["S_feat"], out["T_xy"], out["scale_xy"] = np.zeros(F), np.zeros(F), np.zeros(F), np.zeros(F)
    np.add.at(out["gxy"], f, cxy)
    np.add.at(out["gfeat"], f, cfeat)
    np.add.at(out["S_xy"], f, np.abs(cxy).max(1))
    np.add.at(out["S_feat"], f, np.abs(cfeat).max((1, 2)))
    np.add.at(out["T_xy"], f, txy)
    np.add.at(out["scale_xy"], f, np.maximum(np.abs(cxy).max(1), (np.abs(gk1) + np.abs(gk2)) * reach))
    out["gxy"] = out["gxy"].reshape(F, 3, 2)
    return out


def restatement(pix, fxy, feat, face, gout, eps, defect=None):
    """-> (gxy f32 [F,3,2], gfeat f32 [F,3,D], w f32 [H,3] per hit in sorted order); zero rows for the faces without a hit.
    defect: one of DEFECTS, a deliberate error (the sensitivity cases of tests/test_raster_bwd_ref_cpu.py)"""
    assert defect is None or defect in DEFECTS
    f32 = np.float32
    pix, fxy, feat, gout = (np.asarray(x, f32) for x in (pix, fxy, feat, gout))
    eps = f32(eps)
    F, D = fxy.shape[0], feat.shape[2]
    p, slot, f = _slots(face)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        a, b, c = fxy[f, 0], fxy[f, 1], fxy[f, 2]
        m, pp, nn, q = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
        s, t = pix[p, 0] - a[:, 0], pix[p, 1] - a[:, 1]
        k1, k2, k3 = s * q - nn * t, m * t - s * pp, m * q - nn * pp
        den = k3 + eps
        w1, w2 = k1 / den, k2 / den
        w0 = f32(1) - w1 - w2
        g, ff = gout[p, slot], feat[f]
        gw1, gw2 = np.zeros(f.shape[0], f32), np.zeros(f.shape[0], f32)
        for d in range(D):
            gw1 = gw1 + g[:, d] * (ff[:, 1, d] - ff[:, 0, d])
            gw2 = gw2 + g[:, d] * (ff[:, 2, d] - ff[:, 0, d])
        gk1, gk2 = gw1 / den, gw2 / den
        gk3 = -(gw1 * w1) / den if defect == "gk3 without w2" else -(gw1 * w1 + gw2 * w2) / den
        gm, gp_, gq = gk2 * t + gk3 * q, -gk2 * s - gk3 * nn, gk1 * s + gk3 * m
        gn = -gk1 * t - gk3 * q if defect == "gn with pp and q swapped" else -gk1 * t - gk3 * pp
        gs, gt = gk1 * q - gk2 * pp, -gk1 * nn + gk2 * m
        term = np.concatenate([np.stack([-(gm + gn + gs), -(gp_ + gq + gt), gm, gp_, gn, gq], 1),
                               (np.stack([w0, w1, w2], 1)[:, :, None] * g[:, None, :]).reshape(-1, 3 * D)], 1)
        assert term.dtype == f32 and den.dtype == f32
        # acc += term, in ascending sorted-hit order within every face
        acc = np.zeros((F, 6 + 3 * D), f32)
        start = np.searchsorted(f, f, side="left")
        rank = np.arange(f.shape[0]) - start
        if defect == "last hit missing":
            last = np.searchsorted(f, f, side="right") - 1
            rank = np.where(np.arange(f.shape[0]) == last, -1, rank)
        by_rank = np.argsort(rank, kind="stable")
        cut = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2 if f.size else 1))
        for r in range(len(cut) - 1):
            sel = by_rank[cut[r]: cut[r + 1]]
            acc[f[sel]] = acc[f[sel]] + term[sel]
    return acc[:, :6].reshape(F, 3, 2), acc[:, 6:].reshape(F, 3, D), np.stack([w0, w1, w2], 1)


# ---- the bounds ------------------------------------------------------------------------------------------------------------

def bound_xy(ref, kappa, k=K):
    """[F]: (k kappa_f + n_f) u scale_xy[f] + k D u T_xy[f]"""
    D = ref["gfeat"].shape[2]
    return (k * kappa + ref["n"]) * U * ref["scale_xy"] + k * D * U * ref["T_xy"]


def bound_feat(ref, kappa, k=K):
    """[F]: (k kappa_f + n_f) u S_feat[f]"""
    return (k * kappa + ref["n"]) * U * ref["S_feat"]


def k_needed_xy(err, ref, kappa):
    """[F]: the k at which a face's error meets bound_xy: what is left of the error once the k = 0 term, n_f u scale_xy, is taken
    away, over the factor of k (what K is derived from; -inf for a face without a hit)"""
    D = ref["gfeat"].shape[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref["n"] > 0, (err / U - ref["n"] * ref["scale_xy"]) / (kappa * ref["scale_xy"] + D * ref["T_xy"]), -np.inf)


def k_needed_feat(err, ref, kappa):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref["n"] > 0, (err / U - ref["n"] * ref["S_feat"]) / (kappa * ref["S_feat"]), -np.inf)
