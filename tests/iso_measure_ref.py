"""numpy fp64 restatement of the iso-solid measures on the tets (tet_iso_measure.hip), written from the contract in
include/deftet_hip.h, for the tests.

Everything is computed in float64 from the float32 inputs widened; the two float32 PREDICATES — a corner is inside iff
field > iso, a tet is live iff det > 0 (field_grad_ref.live_mask) and its four corner values are finite — are evaluated in float32,
so the restatement and the library agree on the case of every tet.

    per_tet(field, pos, tets, iso)                       PerTet(frac, area, vol, live, code, S_frac, S_area, S_vol) [B,T]
    totals(field, pos, tets, iso, weights)               (M [B,5], S [B,5])
    fraction_grads(field, pos, tets, iso, gF, gA, gV)    ((grad_field [B,V], grad_pos [B,V,3]), (S_field, S_pos))
    measures_grads(field, pos, tets, iso, go, weights)   the same for the totals' five upstream scalars
    spline_fraction(f, iso)                              the simplex-spline closed form of the fraction (distinct corner values)
    bound(want, S)                                       marching_tets_ref.entry_bound
Every S holds, entry by entry, the sum of the absolute values of the terms that were added into the entry (cancellations inside
cross products and dot products included), which is what entry_bound takes.
"""
import collections

import numpy as np

from tests import field_grad_ref as G
from tests.marching_tets_ref import entry_bound as bound  # noqa: F401  (re-exported)

F32, F64 = np.float32, np.float64

# case code (bit k = corner k inside) -> the local order of the corners: 1 inside — the inside corner first; 3 inside — the OUTSIDE
# corner first; 2 inside — the inside pair, then the outside pair; each group ascending
ORDER = np.array([(0, 1, 2, 3), (0, 1, 2, 3), (1, 0, 2, 3), (0, 1, 2, 3), (2, 0, 1, 3), (0, 2, 1, 3), (1, 2, 0, 3), (3, 0, 1, 2),
                  (3, 0, 1, 2), (0, 3, 1, 2), (1, 3, 0, 2), (2, 0, 1, 3), (2, 3, 0, 1), (1, 0, 2, 3), (0, 1, 2, 3), (0, 1, 2, 3)])
N_IN = np.array([bin(c).count("1") for c in range(16)])

PerTet = collections.namedtuple("PerTet", "frac area vol live code S_frac S_area S_vol")


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _abscross(a, b):
    """the sums of the absolute values of the two products of every component of a x b (a, b already absolute)"""
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


INPUT = [F32]                                    # the inputs' type; the CPU tests set F64 here to difference the restatement itself


def _gather(field, pos, tets):
    """(f32 corner values [B,T,4], fp64 positions [B,T,4,3], int64 tets [B,T,4])"""
    field, pos = np.asarray(field, INPUT[0]), np.asarray(pos, INPUT[0])
    B = field.shape[0]
    field = field.reshape(B, -1)
    tt = G.tets_of(tets, B)
    bi = np.arange(B)[:, None, None]
    return field[bi, tt], pos.astype(F64)[bi, tt], tt


def _cases(field, pos, tets, iso):
    """what every function here starts from: corner values f32 / f64, positions, the live mask, the case codes"""
    f32, x, tt = _gather(field, pos, tets)
    live = G.live_mask(pos, tets) & np.isfinite(f32).all(-1)
    iso = INPUT[0](iso)
    code = ((f32 > iso) << np.arange(4)).sum(-1)
    return f32.astype(F64), x, tt, live, code, float(iso)


def _volume(x):
    """(vol [N], m [N,4,3] = d det / d x_k, |m| term sums [N,4,3]) in float64, the adjugate rows as tet_frame forms them"""
    e = x[:, 1:] - x[:, :1]
    n = np.stack([_cross(e[:, 1], e[:, 2]), _cross(e[:, 2], e[:, 0]), _cross(e[:, 0], e[:, 1])], 1)
    a = np.abs(e)
    an = np.stack([_abscross(a[:, 1], a[:, 2]), _abscross(a[:, 2], a[:, 0]), _abscross(a[:, 0], a[:, 1])], 1)
    vol = (e[:, 0] * n[:, 0]).sum(-1) / 6.0
    m = np.concatenate([-((n[:, 0] + n[:, 1]) + n[:, 2])[:, None], n], 1)
    am = np.concatenate([((an[:, 0] + an[:, 1]) + an[:, 2])[:, None], an], 1)
    return vol, m, am


def _volume_terms(x):
    """the sum of the absolute values of the six products of det / 6"""
    a = np.abs(x[:, 1:] - x[:, :1])
    return (a[:, 0] * _abscross(a[:, 1], a[:, 2])).sum(-1) / 6.0


Cuts = collections.namedtuple("Cuts", "i o tau ctau gap dfrac adfrac G aG dir")


def _local(f, x, code):
    """corner values and edges from local corner 0 in the local order of each tet's code"""
    order = ORDER[code]                                                   # [N,4]
    r = np.arange(len(code))[:, None]
    fl, xl = f[r, order], x[r, order]
    return order, fl, xl - xl[:, :1]


def _case(f, x, code, iso):
    """frac, area, their term sums and the cuts (lists over the 3 or 4 cuts) of N tets that all have 1 or 3, or all have 2 corners
    inside"""
    order, fl, e = _local(f, x, code)
    n_in = N_IN[code]
    with np.errstate(all="ignore"):
        if (n_in != 2).all():
            gap = fl[:, :1] - fl[:, 1:]                                   # [N,3]
            u, cu = (fl[:, :1] - iso) / gap, (iso - fl[:, 1:]) / gap
            one = n_in == 1
            frac = np.where(one, (u[:, 0] * u[:, 1]) * u[:, 2], (cu[:, 0] + u[:, 0] * cu[:, 1]) + (u[:, 0] * u[:, 1]) * cu[:, 2])
            ue = u[:, :, None] * e[:, 1:]                                 # [N,3,3]
            a, b = ue[:, 0] - ue[:, 2], ue[:, 1] - ue[:, 2]
            aa, ab = np.abs(ue[:, 0]) + np.abs(ue[:, 2]), np.abs(ue[:, 1]) + np.abs(ue[:, 2])
            N = _cross(a, b)
            length = np.sqrt((N * N).sum(-1))
            nh = np.where(length[:, None] > 0, N / np.where(length > 0, length, 1.0)[:, None], 0.0)
            g1, g2 = 0.5 * _cross(b, nh), 0.5 * _cross(nh, a)
            ag1, ag2 = 0.5 * _abscross(ab, np.abs(nh)), 0.5 * _abscross(np.abs(nh), aa)
            sgn = np.where(one, 1.0, -1.0)
            others = [u[:, 1] * u[:, 2], u[:, 0] * u[:, 2], u[:, 0] * u[:, 1]]
            Gs, aGs = [g1, g2, -(g1 + g2)], [ag1, ag2, ag1 + ag2]
            cuts = [Cuts(0, k + 1, u[:, k], cu[:, k], gap[:, k], sgn * others[k], np.abs(others[k]), Gs[k], aGs[k], e[:, k + 1]) for k in range(3)]
            return frac, 0.5 * length, frac, 0.5 * _abscross(aa, ab).sum(-1), cuts, order
        pairs = ((0, 2), (0, 3), (1, 2), (1, 3))
        gap = [fl[:, i] - fl[:, o] for i, o in pairs]
        tau = [(fl[:, i] - iso) / g for (i, o), g in zip(pairs, gap)]
        ct = [(iso - fl[:, o]) / g for (i, o), g in zip(pairs, gap)]
        (al, be, ga, de), (cal, cbe, cga, _cde) = tau, ct
        frac = (al * be + (cal * be) * ga) + (cbe * ga) * de
        e1, e2, e3 = e[:, 1], e[:, 2], e[:, 3]
        e21, e31 = e2 - e1, e3 - e1
        d1 = (e1 + de[:, None] * e31) - al[:, None] * e2
        d2 = (e1 + ga[:, None] * e21) - be[:, None] * e3
        ad1 = (np.abs(e1) + np.abs(de[:, None] * e31)) + np.abs(al[:, None] * e2)
        ad2 = (np.abs(e1) + np.abs(ga[:, None] * e21)) + np.abs(be[:, None] * e3)
        N = _cross(d1, d2)
        length = np.sqrt((N * N).sum(-1))
        nh = np.where(length[:, None] > 0, N / np.where(length > 0, length, 1.0)[:, None], 0.0)
        g13, g12 = 0.5 * _cross(d2, nh), 0.5 * _cross(nh, d1)
        ag13, ag12 = 0.5 * _abscross(ad2, np.abs(nh)), 0.5 * _abscross(np.abs(nh), ad1)
        dfrac = [be * cga, (al + cal * ga) - ga * de, cal * be + cbe * de, cbe * ga]
        adfrac = [be * cga, (al + cal * ga) + ga * de, cal * be + cbe * de, cbe * ga]
        Gs, aGs, dirs = [-g13, -g12, g12, g13], [ag13, ag12, ag12, ag13], [e2, e3, e21, e31]
        cuts = [Cuts(pairs[k][0], pairs[k][1], tau[k], ct[k], gap[k], dfrac[k], adfrac[k], Gs[k], aGs[k], dirs[k]) for k in range(4)]
        return frac, 0.5 * length, frac, 0.5 * _abscross(ad1, ad2).sum(-1), cuts, order


def _groups(live, code):
    """the flat ids of the live tets with 1 or 3, and with 2, corners inside"""
    n_in = N_IN[code]
    return [np.nonzero(live & ((n_in == 1) | (n_in == 3)))[0], np.nonzero(live & (n_in == 2))[0]]


def per_tet(field, pos, tets, iso=0.0):
    f, x, _tt, live, code, iso64 = _cases(field, pos, tets, iso)
    shape = live.shape
    f, x, lv, cd = f.reshape(-1, 4), x.reshape(-1, 4, 3), live.reshape(-1), code.reshape(-1)
    frac = np.where(lv & (cd == 15), 1.0, 0.0)
    area, S_area = np.zeros(len(cd)), np.zeros(len(cd))
    S_frac = frac.copy()
    for ids in _groups(lv, cd):
        if ids.size:
            frac[ids], area[ids], S_frac[ids], S_area[ids], _c, _o = _case(f[ids], x[ids], cd[ids], iso64)
    with np.errstate(all="ignore"):
        vol, S_vol = np.where(lv, _volume(x)[0], 0.0), np.where(lv, _volume_terms(x), 0.0)
    return PerTet(*(a.reshape(shape) for a in (frac, area, vol, lv, cd, S_frac, S_area, S_vol)))


def totals(field, pos, tets, iso=0.0, weights=None):
    """(M [B,5], S [B,5]): sum frac vol, sum area, sum w frac vol, sum w vol, sum vol over the live tets, and the sums of the
    absolute values of their terms"""
    p = per_tet(field, pos, tets, iso)
    w = np.ones(p.frac.shape) if weights is None else np.asarray(weights, F32).astype(F64)
    fv = p.frac * p.vol
    terms = np.stack([fv, p.area, w * fv, w * p.vol, p.vol], -1)
    terms = np.where(p.live[:, :, None], terms, 0.0)
    return terms.sum(1), np.abs(terms).sum(1)


def _vertex_grads(field, pos, tets, iso, upstream):
    """upstream(frac [N], vol [N]) -> (gF, gA, gV, |gF| terms, |gA| terms, |gV| terms) of the N = B T tets, flat"""
    f, x, tt, live, code, iso64 = _cases(field, pos, tets, iso)
    B, T = live.shape
    V = np.asarray(pos).shape[1]
    f, x, lv, cd = f.reshape(-1, 4), x.reshape(-1, 4, 3), live.reshape(-1), code.reshape(-1)
    N = len(cd)
    frac = np.where(lv & (cd == 15), 1.0, 0.0)
    cases = []
    for ids in _groups(lv, cd):
        if ids.size:
            fr, _a, _sf, _sa, cuts, order = _case(f[ids], x[ids], cd[ids], iso64)
            frac[ids] = fr
            cases.append((ids, cuts, order))
    with np.errstate(all="ignore"):
        vol, m, am = _volume(x)
    vol = np.where(lv, vol, 0.0)
    gF, gA, gV, aF, aA, aV = upstream(frac, vol)
    gf, Sf = np.zeros((N, 4)), np.zeros((N, 4))                           # per corner, the tet's own order
    gp, Sp = np.zeros((N, 4, 3)), np.zeros((N, 4, 3))
    ids = np.nonzero(lv)[0]
    gp[ids] = gV[ids, None, None] * (m[ids] / 6.0)
    Sp[ids] = aV[ids, None, None] * (am[ids] / 6.0)
    for ids, cuts, order in cases:
        r = np.arange(len(ids))
        for c in cuts:
            dot, adot = (c.G * c.dir).sum(-1), (c.aG * np.abs(c.dir)).sum(-1)
            ck = gF[ids] * c.dfrac + gA[ids] * dot
            ack = aF[ids] * c.adfrac + aA[ids] * adot
            for end, wgt in ((c.i, c.ctau), (c.o, c.tau)):
                corner = order[r, end]
                gf[ids, corner] += ck * (wgt / c.gap)
                Sf[ids, corner] += ack * np.abs(wgt / c.gap)
                gp[ids, corner] += (gA[ids] * wgt)[:, None] * c.G
                Sp[ids, corner] += (aA[ids] * np.abs(wgt))[:, None] * c.aG
    out = [np.zeros((B, V)), np.zeros((B, V, 3)), np.zeros((B, V)), np.zeros((B, V, 3))]
    flat_v = (np.arange(B)[:, None, None] * V + tt).reshape(-1)          # [B T 4]
    for dst, src in zip(out, (gf, gp, Sf, Sp)):
        np.add.at(dst.reshape((B * V,) + dst.shape[2:]), flat_v, src.reshape((N * 4,) + src.shape[2:]))
    return (out[0], out[1]), (out[2], out[3])


def _flat64(g, n):
    return np.zeros(n) if g is None else np.asarray(g, F32).astype(F64).reshape(-1)


def fraction_grads(field, pos, tets, iso, g_frac=None, g_area=None, g_vol=None):
    """the gradients of sum(frac g_frac) + sum(area g_area) + sum(vol g_vol) on field and pos, with their term sums"""
    def upstream(frac, vol):
        g = [_flat64(x, len(frac)) for x in (g_frac, g_area, g_vol)]
        return g + [np.abs(x) for x in g]
    return _vertex_grads(field, pos, tets, iso, upstream)


def measures_grads(field, pos, tets, iso, go, weights=None):
    """the gradients of sum(totals * go) on field and pos (go [B,5]; the weights a constant), with their term sums"""
    go = np.asarray(go, F32).astype(F64)
    B = go.shape[0]

    def upstream(frac, vol):
        T = len(frac) // B
        w = np.ones(len(frac)) if weights is None else np.asarray(weights, F32).astype(F64).reshape(-1)
        g = [np.repeat(go[:, k], T) for k in range(5)]
        s, a_s = g[0] + w * g[2], np.abs(g[0]) + np.abs(w * g[2])
        return (s * vol, g[1], (s * frac + w * g[3]) + g[4],
                a_s * np.abs(vol), np.abs(g[1]), (a_s * np.abs(frac) + np.abs(w * g[3])) + np.abs(g[4]))
    return _vertex_grads(field, pos, tets, iso, upstream)


def spline_fraction(f, iso):
    """1 - sum_i (iso - f_i)_+^3 / prod_{j != i} (f_j - f_i) of corner values f [...,4], pairwise distinct: the share of a simplex
    on which the linear interpolant exceeds iso"""
    f = np.asarray(f, F64)
    out = np.ones(f.shape[:-1])
    for i in range(4):
        den = np.prod(np.stack([f[..., j] - f[..., i] for j in range(4) if j != i], -1), -1)
        out = out - np.maximum(iso - f[..., i], 0.0) ** 3 / den
    return out


def mesh_area_by_tet(verts, faces, tet_id, n_tet):
    """float64 [n_tet]: the area of a marching-tetrahedra mesh's faces, summed per tet"""
    v = np.asarray(verts, F64)[np.asarray(faces, np.int64)]
    a = 0.5 * np.sqrt((np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) ** 2).sum(-1))
    return np.bincount(np.asarray(tet_id, np.int64), weights=a, minlength=n_tet)
