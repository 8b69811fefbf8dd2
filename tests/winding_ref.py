"""A numpy fp64 restatement of the winding-number tree of deftet_amd/csrc/winding_number.hip: the same depth chooser, binning rule,
node quantities, opening test and far-field term, with no fp32 in it.  tests/test_winding_ref_cpu.py measures its error E0 against
the exact sum (check_sign_ref.winding_number); the GPU fast path is then held to 2 E0.

    L = levels(F)                       depth of the tree
    tree = build(verts, faces)          nodes of every level, Morton-indexed, and the faces sorted by leaf (stable)
    w, n_node, n_face = fast(tree, pts, beta)     values, and per point the far-field terms taken and the faces evaluated
    exact(verts, faces, pts)            the plain sum in face order (the same term; compared with check_sign_ref in the CPU test)
"""
import numpy as np

MAX_L = 5
BETA = 3.0


def levels(n_face):
    """floor((floor(log2 F) - 2) / 2) clamped to [0, 5] (C division: truncation towards zero)"""
    lg = max(int(n_face), 1).bit_length() - 1
    return min(max(int((lg - 2) / 2), 0), MAX_L)


def level_offset(l):
    return ((1 << (3 * l)) - 1) // 7


def _spread3(x):
    out = np.zeros_like(x)
    for bit in range(MAX_L):
        out |= ((x >> bit) & 1) << (3 * bit)
    return out


def leaf_of(xyz, lo, inv, L):
    """Morton code (x in the lowest bit of a triple) of the cell floor((x - lo) inv), clamped to [0, 2^L - 1] per axis"""
    G = 1 << L
    c = np.clip(np.floor((xyz - lo[None]) * inv[None]), 0, G - 1).astype(np.int64)
    return _spread3(c[:, 0]) | (_spread3(c[:, 1]) << 1) | (_spread3(c[:, 2]) << 2)


def build(verts, faces, L=None):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    L = levels(f.shape[0]) if L is None else L
    tri = v[f]                                                       # [F,3,3]
    if f.shape[0]:
        corners = tri.reshape(-1, 3)
        lo, hi = corners.min(0), corners.max(0)
    else:
        lo, hi = np.zeros(3), np.zeros(3)
    w = hi - lo
    inv = np.where(w > 1e-30, (1 << L) / np.where(w > 1e-30, w, 1.0), 0.0)
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * (1.0 / 3.0)
    key = leaf_of(cen, lo, inv, L)
    order = np.argsort(key, kind="stable")
    key, tri, cen = key[order], tri[order], cen[order]
    n_leaf = 1 << (3 * L)
    seg = np.searchsorted(key, np.arange(n_leaf + 1))
    # per level: N [n,3], radius [n] (-1: empty), centre [n,3], area [n]
    nvec = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(nvec, axis=1)
    N, R, C, A = np.zeros((n_leaf, 3)), np.full(n_leaf, -1.0), np.zeros((n_leaf, 3)), np.zeros(n_leaf)
    for m in np.nonzero(seg[1:] > seg[:-1])[0]:
        s, e = seg[m], seg[m + 1]
        N[m], A[m] = nvec[s:e].sum(0), area[s:e].sum()
        C[m] = (area[s:e, None] * cen[s:e]).sum(0) / A[m] if A[m] > 0 else cen[s:e].mean(0)
        R[m] = np.sqrt(((tri[s:e].reshape(-1, 3) - C[m][None]) ** 2).sum(1).max())
    lv = {L: (N, R, C, A)}
    for l in range(L - 1, -1, -1):
        cN, cR, cC, cA = lv[l + 1]
        n = 1 << (3 * l)
        N, R, C, A = np.zeros((n, 3)), np.full(n, -1.0), np.zeros((n, 3)), np.zeros(n)
        for m in range(n):
            ch = np.arange(8 * m, 8 * m + 8)
            ch = ch[cR[ch] >= 0]
            if ch.size == 0:
                continue
            N[m], A[m] = cN[ch].sum(0), cA[ch].sum()
            C[m] = (cA[ch, None] * cC[ch]).sum(0) / A[m] if A[m] > 0 else cC[ch].mean(0)
            R[m] = (np.linalg.norm(cC[ch] - C[m][None], axis=1) + cR[ch]).max()
        lv[l] = (N, R, C, A)
    return {"L": L, "levels": lv, "seg": seg, "tri": tri, "lo": lo, "inv": inv, "order": order}


def _terms(tri, p):
    """solid angles over 4 pi of the faces tri [K,3,3] about the points p [P,3] -> [P,K]"""
    a, b, c = (tri[None, :, k, :] - p[:, None, :] for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    det = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return np.arctan2(det, den) / (2.0 * np.pi)


def exact(verts, faces, pts, chunk=1 << 22):
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    p = np.asarray(pts, np.float64)
    out = np.zeros(p.shape[0])
    step = max(1, chunk // max(tri.shape[0], 1))
    for s in range(0, p.shape[0], step):
        out[s:s + step] = _terms(tri, p[s:s + step]).sum(1)
    return out


def fast(tree, pts, beta=BETA):
    p = np.asarray(pts, np.float64)
    L, lv, seg, tri = tree["L"], tree["levels"], tree["seg"], tree["tri"]
    w, n_node, n_face = np.zeros(p.shape[0]), np.zeros(p.shape[0], np.int64), np.zeros(p.shape[0], np.int64)

    def walk(l, m, idx):                                             # idx: the points that walk this subtree
        N, R, C, _A = lv[l]
        if R[m] < 0 or idx.size == 0:
            return
        d = C[m][None] - p[idx]
        d2 = (d * d).sum(1)
        far = d2 > beta * beta * R[m] * R[m]
        fi = idx[far]
        w[fi] += (d[far] @ N[m]) / (d2[far] * np.sqrt(d2[far])) / (4.0 * np.pi)
        n_node[fi] += 1
        op = idx[~far]
        if op.size == 0:
            return
        if l == L:
            s, e = seg[m], seg[m + 1]
            w[op] += _terms(tri[s:e], p[op]).sum(1)
            n_face[op] += e - s
        else:
            for c in range(8):
                walk(l + 1, 8 * m + c, op)

    walk(0, 0, np.arange(p.shape[0]))
    return w, n_node, n_face
