"""numpy restatement of the surface extraction (deftet_amd/csrc/surface_extract.hip), for the tests.

neighbour_table: nbr[t][i] = the tet across local face i of t (-1: none), from a dict of sorted face keys.  face_mask: the two
predicates as the reference evaluates them — BINARY in fp32, THRESHOLD with the difference in float64 and the occupancy test in
fp32.  extract: the rows in ascending (tet, local face) order.  obj_text / obj_color_text: the reference's per-triangle text."""
import numpy as np

CORNER = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]])      # local face i -> corners (a, b, c) = (i, i^1, i^2)
THRESHOLDS = (0.005, 0.05, 0.15, 0.25)


def neighbour_table(tets):
    tets = np.asarray(tets, np.int64)
    owners = {}
    for t, tet in enumerate(tets.tolist()):
        for i in range(4):
            owners.setdefault(tuple(sorted(tet[c] for c in CORNER[i])), []).append((t, i))
    nbr = -np.ones((tets.shape[0], 4), np.int64)
    for own in owners.values():
        if len(own) > 2:
            raise ValueError("a face has more than two owners")
        if len(own) == 2:
            (t0, f0), (t1, f1) = own
            nbr[t0, f0], nbr[t1, f1] = t1, t0
    return nbr


def face_mask(occ_t, nbr, mode, htres=None):
    """bool [T,4]; occ_t float32 [T]"""
    o = np.asarray(occ_t, np.float32).reshape(-1)
    has = nbr >= 0
    with np.errstate(invalid="ignore"):
        if mode == "binary":
            no = o[np.where(has, nbr, 0)]
            return has & (no != o[:, None]) & (o[:, None] == np.float32(1))
        no = np.where(has, o[np.where(has, nbr, 0)].astype(np.float64), 0.0)
        return (np.abs(no - o[:, None].astype(np.float64)) > float(htres)) & (o[:, None] > np.float32(float(htres) * 2))


def occ_from_weights(weights_v, tets):
    return np.max(np.asarray(weights_v, np.float32).reshape(-1)[np.asarray(tets, np.int64)], axis=1)


def extract(tet_tx4x3, occ_t, nbr, mode, htres=None, attr_tx4xc=None, tets=None):
    """dict(face [F,3,3], face_attr [F,3,C] or None, index [F,2], faces [F,3] or None) of one shape"""
    t, i = np.nonzero(face_mask(occ_t, nbr, mode, htres))          # row-major: ascending (t, i)
    corner = CORNER[i]                                             # [F,3]
    tet = np.asarray(tet_tx4x3)
    return dict(face=tet[t[:, None], corner], face_attr=None if attr_tx4xc is None else np.asarray(attr_tx4xc)[t[:, None], corner],
                index=np.stack([t, i], 1).astype(np.int64), faces=None if tets is None else np.asarray(tets, np.int64)[t[:, None], corner])


def weld(faces_fx3, verts_vx3, attrs=None):
    old = np.unique(faces_fx3)
    remap = -np.ones(verts_vx3.shape[0], np.int64)
    remap[old] = np.arange(old.size)
    return verts_vx3[old], (None if attrs is None else attrs[old]), remap[faces_fx3], old


def obj_text(tri_fx3x3):
    out = []
    for k, tri in enumerate(np.asarray(tri_fx3x3)):
        for c in range(3):
            out.append("v %f %f %f\n" % (tri[c][0], tri[c][1], tri[c][2]))
        out.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 3, 3 * k + 2))
    return "".join(out)


def obj_color_text(tri_fx3x3, col_fx3x3):
    out = []
    col_fx3x3 = np.asarray(col_fx3x3)
    for k, tri in enumerate(np.asarray(tri_fx3x3)):
        for c in range(3):
            out.append("v %f %f %f %f %f %f\n" % (tri[c][0], tri[c][1], tri[c][2], col_fx3x3[k][c][0], col_fx3x3[k][c][1], col_fx3x3[k][c][2]))
        out.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 3, 3 * k + 2))
    return "".join(out)


def threshold_occupancies(T, nbr, seed):
    """float32 [K,T] occupancies for the THRESHOLD fixtures and tests: random; per threshold h a row that puts values ON the two
    comparisons (occ = float32(2h) and the next float above it; neighbour differences of exactly h where h is a float32, one ulp
    to either side of it otherwise); a NaN; nothing above any threshold; every tet occupied."""
    rng = np.random.default_rng(seed)
    rows = [rng.random(T).astype(np.float32), (rng.random(T) < 0.5).astype(np.float32)]
    for h in THRESHOLDS:
        t2 = np.float32(h * 2)
        o = np.full(T, t2, np.float32)
        o[::3] = np.nextafter(t2, np.float32(np.inf))
        o[1::5] = np.float32(h * 4)
        for t in range(0, T, 4):                                   # a neighbour whose difference sits on h
            n = nbr[t][nbr[t] >= 0]
            if n.size:
                base = np.float32(np.float64(o[t]) - h) if o[t] > h else np.float32(0)
                o[n[0]] = base
                if n.size > 1:
                    o[n[1]] = np.nextafter(base, np.float32(-np.inf))
                if n.size > 2:
                    o[n[2]] = np.nextafter(base, np.float32(np.inf))
        rows.append(o)
    nan = rng.random(T).astype(np.float32)
    nan[T // 2] = np.nan
    nan[0] = np.inf
    rows += [nan, np.full(T, 0.005, np.float32), np.ones(T, np.float32)]
    return np.stack(rows)


def binary_occupancies(T, seed):
    """float32 [K,2,T]: random binary pairs; an empty shape next to a full one; a NaN and a non-binary value"""
    rng = np.random.default_rng(seed)
    a = (rng.random((2, T)) < 0.5).astype(np.float32)
    b = np.stack([np.zeros(T, np.float32), np.ones(T, np.float32)])
    c = (rng.random((2, T)) < 0.6).astype(np.float32)
    c[0, T // 3] = np.nan
    c[1, T // 2] = 0.5
    c[1, 0] = 2.0
    return np.stack([a, b, c])
