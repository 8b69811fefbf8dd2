"""CPU tests of the iso-solid measures on the tets: the restatement of tests/iso_measure_ref.py against the
simplex-spline closed form, the coarea identity and its own differences on random tets (every inside count, corners on the level);
against the closed mesh of the marching-tetrahedra restatement on spheres20(); the five symbols of the C ABI."""
import ctypes
import os
import re

import numpy as np

from tests import field_grad_ref as G
from tests import iso_measure_ref as ref
from tests import marching_tets_cases as cases
from tests import marching_tets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["deftet_tet_iso_fraction_fwd_f32", "deftet_tet_iso_fraction_bwd_f32", "deftet_tet_iso_measures_workspace_bytes",
           "deftet_tet_iso_measures_fwd_f32", "deftet_tet_iso_measures_bwd_f32"]
ISO, H = 0.125, 2.0 ** -10                                    # both float32 numbers


def random_tets(n, seed, on_level=False):
    """(pos f32 [1,4n,3], tets int64 [n,4], field f32 [1,4n]): n separate positively oriented tets with N(0,1) corner values; no
    value within 3 H of ISO, so that ISO +- 2 H is the same case; on_level: one corner of every third tet exactly on ISO"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, (1, 4 * n, 3)).astype(np.float32)
    tets = np.arange(4 * n, dtype=np.int64).reshape(n, 4)
    flip = ~G.live_mask(pos, tets)[0]
    tets[flip] = tets[flip][:, [1, 0, 2, 3]]
    f = rng.normal(0, 0.6, (1, 4 * n)).astype(np.float32)
    near = np.abs(f - ISO) < 3 * H
    f = np.where(near, f + np.float32(6 * H) * np.where(f > ISO, 1, -1), f).astype(np.float32)
    if on_level:
        f[0, tets[::3, 1]] = ISO
    assert G.live_mask(pos, tets).all()
    return pos, tets, f


def test_fraction_equals_the_simplex_spline_closed_form():
    for on_level in (False, True):
        pos, tets, f = random_tets(300, 11, on_level)
        p = ref.per_tet(f, pos, tets, ISO)
        assert set(ref.N_IN[p.code[0]].tolist()) == {0, 1, 2, 3, 4} and p.live.all()
        want = ref.spline_fraction(f[0][tets], ISO)
        assert np.abs(p.frac[0] - want).max() < 1e-12, np.abs(p.frac[0] - want).max()      # (the spline form cancels: ~1e-13 observed)
        assert ((p.frac >= 0) & (p.frac <= 1)).all()
        n_in = ref.N_IN[p.code[0]]
        assert np.all(p.frac[0][n_in == 0] == 0) and np.all(p.frac[0][n_in == 4] == 1) and np.all(p.area[0][(n_in == 0) | (n_in == 4)] == 0)
        if on_level:                                                     # a corner on the level is outside: strict predicate
            assert np.all((p.code[0][::3] >> 1) & 1 == 0)


def test_area_obeys_the_coarea_identity():
    pos, tets, f = random_tets(300, 12)
    stencil = [ref.per_tet(f, pos, tets, ISO + k * H) for k in (-2, -1, 1, 2)]
    assert all(np.array_equal(s.code, stencil[0].code) for s in stencil)   # the condition on the input: one case over the stencil
    fv = [s.frac[0] * s.vol[0] for s in stencil]
    dfv = (fv[0] - 8 * fv[1] + 8 * fv[2] - fv[3]) / (12 * H)               # exact for the cubic frac is in iso; rounding 2^-52 / H
    p = ref.per_tet(f, pos, tets, ISO)
    g, _vol = G.gradient(f[:, :, None], pos, tets, np.float64)
    want = -p.area[0] / np.sqrt((g[0, :, 0] ** 2).sum(-1))
    assert (p.area[0] > 0).sum() > 150
    assert np.abs(dfv - want).max() < 1e-10 * max(1.0, np.abs(want).max()), np.abs(dfv - want).max()
    # the same identity through the restatement's own gradient: shifting the field by c is shifting iso by -c
    (gf, _gp), _S = ref.fraction_grads(f, pos, tets, ISO, g_frac=np.ones((1, len(tets)), np.float32))
    total = np.zeros(len(tets))
    np.add.at(total, np.repeat(np.arange(len(tets)), 4), gf[0][tets.reshape(-1)])        # (the tets share no vertex)
    assert np.abs(total * p.vol[0] + want).max() < 1e-11 * max(1.0, np.abs(want).max())


def test_gradients_equal_central_differences_of_the_restatement():
    pos, tets, f = random_tets(40, 13)
    rng = np.random.default_rng(5)
    T = len(tets)
    gF, gA, gV = (rng.normal(size=(1, T)).astype(np.float32) for _ in range(3))
    go, w = rng.normal(size=(1, 5)).astype(np.float32), rng.uniform(0, 1, (1, T)).astype(np.float32)
    (gf, gp), _S = ref.fraction_grads(f, pos, tets, ISO, gF, gA, gV)
    (mf, mp), _S = ref.measures_grads(f, pos, tets, ISO, go, w)
    ref.INPUT[0] = np.float64
    try:
        def loss(field, p):
            t = ref.per_tet(field, p, tets, ISO)
            m, _ = ref.totals(field, p, tets, ISO, w)
            return float((t.frac * gF + t.area * gA + t.vol * gV).sum()), float((m * go).sum())
        h = 1e-6
        f64, p64 = f.astype(np.float64), pos.astype(np.float64)
        worst = 0.0
        for v in range(0, 4 * T, 3):
            d = np.zeros_like(f64)
            d[0, v] = h
            a, b = loss(f64 + d, p64), loss(f64 - d, p64)
            worst = max(worst, abs((a[0] - b[0]) / (2 * h) - gf[0, v]), abs((a[1] - b[1]) / (2 * h) - mf[0, v]))
            for k in range(3):
                d = np.zeros_like(p64)
                d[0, v, k] = h
                a, b = loss(f64, p64 + d), loss(f64, p64 - d)
                worst = max(worst, abs((a[0] - b[0]) / (2 * h) - gp[0, v, k]), abs((a[1] - b[1]) / (2 * h) - mp[0, v, k]))
    finally:
        ref.INPUT[0] = np.float32
    scale = max(np.abs(gf).max(), np.abs(gp).max(), np.abs(mf).max(), np.abs(mp).max())
    assert worst < 1e-6 * scale, (worst, scale)                           # h^2 f''' / 6 and 2^-52 / h of central differences at h = 1e-6


def sphere_mesh64(b):
    """the closed marching-tetrahedra mesh of shape b of spheres20() with float64 vertices: (verts, faces, tet_id)"""
    pos, field = cases.spheres20()
    _p, tets, edges, tet_edge = cases.grid(20, 1)
    m = R.marching_tets(pos[b], field[b], tets, 0.0, edges=edges, tet_edge=tet_edge)
    (_t, _tb), (verts, _vb), _ = R.forward64(pos[b], field[b], edges, 0.0)
    assert all(R.closed_and_oriented(m.faces, len(verts))[:2])
    return verts, m.faces, m.tet_id


def test_totals_equal_the_closed_mesh_of_marching_tets_on_spheres20():
    pos, field = cases.spheres20()
    tets = cases.grid(20, 1)[1]
    p = ref.per_tet(field, pos, tets, 0.0)
    M, S = ref.totals(field, pos, tets, 0.0)
    assert p.live.all() and np.allclose(M[:, 4], 1.0, rtol=0, atol=1e-6)    # the jitter keeps the cube's volume
    for b in range(2):
        verts, faces, tet_id = sphere_mesh64(b)
        vol, by_tet = R.signed_volume(verts, faces), ref.mesh_area_by_tet(verts, faces, tet_id, len(tets))
        assert abs(M[b, 0] - vol) <= 1e-12 * vol, (M[b, 0], vol)
        assert abs(M[b, 1] - by_tet.sum()) <= 1e-12 * by_tet.sum()
        assert np.abs(p.area[b] - by_tet).max() <= 1e-12 * by_tet.max()
        assert np.array_equal(p.area[b] > 0, by_tet > 0)
        r = (0.3, 0.25)[b]                                               # the scale only: a polyhedron just inside the sphere, three cells to the radius
        assert 0.85 < M[b, 0] / (4 / 3 * np.pi * r ** 3) < 1.0 and 0.9 < M[b, 1] / (4 * np.pi * r ** 2) < 1.0


def test_dead_and_non_finite_tets_give_nothing():
    pos, tets, dead, _lonely = G.dead_tet_mesh()
    f = G.normal_field((1, pos.shape[1]))
    f[0, tets[3, 2]] = np.nan
    f[0, tets[30, 0]] = np.inf
    p = ref.per_tet(f, pos, tets, 0.0)
    gone = ~p.live[0]
    assert gone[list(dead)].all() and gone[3] and gone[30] and gone.sum() < len(tets) / 2
    for a in (p.frac, p.area, p.vol):
        assert np.all(a[0][gone] == 0) and np.isfinite(a).all()
    M, _S = ref.totals(f, pos, tets, 0.0)
    (gf, gp), _ = ref.measures_grads(f, pos, tets, 0.0, np.ones((1, 5), np.float32))
    assert np.isfinite(M).all() and np.isfinite(gf).all() and np.isfinite(gp).all()
    assert abs(M[0, 4] - p.vol.sum()) < 1e-15 and gf[0, tets[3, 2]] == 0      # (every tet of that vertex is dead)


# ---------------------------------------------------------------------------- the C ABI
def test_header_carries_the_400_note_and_declares_the_entries():
    from deftet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    note = re.search(r"^/\* 400:(.*?)\*/", txt, flags=re.S | re.M)
    assert note, "no 400: version note"
    for s in SYMBOLS:
        assert re.sub(r"_(fwd|bwd)_f32$", "", s) in note.group(1), s
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES, s


def test_library_exports_the_entries_and_checks_their_arguments():
    from deftet_amd import _lib, build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    assert lib.deftet_version() >= 400
    buf = ctypes.create_string_buffer(1 << 16)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed
    err = lib.deftet_last_error
    for B in (1, 3, 8):
        need = lib.deftet_tet_iso_measures_workspace_bytes(B)
        assert need == (B * 64 * 5 * 8 + 255) // 256 * 256               # 64 partials of 5 doubles per shape
        for ws, n in ((None, need), (P, need - 1), (ctypes.c_void_p(P.value + 16), need)):
            assert lib.deftet_tet_iso_measures_fwd_f32(P, P, P, None, P, 0.0, B, 27, 48, 1, ws, n, None) == -1
            assert b"workspace null, misaligned or too small: need %d bytes" % need in err()
    assert lib.deftet_tet_iso_measures_workspace_bytes(-1) == 0
    for iso in (float("nan"), float("inf")):
        assert lib.deftet_tet_iso_fraction_fwd_f32(P, P, P, P, None, None, iso, 1, 10, 20, 1, None) == -1 and b"iso is not finite" in err()
        assert lib.deftet_tet_iso_measures_bwd_f32(P, None, P, P, P, P, P, P, P, iso, 1, 10, 20, 1, None) == -1 and b"iso is not finite" in err()
    assert lib.deftet_tet_iso_fraction_fwd_f32(P, P, P, None, None, None, 0.0, 1, 10, 20, 1, None) == -1 and b"null pointer" in err()
    assert lib.deftet_tet_iso_fraction_bwd_f32(P, None, None, P, P, ctypes.c_void_p(P.value + 4), P, P, P, P, 0.0, 1, 10, 20, 1, None) == -1
    assert b"16-byte aligned" in err()
    assert lib.deftet_tet_iso_fraction_fwd_f32(P, P, P, P, None, None, 0.0, 1, 10, 20, 2, None) == -1 and b"batch must be 1 or" in err()
    assert lib.deftet_tet_iso_fraction_fwd_f32(None, None, None, None, None, None, 0.0, 2, 10, 0, 1, None) == 0      # nothing to do
