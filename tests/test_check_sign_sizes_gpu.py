"""check_sign at the sizes of real ground-truth meshes, past every size switch of check_sign.hip, and pinned to a
reference that has no ray in it: the fp64 generalised winding number of tests/check_sign_ref.py, computed in
torch.float64 on the device.  PARITY with Kaolin stays UNPINNED (test_check_sign_gpu.py says why); what is pinned
here is that on closed meshes — sphere with pole fans, torus, nested shell, a fine sphere in a 12-face cube — ray
parity from both HIP paths is the parity of the winding number wherever ray parity is well-posed
(check_sign_ref.set_aside marks the rest, at most 1 % of a case), and that the crossing COUNTS of the grid path,
the brute path and the oracle stay equal bit for bit
  * above 128 * 256 faces, where k_prep strides and the box partials are capped (a, b, d),
  * above 1,048,576 faces, where the grid size is capped at 512 (c),
  * in ragged batches whose largest mesh fixes the launch width, with faceless meshes anywhere, and with 32 shapes
    or more, where the offsets reach the device in several launches of host_ints (d, e).
The CPU oracle is compared on a fixed, seeded subsample of the points wherever the whole set would cost more than
about 5e8 ray-face tests; the two HIP paths are always compared on all points.

Set-aside shares measured on an MI355X (in % of a shape's 30,000 points): sphere 0.070 / 0.053, torus 0.057 / 0.087,
shell 0.083 / 0.080, mixed 0.060 / 0.080, 203,400-face sphere 0.070; 1 of the 256 points (0.39 %) of either million-face
sphere.  Three points in all differed from the winding parity, each of them set aside."""
import math

import numpy as np
import pytest
import torch

from tests import check_sign_ref as R

pytestmark = pytest.mark.gpu

ORACLE_TESTS = 5e8            # ray-face tests the CPU oracle is asked for at most, per comparison
MAX_SET_ASIDE = 0.01
K_PARTS_FACES = 128 * 256     # check_sign.hip: kParts box partials of 256 faces each; above it k_prep strides
MAX_G, MAX_SPAN = 512, 16
DEVICE_BUDGET = 1 << 25       # elements per fp64 temporary of the reference on the device


def _t(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _pick_g(F):
    return int(math.ceil(math.sqrt(F) / 2.0))


SECOND = (0.9, np.float64([0.03, -0.02, 0.05]))


def _two_shapes(v):
    """the same mesh twice with different vertex positions: as is, and scaled by 0.9 and shifted"""
    return np.stack([v, (v.astype(np.float64) * SECOND[0] + SECOND[1]).astype(np.float32)])


def _points(verts_b, faces, n_uniform, n_near, seed):
    return np.stack([R.points_for(v, faces, n_uniform, n_near, seed + 10 * b) for b, v in enumerate(verts_b)])


def _hip_counts(cuda, verts, faces, pts):
    """(inside, count) of the grid path and of the brute path, device tensors"""
    from deftet_amd import hip_ops
    v, f, p = _t(verts, cuda), _t(faces, cuda), _t(pts, cuda)
    return hip_ops.check_sign(v, f, p, brute=False, return_count=True), hip_ops.check_sign(v, f, p, brute=True, return_count=True)


def _subsample(B, N, F, seed):
    """all points where the oracle can afford them, else a fixed seeded subsample (sorted indices)"""
    n = int(ORACLE_TESTS // max(B * F, 1))
    if n >= N:
        return np.arange(N)
    return np.sort(np.random.default_rng(seed).choice(N, size=n, replace=False))


def _check_counts(cuda, oracle, verts, faces, pts, seed=0):
    """grid == brute on all points, both == oracle on the (sub)sample; returns the grid path's (inside, count) as numpy"""
    (a, ca), (b, cb) = _hip_counts(cuda, verts, faces, pts)
    assert torch.equal(ca, cb) and torch.equal(a, b)
    assert torch.equal(a, (ca & 1).bool())
    idx = _subsample(pts.shape[0], pts.shape[1], faces.shape[0], seed)
    want, cw = oracle.check_sign(verts, faces, pts[:, idx], return_count=True)
    ca_n, a_n = ca.cpu().numpy(), a.cpu().numpy()
    assert np.array_equal(ca_n[:, idx], cw) and np.array_equal(a_n[:, idx], want)      # crossing counts, bit for bit
    return a_n, ca_n


def _winding_pin(cuda, name, verts, faces, pts, inside, idx=None):
    """parity == winding parity wherever the point is not set aside, per shape; the set-aside share is capped.
    Returns the set-aside mask of every shape."""
    f = _t(faces, cuda)
    asides = []
    for b in range(verts.shape[0]):
        p = pts[b] if idx is None else pts[b][idx]
        got = inside[b] if idx is None else inside[b][idx]
        pd = _t(p, cuda)
        w = R.winding_number(_t(verts[b], cuda), f, pd, budget=DEVICE_BUDGET)
        assert w.dtype == torch.float64 and w.device.type == torch.device(cuda).type
        aside = R.set_aside(_t(verts[b], cuda), f, pd, budget=DEVICE_BUDGET).cpu().numpy()
        w = w.cpu().numpy()
        assert np.abs(w - np.round(w)).max() <= 1e-9
        diff = got != R.winding_inside(w)
        asides.append(aside)
        print("%s shape %d: %d faces, %d points, set aside %.3f %%, mismatches %d, of them not set aside %d"
              % (name, b, faces.shape[0], p.shape[0], 100 * aside.mean(), diff.sum(), (diff & ~aside).sum()))
        assert not (diff & ~aside).any()
        assert aside.mean() <= MAX_SET_ASIDE
    return asides


# ------------------------------------------------------------------------------------------ a. fp64 pin at real sizes
def _pin_mesh(kind):
    if kind == "sphere":
        v, f = R.uv_sphere(92)                                      # 33,488 faces
        return R.rotate(v, 21), f, 21
    if kind == "torus":
        v, f = R.torus(170, 100)                                    # 34,000 faces; the one UNROTATED case: rings in planes z = const
        return v, f, None
    if kind == "shell":
        v, f = R.shell(91)                                          # 65,520
        return R.rotate(v, 23), f, 23
    if kind == "mixed":
        v, f = R.mixed(92)                                          # 33,488 + 12
        return R.rotate(v, 24), f, 24
    v, f = R.uv_sphere(226)                                         # 203,400: the size of a ground-truth mesh
    return R.rotate(v, 25), f, 25


PIN_KINDS = ["sphere", "torus", "shell", "mixed", "sphere_203k"]


@pytest.mark.parametrize("kind", PIN_KINDS)
def test_parity_is_the_fp64_winding_parity(cuda, oracle, kind):
    v, f, rot = _pin_mesh(kind)
    F = f.shape[0]
    assert F > K_PARTS_FACES
    verts = v[None] if kind == "sphere_203k" else _two_shapes(v)
    pts = _points(verts, f, 20000, 10000, seed=300 + 100 * PIN_KINDS.index(kind))
    inside, cnt = _check_counts(cuda, oracle, verts, f, pts, seed=1)
    asides = _winding_pin(cuda, kind, verts, f, pts, inside)
    assert cnt.max() >= (4 if kind in ("torus", "shell") else 2)
    assert 0.02 < inside.mean() < 0.6
    if kind == "mixed":
        # the twelve cube faces span far more than 16 cells each: they are in the list that every point tests.  The grid
        # covers the enlarged boxes of the regular faces: an axis of it is at most (1 + 1/16) E long, E the mesh's largest extent
        G = _pick_g(F)
        cell = 1.0625 * float((v.max(0) - v.min(0))[1:].max()) / G
        tri = v[f[-12:]]
        span = np.floor((tri[:, :, 1].max(1) - tri[:, :, 1].min(1)) / cell) * np.floor((tri[:, :, 2].max(1) - tri[:, :, 2].min(1)) / cell)
        assert span.max() > MAX_SPAN
        # ... and they were counted: between the cube and the sphere the cube once, plus the sphere twice where the ray meets it
        # (1 or 3: inside); within the sphere two, the sphere's and the cube's (an even count: outside by parity, as the
        # winding number 2 says)
        q = R.rotation(rot)
        for b, (s, t) in enumerate(((1.0, np.zeros(3)), SECOND)):
            local = ((pts[b].astype(np.float64) - t) / s) @ q
            aside = asides[b]
            rad = np.linalg.norm(local, axis=1)
            between = (np.abs(local).max(1) < R.CUBE_H - 1e-3) & (rad > R.MIXED_R + 1e-3) & ~aside
            within = (rad < R.MIXED_R - 1e-3) & ~aside
            assert between.mean() > 0.1 and within.mean() > 0.01
            assert inside[b][between].all() and np.isin(cnt[b][between], (1, 3)).all() and (cnt[b][between] == 3).any()
            assert (cnt[b][within] == 2).all()


# ------------------------------------------------------------------------------------------ b. around 128 * 256 faces
_big = {}


def _sphere_70k():
    if not _big:
        v, f = R.uv_sphere(133)                                     # 70,224 faces
        _big["m"] = (R.rotate(v, 31), f)
    return _big["m"]


F_AROUND = [K_PARTS_FACES - 1, K_PARTS_FACES, K_PARTS_FACES + 1, 2 * K_PARTS_FACES + 1]


def _through_faces(v, f):
    """points whose ray crosses, at its centroid, one of the faces a wrong loop bound or stride would lose: the first ones,
    those on either side of every multiple of 128 * 256, and the last ones.  (A lost face changes the count of its point; random
    points alone would hardly ever look through one given face of 30,000.)"""
    F = f.shape[0]
    ks = sorted({k for m in range(0, F + 1, K_PARTS_FACES) for k in range(m - 3, m + 3) if 0 <= k < F} | set(range(F - 3, F)))
    c = v.astype(np.float64)[f[ks]].mean(1)
    return (c - np.float64([0.05, 0.0, 0.0])).astype(np.float32), ks


@pytest.mark.parametrize("F", F_AROUND)
def test_counts_around_the_partial_cap(cuda, oracle, F):
    """the first F faces of one sphere (an open surface is fine for counts): at 32,769 faces k_prep's loop takes its first
    second trip, at 65,537 every thread has taken two and the first a third"""
    v, f = _sphere_70k()
    f = np.ascontiguousarray(f[:F])
    assert f.shape[0] == F and F_AROUND[-1] > K_PARTS_FACES
    verts = _two_shapes(v)
    aimed = np.stack([_through_faces(vb, f)[0] for vb in verts])
    pts = np.concatenate([_points(verts, f, 3000, 1000 - aimed.shape[1], seed=40), aimed], axis=1)
    assert pts.shape == (2, 4000, 3)
    _, cnt = _check_counts(cuda, oracle, verts, f, pts, seed=2)
    assert cnt.max() >= 2 and (cnt[:, -aimed.shape[1]:] >= 1).all()


def _tiny_torus(seed=5, n_u=12, n_v=7):
    v, f = R.torus(n_u, n_v)
    return R.rotate(v, seed), f


def _one_face():
    return np.float32([[-0.3, -0.5, -0.4], [-0.3, 0.5, -0.3], [-0.25, -0.1, 0.6]]), np.int64([[0, 1, 2]])


def _check_ragged(cuda, oracle, meshes, pts):
    """check_sign_ragged on both paths == per-shape check_sign == per-shape oracle, counts and all"""
    from deftet_amd import hip_ops
    vl, fl, p = [_t(m[0], cuda) for m in meshes], [_t(m[1], cuda) for m in meshes], _t(pts, cuda)
    want = [oracle.check_sign(m[0][None], m[1], pts[b:b + 1], return_count=True) for b, m in enumerate(meshes)]
    for brute in (False, True):
        got, cnt = hip_ops.check_sign_ragged(vl, fl, p, brute=brute, return_count=True, check=True)
        assert got.shape == pts.shape[:2] and got.dtype == torch.bool
        for b, m in enumerate(meshes):
            one, c1 = hip_ops.check_sign(vl[b][None], fl[b], p[b:b + 1], brute=brute, return_count=True)
            assert torch.equal(cnt[b], c1[0]) and torch.equal(got[b], one[0]), (brute, b)
            assert np.array_equal(cnt[b].cpu().numpy(), want[b][1][0]), (brute, b)
            assert np.array_equal(got[b].cpu().numpy(), want[b][0][0]), (brute, b)
            if m[1].shape[0] == 0:                                  # no faces: all outside, no crossing
                assert not got[b].any() and not cnt[b].any()
    return cnt


@pytest.mark.parametrize("F", F_AROUND)
def test_ragged_batch_whose_largest_mesh_sets_the_launch_width(cuda, oracle, F):
    """[tiny torus, F faces, one face]: the launch width comes from the F faces, so most blocks of the two small meshes
    see no face and store an empty box partial"""
    v, f = _sphere_70k()
    meshes = [_tiny_torus(), ((v * np.float32(0.9)).astype(np.float32), np.ascontiguousarray(f[:F])), _one_face()]
    pts = np.stack([R.uniform_points(v, 4000, seed=50 + b) for b in range(3)])
    aimed = _through_faces(*meshes[1])[0]
    pts[1, -aimed.shape[0]:] = aimed
    cnt = _check_ragged(cuda, oracle, meshes, pts)
    assert (cnt[1, -aimed.shape[0]:] >= 1).all()
    assert all(cnt[b].max() >= 1 for b in range(3))


# ------------------------------------------------------------------------------------------ c. the cap of the grid size
@pytest.mark.parametrize("n_lat,capped", [(513, True), (511, False)])
def test_grid_size_cap(cuda, oracle, n_lat, capped):
    """1,050,624 faces: ceil(sqrt(F) / 2) = 513 is cut to 512; 1,042,440 faces: G = 511, the last sizes without the cut"""
    v, f = R.uv_sphere(n_lat)
    v = R.rotate(v, 60 + n_lat)
    F = f.shape[0]
    assert F == R.sphere_faces_of(n_lat) and (_pick_g(F) > MAX_G) == capped and (F > 1048576) == capped
    pts = _points(v[None], f, 2048, 2048, seed=70)
    (a, ca), (b, cb) = _hip_counts(cuda, v[None], f, pts)
    assert torch.equal(ca, cb) and torch.equal(a, b)                # every point
    assert int(ca.max()) >= 2
    idx = np.sort(np.random.default_rng(71).choice(pts.shape[1], size=256, replace=False))
    assert 256 * F <= ORACLE_TESTS
    want, cw = oracle.check_sign(v[None], f, pts[:, idx], return_count=True)
    assert np.array_equal(ca.cpu().numpy()[:, idx], cw) and np.array_equal(a.cpu().numpy()[:, idx], want)
    _winding_pin(cuda, "sphere n_lat=%d" % n_lat, v[None], f, pts, a.cpu().numpy(), idx=idx)


# ------------------------------------------------------------------------------------------ d. ragged batches
def _sphere_40k():
    if "s40" not in _big:
        v, f = R.uv_sphere(101)                                     # 40,400 faces
        _big["s40"] = (R.rotate(v, 32), f)
    return _big["s40"]


def _no_faces(n_verts):
    return np.random.default_rng(n_verts).random((n_verts, 3)).astype(np.float32) - 0.5, np.zeros((0, 3), np.int64)


@pytest.mark.parametrize("order", ["01234", "20143", "31402"])
def test_ragged_batch_with_faceless_meshes(cuda, oracle, order):
    """[no faces, one face, 40k sphere, tiny torus, no faces] and two permutations: faceless meshes in the middle, a real
    mesh first and last.  (k_prep, k_bin and k_query with M.F == 0: the face loops do not run, every thread of k_bin
    leaves at k >= F after the wave-wide box reduction, a point's cell holds an empty list and the irregular count is 0 —
    nothing of an empty mesh is dereferenced; one of the two has no vertices either.)"""
    base = [_no_faces(5), _one_face(), _sphere_40k(), _tiny_torus(), _no_faces(0)]
    meshes = [base[int(c)] for c in order]
    assert max(m[1].shape[0] for m in meshes) > K_PARTS_FACES
    nf = [m[1].shape[0] for m in meshes]
    assert order == "01234" or (nf[0] and nf[-1] and 0 in nf[1:-1])
    pts = np.stack([R.uniform_points(_sphere_40k()[0], 2000, seed=80 + b) for b in range(5)])
    _check_ragged(cuda, oracle, meshes, pts)


def test_ragged_batch_of_33_shapes(cuda, oracle):
    """2 (B + 1) = 68 offsets: more than one launch of host_ints carries (64 values each)"""
    meshes = []
    for b in range(33):
        if b in (7, 32):
            meshes.append(_no_faces(3))
        elif b % 3 == 0:
            v, f = R.uv_sphere(4 + b // 3)
            meshes.append((R.rotate(v, 200 + b), f))
        elif b % 3 == 1:
            meshes.append(_tiny_torus(200 + b, 8 + b, 5 + b // 4))
        else:
            v, f = R.shell(3 + b // 3)
            meshes.append((R.rotate(v, 200 + b), f))
    B = len(meshes)
    assert B == 33 and 2 * (B + 1) > 64
    assert len({(m[0].shape[0], m[1].shape[0]) for m in meshes}) == B - 1             # all different (the two faceless ones alike)
    pts = np.stack([R.uniform_points(_sphere_40k()[0], 600, seed=90 + b) for b in range(B)])
    cnt = _check_ragged(cuda, oracle, meshes, pts)
    assert int(cnt.max()) >= 4


def test_module_with_two_large_meshes(cuda):
    """DefTet.check_tet_inside_sdfs with a per-shape list of two meshes of 40k faces or more == the ragged call"""
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    v1, f1 = R.torus(150, 140)                                      # 42,000 faces
    meshes = [_sphere_40k(), (R.rotate(v1, 33), f1)]
    assert all(m[1].shape[0] >= 40000 for m in meshes)
    pts = np.stack([R.points_for(m[0], m[1], 3000, 1000, seed=95 + b) for b, m in enumerate(meshes)])
    vl, fl, p = [_t(m[0], cuda) for m in meshes], [_t(m[1], cuda) for m in meshes], _t(pts, cuda)
    tet = p[:, :, None, :].expand(-1, -1, 4, -1).contiguous()       # four equal corners: the centroid is the point, exactly
    occ = DefTet(device=cuda).check_tet_inside_sdfs(tet, ([v[None] for v in vl], [[f] for f in fl]))
    want = hip_ops.check_sign_ragged(vl, fl, p)
    assert occ.shape == (2, 4000, 1) and occ.dtype == torch.float32
    assert torch.equal(occ[..., 0] > 0.5, want) and torch.equal(want, hip_ops.check_sign_ragged(vl, fl, p, brute=True))
    assert 0.05 < want.float().mean() < 0.9


def test_ragged_mesh_without_vertices_raises(cuda):
    """a face of a mesh that has NO vertices, placed last: every index is outside its mesh, nothing is gathered for it (vertex 0
    would lie past the end of the vertex array), and check=True raises"""
    from deftet_amd import hip_ops
    tv, tf = _tiny_torus()
    vl = [_t(tv, cuda), torch.zeros(0, 3, device=cuda)]
    fl = [_t(tf, cuda), torch.zeros(1, 3, dtype=torch.int64, device=cuda)]
    p = _t(np.stack([R.uniform_points(tv, 300, seed=b) for b in range(2)]), cuda)
    for brute in (False, True):
        with pytest.raises(IndexError):
            hip_ops.check_sign_ragged(vl, fl, p, brute=brute, check=True)
        got, cnt = hip_ops.check_sign_ragged(vl, fl, p, brute=brute, return_count=True, check=False)
        assert not cnt[1].any() and not got[1].any()                # the record of such a face never hits
        assert torch.equal(cnt[0], hip_ops.check_sign(vl[0][None], fl[0], p[:1], brute=brute, return_count=True)[1][0])


# ------------------------------------------------------------------------------------------ e. host_ints on its own
def _values(n, seed):
    special = [0, -1, 2 ** 31 - 1, -(2 ** 31), 2 ** 24 + 1, -(2 ** 24) - 1, 7]
    rng = np.random.default_rng(seed)
    vals = [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, size=n)]
    for i, s in enumerate(special[:n]):
        vals[(i * 11) % n] = s
    return vals


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 130])
def test_host_ints(cuda, n):
    """one launch carries 64 values: 0, 1, up to, at and past one launch, exactly two, and a third, partial one"""
    from deftet_amd import hip_ops
    vals = _values(n, n)
    wide = list(vals)
    if n:
        wide[n // 2] = 2 ** 40 + 3                                  # int64 only
    a = hip_ops.host_ints(vals, cuda, i32=True)
    b = hip_ops.host_ints(wide, cuda, i64=True)
    c = hip_ops.host_ints(vals, cuda, f32=True)
    a3, b3, c3 = hip_ops.host_ints(vals, cuda, i32=True, i64=True, f32=True)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        a_s, c_s = hip_ops.host_ints(vals, cuda, i32=True, f32=True)
    torch.cuda.current_stream(cuda).wait_stream(side)
    w32, w64, wf = torch.tensor(vals, dtype=torch.int32), torch.tensor(vals, dtype=torch.int64), torch.tensor(vals, dtype=torch.float32)
    for got, want in ((a, w32), (a3, w32), (a_s, w32), (b, torch.tensor(wide, dtype=torch.int64)), (b3, w64), (c, wf), (c3, wf), (c_s, wf)):
        assert got.dtype == want.dtype and got.shape == (n,) and got.device.type == "cuda"
        assert torch.equal(got.cpu(), want)
    if n > 4:
        assert 2 ** 24 + 1 in vals and float(wf[vals.index(2 ** 24 + 1)]) == 2.0 ** 24     # rounded as torch.tensor rounds it
