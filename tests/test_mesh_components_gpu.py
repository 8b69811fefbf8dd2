"""Mesh components, their measures and the mesh clean-up on the GPU (hip_ops.mesh_components / mesh_cleanup / mesh_cleanup_list,
deftet_amd/csrc/mesh_components.hip) against the numpy / scipy reference (tests/mesh_components_ref.py) on the
meshes of tests/mesh_components_cases.py: every integer result bit-equal, the float64 measures inside the worst case of any
summation order, the same bytes on every run and at every position of a concatenated list, the selection keyword by keyword, the
gather and its backward as plain copies, the refusals, and the keywords of the three callers end to end.

The measures' bound, per component of n faces: |area - ref| <= (n + 16) 2^-53 S_area, S_area = sum |b-a| |c-a|, and
|volume - ref| <= (n + 16) 2^-53 S_vol, S_vol = sum |a| |b| |c| — n - 1 additions of non-negative magnitudes bounded by S in any
order, plus the roundings inside one term (under 16 for either formula), against an fsum reference that is exact to one rounding."""
import numpy as np
import pytest
import torch

from tests import mesh_components_cases as K
from tests import mesh_components_ref as ref
from tests.tol import check_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = tuple(K.CASES)
CONNECTIVITY = ("edge", "vertex")
INT_FIELDS = ("labels", "count", "n_face", "boundary_edges", "nonmanifold_edges", "misoriented_edges")


@pytest.fixture(scope="module")
def ops(cuda):
    from deftet_amd import hip_ops
    return hip_ops


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return None if x is None else x.detach().cpu().numpy()


def attrs(name, C):
    v, _f = K.case(name)
    return np.random.default_rng([7, C]).normal(size=(v.shape[0], C)).astype(np.float32)


def components(ops, name, connectivity="edge", **kw):
    v, f = K.case(name)
    return ops.mesh_components(dev(f), v.shape[0], dev(v), connectivity=connectivity, **kw)


def assert_clean_equals(got, want, v, a=None):
    """CleanMesh against ref.Clean: the integers bit for bit, the rows plain copies"""
    assert np.array_equal(host(got.face_map), want.face_map) and np.array_equal(host(got.vertex_map), want.vertex_map)
    assert got.faces.dtype == torch.int64 and np.array_equal(host(got.faces), want.faces)
    assert host(got.verts).tobytes() == v[want.vertex_map].tobytes()
    if a is not None:
        assert host(got.attr).tobytes() == a[want.vertex_map].tobytes()


# ---------------------------------------------------------------------------- integers
@pytest.mark.parametrize("connectivity", CONNECTIVITY)
@pytest.mark.parametrize("name", NAMES)
def test_integer_results_are_bit_equal(ops, name, connectivity):
    v, f = K.case(name)
    want = K.reference(name, connectivity)
    got = components(ops, name, connectivity)
    for field in INT_FIELDS:
        g = getattr(got, field)
        assert g.dtype == torch.int32 and np.array_equal(host(g).astype(np.int64), getattr(want, field)), field
    assert np.array_equal(host(got.closed), want.closed)
    if f.shape[0] == 0:
        return
    V = v.shape[0]
    clean = ops.mesh_cleanup(dev(v), dev(f), connectivity=connectivity)                   # nothing selected: compaction alone
    assert_clean_equals(clean, ref.cleanup(f, V, want), v)
    largest = ops.mesh_cleanup(dev(v), dev(f), keep_largest=True, connectivity=connectivity)
    assert_clean_equals(largest, ref.cleanup(f, V, want, keep_largest=True), v)


def test_a_mesh_without_faces(ops):
    v, f = K.case("empty")
    got = ops.mesh_components(dev(f), 4)
    assert got.labels.shape == (0,) and got.count.tolist() == [0] and got.area is None and got.closed.shape == (0,)
    clean = ops.mesh_cleanup(dev(v), dev(f), keep_largest=True, drop_voids=True, return_components=True)
    assert torch.equal(clean.verts, dev(v)) and clean.faces.shape == (0, 3) and clean.vertex_map.tolist() == [0, 1, 2, 3]
    assert clean.face_map.shape == (0,) and clean.components.count.tolist() == [0]


# ---------------------------------------------------------------------------- measures
@pytest.mark.parametrize("connectivity", CONNECTIVITY)
@pytest.mark.parametrize("name", [n for n in NAMES if n != "empty"])
def test_measures_stay_inside_the_summation_bound(ops, name, connectivity):
    want = K.reference(name, connectivity)
    got = components(ops, name, connectivity)
    assert got.area.dtype == torch.float64 and got.volume.dtype == torch.float64
    scale = (want.n_face + 16.0) * 2.0 ** -53 * (want.n_face > 0)
    ua = check_bound("%s area" % name, got.area, want.area, scale * want.S_area)
    uv = check_bound("%s volume" % name, got.volume, want.volume, scale * want.S_vol)
    print("%s (%s): area uses %.4f of its bound, volume %.4f" % (name, connectivity, ua, uv))


# ---------------------------------------------------------------------------- the same bits
def _bytes(t):
    return None if t is None else host(t).tobytes()


@pytest.mark.parametrize("name", ("hollow", "chunks", "singles"))
def test_two_runs_give_the_same_bytes(ops, name):
    v, f = K.case(name)
    a = attrs(name, 3)
    runs = []
    for _ in range(2):
        c = components(ops, name)
        m = ops.mesh_cleanup(dev(v), dev(f), dev(a), keep_largest=True, drop_voids=True, min_faces=2, return_components=True)
        runs.append([_bytes(x) for x in tuple(c) + tuple(m[:5]) + tuple(m.components)])
    assert runs[0] == runs[1]


LIST = ("hollow", "single", "chunks", "empty", "two_copies")
OPTIONS = dict(drop_voids=True, min_faces=2, keep_largest=True, largest_by="area")


def test_a_shape_alone_and_inside_a_list(ops):
    meshes = [K.case(n) for n in LIST]
    at = [attrs(n, 2) for n in LIST]
    out, vmaps, fmaps = ops.mesh_cleanup_list([dev(v) for v, _f in meshes], [dev(f) for _v, f in meshes], [dev(a) for a in at],
                                              return_maps=True, **OPTIONS)
    for k, name in enumerate(LIST):
        v, f = meshes[k]
        alone = ops.mesh_cleanup(dev(v), dev(f), dev(at[k]), **OPTIONS)
        for x, y in ((out.verts[k], alone.verts), (out.faces[k], alone.faces), (out.vert_attr[k], alone.attr), (vmaps[k], alone.vertex_map),
                     (fmaps[k], alone.face_map)):
            assert x.dtype == y.dtype and x.shape == y.shape and _bytes(x) == _bytes(y), name
        if f.shape[0]:
            want = ref.cleanup(f, v.shape[0], K.reference(name), **OPTIONS)
            assert_clean_equals(alone, want, v, at[k])
    assert torch.equal(out.verts[3], dev(meshes[3][0])) and out.faces[3].shape == (0, 3)   # the empty shape: as it is
    # the measures themselves, at every position of one concatenated list
    live = [k for k in range(len(LIST)) if meshes[k][1].shape[0]]
    voff = np.cumsum([0] + [meshes[k][0].shape[0] for k in live])
    foff = np.cumsum([0] + [meshes[k][1].shape[0] for k in live])
    v = np.concatenate([meshes[k][0] for k in live])
    f = np.concatenate([meshes[k][1] + voff[i] for i, k in enumerate(live)])
    both = ops.mesh_components(dev(f), v.shape[0], dev(v), face_offsets=foff.tolist(), vertex_offsets=voff.tolist())
    for i, k in enumerate(live):
        alone = components(ops, LIST[k])
        rows = slice(int(foff[i]), int(foff[i + 1]))
        assert _bytes(both.area[rows]) == _bytes(alone.area) and _bytes(both.volume[rows]) == _bytes(alone.volume), LIST[k]
        assert torch.equal(both.labels[rows] - int(foff[i]), alone.labels) and torch.equal(both.n_face[rows], alone.n_face)
        assert int(both.count[i]) == int(alone.count[0])


# ---------------------------------------------------------------------------- selection
def _between(values):
    """a threshold that no value is close to: the middle of the widest gap between neighbours of the sorted distinct values"""
    s = np.unique(values)
    k = int(np.argmax(np.diff(s)))
    return float(0.5 * (s[k] + s[k + 1]))


@pytest.mark.parametrize("name", ("hollow", "two_copies", "chunks"))
def test_every_keyword_alone_and_all_together(ops, name):
    v, f = K.case(name)
    V = v.shape[0]
    want = K.reference(name)
    roots = np.nonzero(want.n_face)[0]
    min_area = _between(want.area[roots])
    min_faces = int(np.ceil(_between(want.n_face[roots].astype(np.float64)))) if np.unique(want.n_face[roots]).size > 1 else 21
    singles = [dict(drop_voids=True), dict(min_faces=min_faces), dict(min_area=min_area), dict(keep_largest=True),
               dict(keep_largest=True, largest_by="area")]
    together = dict(drop_voids=True, min_faces=2, min_area=float(want.area[roots].min()) * 0.5, keep_largest=True)
    for kw in singles + [together]:
        got = ops.mesh_cleanup(dev(v), dev(f), return_components=True, **kw)
        expect = ref.cleanup(f, V, want, **kw)
        assert_clean_equals(got, expect, v)
        assert np.array_equal(host(got.components.labels).astype(np.int64), want.labels), kw
        print("%s %s: %d of %d faces, %d of %d vertices" % (name, kw, expect.face_map.size, f.shape[0], expect.vertex_map.size, V))


def test_hollow_selection_counts_and_ties(ops):
    v, f = K.case("hollow")
    pieces = lambda m: torch.unique(m.components.labels[m.face_map]).numel()
    drop = ops.mesh_cleanup(dev(v), dev(f), drop_voids=True, return_components=True)
    assert pieces(drop) == 4 and drop.faces.shape[0] == 8240 - 1716
    more = ops.mesh_cleanup(dev(v), dev(f), drop_voids=True, min_faces=100, return_components=True)
    assert pieces(more) == 3 and more.faces.shape[0] == 5960 + 288 + 204
    shell = ops.mesh_cleanup(dev(v), dev(f), keep_largest=True, return_components=True)
    assert pieces(shell) == 1 and shell.faces.shape[0] == 5960 and int(shell.faces.max()) == shell.verts.shape[0] - 1
    # equal face counts: the smaller label; by area the copies differ and the larger one wins wherever it stands
    v2, f2 = K.case("two_copies")
    assert ops.mesh_cleanup(dev(v2), dev(f2), keep_largest=True).face_map.tolist() == list(range(20))
    swapped = np.concatenate([f2[20:], f2[:20]])
    assert ops.mesh_cleanup(dev(v2), dev(swapped), keep_largest=True).face_map.tolist() == list(range(20))
    assert ops.mesh_cleanup(dev(v2), dev(swapped), keep_largest=True, largest_by="area").face_map.tolist() == list(range(20, 40))
    assert ops.mesh_cleanup(dev(v2), dev(swapped), drop_voids=True).face_map.tolist() == list(range(20, 40))


# ---------------------------------------------------------------------------- gather
@pytest.mark.parametrize("C", (1, 3, 8))
def test_gather_and_its_backward_are_plain_copies(ops, C):
    v, f = K.case("hollow")
    a = attrs("hollow", C)
    V = v.shape[0]
    tv, ta = dev(v).requires_grad_(True), dev(a).requires_grad_(True)
    m = ops.mesh_cleanup(tv, dev(f), ta, keep_largest=True)
    assert torch.equal(m.verts, tv.detach().index_select(0, m.vertex_map)) and torch.equal(m.attr, ta.detach().index_select(0, m.vertex_map))
    assert 0 < m.verts.shape[0] < V and m.attr.shape == (m.verts.shape[0], C)
    rng = np.random.default_rng(C)
    gv, ga = dev(rng.normal(size=tuple(m.verts.shape)).astype(np.float32)), dev(rng.normal(size=tuple(m.attr.shape)).astype(np.float32))

    def scatter(g, width):
        return torch.zeros(V, width, device=DEV).index_copy_(0, m.vertex_map, g)
    dv, da = torch.autograd.grad([m.verts, m.attr], [tv, ta], [gv, ga], retain_graph=True)
    assert _bytes(dv) == _bytes(scatter(gv, 3)) and _bytes(da) == _bytes(scatter(ga, C))
    dropped = torch.ones(V, dtype=torch.bool, device=DEV)
    dropped[m.vertex_map] = False
    assert bool((dv[dropped] == 0).all()) and bool((da[dropped] == 0).all()) and not bool(torch.signbit(dv[dropped]).any())
    # only one of the two output gradients is supplied
    dv1, da1 = torch.autograd.grad([m.verts], [tv, ta], [gv], retain_graph=True, allow_unused=True)
    assert _bytes(dv1) == _bytes(dv) and (da1 is None or not bool(da1.any()))
    dv2, da2 = torch.autograd.grad([m.attr], [tv, ta], [ga], allow_unused=True)
    assert _bytes(da2) == _bytes(da) and (dv2 is None or not bool(dv2.any()))


# ---------------------------------------------------------------------------- refusals: plain argument errors
def test_refusals(ops):
    from deftet_amd import _lib
    v, f = K.case("tetrahedron")
    tv, tf = dev(v), dev(f)
    bad = f.copy()
    bad[2, 1] = 4
    with pytest.raises(IndexError):
        ops.mesh_components(dev(bad), 4)
    with pytest.raises(IndexError):
        ops.mesh_cleanup(tv, dev(bad), keep_largest=True)
    bad[2, 1] = -1
    with pytest.raises(IndexError):
        ops.mesh_components(dev(bad), 4, connectivity="vertex")
    twice = f.copy()
    twice[1, 2] = twice[1, 0]
    with pytest.raises(ValueError):
        ops.mesh_components(dev(twice), 4)
    with pytest.raises(ValueError):
        ops.mesh_cleanup(tv, dev(twice))
    ops.mesh_components(dev(twice), 4, check=False)                                      # the flags are not read: no error
    for wrong in (tf.reshape(-1), tf[:, :2], tf.float(), tf.reshape(2, 2, 3)):
        with pytest.raises(RuntimeError):
            ops.mesh_components(wrong, 4)
    for wrong in (tv[:3], tv.double(), tv[:, :2]):
        with pytest.raises(RuntimeError):
            ops.mesh_components(tf, 4, verts=wrong)
    for wrong in (tv.double(), tv[:, :2], tv.reshape(-1)):
        with pytest.raises(RuntimeError):
            ops.mesh_cleanup(wrong, tf)
    for wrong in (tv[:3], tv.double(), torch.zeros(4, 9, device=DEV), torch.zeros(4, device=DEV)):
        with pytest.raises(RuntimeError):
            ops.mesh_cleanup(tv, tf, wrong)
    for cpu in ((tv, tf.cpu(), None), (tv.cpu(), tf, None), (tv, tf, tv.cpu())):
        with pytest.raises(_lib.DefTetHipError):
            ops.mesh_cleanup(*cpu)
    with pytest.raises(_lib.DefTetHipError):
        ops.mesh_components(tf.cpu(), 4)
    with pytest.raises(ValueError):
        ops.mesh_components(tf, 2 ** 31)
    with pytest.raises(ValueError):
        ops.mesh_components(tf, 4, face_offsets=[0, 4])
    with pytest.raises(ValueError):
        ops.mesh_components(tf, 4, face_offsets=[0, 3], vertex_offsets=[0, 4])
    with pytest.raises(ValueError):
        ops.mesh_cleanup(tv, tf, min_area=-1.0)
    with pytest.raises(RuntimeError):
        ops.mesh_cleanup_list(ops.IsoMesh([tv], [tf], None, None, None, None), [tf])


# ---------------------------------------------------------------------------- the keywords end to end
class HollowModel:
    """the attributes and methods the marching-tetrahedra routes read of a render model; feature 0 is the hollow field"""

    def __init__(self):
        pos, tets, _e, _te, field = K.hollow_grid(40)
        self.tfpoint_px3 = dev(pos[0])
        self.tfpointmov_px3 = torch.zeros_like(self.tfpoint_px3).requires_grad_(True)
        feat = np.random.default_rng(6).normal(size=(pos.shape[1], 4)).astype(np.float32)
        feat[:, 0] = field
        self.tfpointfeat_pxd = dev(feat).requires_grad_(True)
        self.tftet_tx4 = dev(tets)
        self.tets = tets

    def get_point(self, with_coef=False):
        return self.tfpoint_px3 + self.tfpointmov_px3

    def get_feat(self):
        return self.tfpointfeat_pxd


def hollow_process(points, feat):
    return feat[:, :1], torch.sigmoid(feat[:, 1:4])


@pytest.fixture(scope="module")
def model(ops):
    return HollowModel()


def test_render_marching_tets_keywords(ops, model):
    from deftet_amd.render import iso_surface
    base = iso_surface.marching_tets(model, 0.0, hollow_process, return_index=True)
    off = iso_surface.marching_tets(model, 0.0, hollow_process, return_index=True, keep_largest=False, min_faces=0, drop_voids=False)
    assert base.faces.shape[0] == 8240 and base.verts.shape[0] == 4130
    for x, y in zip(base, off):
        assert _bytes(x) == _bytes(y)                                                    # the defaults: byte for byte what it was
    shell = iso_surface.marching_tets(model, 0.0, hollow_process, return_index=True, keep_largest=True)
    maps = ops.mesh_cleanup(base.verts.detach(), base.faces, keep_largest=True)
    assert shell.faces.shape[0] == 5960 and torch.equal(shell.faces, maps.faces)
    assert torch.equal(shell.verts, base.verts[maps.vertex_map]) and torch.equal(shell.vert_attr, base.vert_attr[maps.vertex_map])
    assert torch.equal(shell.edge_id, base.edge_id[maps.vertex_map]) and torch.equal(shell.t, base.t[maps.vertex_map])
    assert torch.equal(shell.tet_id, base.tet_id[maps.face_map])
    assert bool((shell.edge_id[1:] > shell.edge_id[:-1]).all()) and bool((shell.tet_id[1:] >= shell.tet_id[:-1]).all())   # orders survive
    gm, gf = torch.autograd.grad(shell.verts.square().sum() + shell.vert_attr.sum(), (model.tfpointmov_px3, model.tfpointfeat_pxd))
    assert bool(torch.isfinite(gm).all()) and float(gm.abs().max()) > 0 and float(gf.abs().max()) > 0
    fine = iso_surface.marching_tets(model, 0.0, hollow_process, subdivide=1, keep_largest=True)
    assert fine.faces.shape[0] == 4 * 5960
    want = ops.loop_subdivide_mesh(shell.verts, shell.faces, shell.vert_attr)
    assert torch.equal(fine.verts, want[0]) and torch.equal(fine.faces, want[1])          # cleaned BEFORE the subdivision
    normals = iso_surface.marching_tets_normals(model, 0.0, hollow_process, drop_voids=True, min_faces=100)
    assert normals.faces.shape[0] == 5960 + 288 + 204 and normals.vert_attr.shape == normals.verts.shape


def test_deftet_iso_surface_keywords(ops):
    from deftet_amd.layers.DefTet.deftet import DefTet, clear_topology_cache
    from tests import marching_tets_cases as MK
    pos, tets, _e, _te = MK.grid(16, 1)
    B = 2
    pos = np.repeat(pos, B, axis=0)
    cent = pos[:, tets].mean(2)
    ball = lambda b, c, r: np.clip(0.5 + 3.0 * (1.0 - np.linalg.norm(cent[b] - np.asarray(c, np.float32), axis=1) / r), 0.0, 1.0)
    # a ball and a floater per shape: 576 + 24 faces and 180 + 144 on the CPU restatement of the route
    occ = np.stack([np.maximum(ball(0, (-.1, -.1, -.1), 0.3), ball(0, (.33, .33, .33), 0.12)),
                    np.maximum(ball(1, (-.1, -.1, -.1), 0.2), ball(1, (.28, .28, .28), 0.16))]).astype(np.float32)
    tets_b = dev(np.repeat(tets[None], B, axis=0))
    layer = DefTet()
    p, o = dev(pos).requires_grad_(True), dev(occ[:, :, None]).requires_grad_(True)
    base = layer.iso_surface(p, tets_b, o, iso=0.5)
    off = layer.iso_surface(p, tets_b, o, iso=0.5, keep_largest=False, min_faces=0, drop_voids=False)
    clean = layer.iso_surface(p, tets_b, o, iso=0.5, drop_voids=True, min_faces=100)
    dropped = 0
    for b in range(B):
        assert _bytes(base.verts[b]) == _bytes(off.verts[b]) and _bytes(base.faces[b]) == _bytes(off.faces[b])
        v, f = host(base.verts[b]), host(base.faces[b])
        comps = ref.components(f, v.shape[0], v)
        assert int(comps.count[0]) >= 2, "the input of this test has a floater in every shape"
        want = ref.cleanup(f, v.shape[0], comps, drop_voids=True, min_faces=100)
        assert np.array_equal(host(clean.faces[b]), want.faces) and _bytes(clean.verts[b]) == v[want.vertex_map].tobytes()
        alone = ops.mesh_cleanup(base.verts[b], base.faces[b], drop_voids=True, min_faces=100)
        assert _bytes(alone.verts) == _bytes(clean.verts[b]) and torch.equal(alone.faces, clean.faces[b])
        dropped += f.shape[0] - want.face_map.size
    assert dropped > 0
    gp, go = torch.autograd.grad(sum(v.square().sum() for v in clean.verts), (p, o))
    assert bool(torch.isfinite(gp).all()) and float(gp.abs().max()) > 0 and float(go.abs().max()) > 0
    fine = layer.iso_surface(p, tets_b, o, iso=0.5, drop_voids=True, min_faces=100, subdivide=1)
    assert [int(x.shape[0]) for x in fine.faces] == [4 * int(x.shape[0]) for x in clean.faces]
    clear_topology_cache()


def test_save_surface_objs_keywords(ops, model, tmp_path):
    from deftet_amd.render import export
    nbr = ops.tet_face_neighbours(model.tets, model.tfpoint_px3.shape[0], torch.device(DEV))
    w, col = hollow_process(model.get_point(True), model.get_feat())
    for d in ("a", "b", "c"):
        (tmp_path / d).mkdir()
    args = (model.get_point(True), (w, col), model.tets, nbr)
    old = export.save_surface_objs(*args, str(tmp_path / "a"), "s", thresholds=(0.02,), iso=0.0)
    off = export.save_surface_objs(*args, str(tmp_path / "b"), "s", thresholds=(0.02,), iso=0.0, iso_keep_largest=False, iso_min_faces=0,
                                   iso_drop_voids=False)
    new = export.save_surface_objs(*args, str(tmp_path / "c"), "s", thresholds=(0.02,), iso=0.0, iso_keep_largest=True)
    read = lambda path: open(path, "rb").read()
    count = lambda path, tag: sum(1 for line in open(path) if line.startswith(tag))
    assert [q.rsplit("/", 1)[1] for q in old] == [q.rsplit("/", 1)[1] for q in new] and len(old) == 4
    for k in range(4):
        assert read(old[k]) == read(off[k])                                              # the defaults: byte-identical files
    for k in (0, 1):
        assert read(old[k]) == read(new[k]) and count(old[k], "f ") > 0                  # the tet- files are left alone
    for k in (2, 3):
        assert count(old[k], "f ") == 8240 and count(new[k], "f ") == 5960 and count(new[k], "v ") == 5960 // 2 + 2
        assert len(read(new[k])) < len(read(old[k]))
