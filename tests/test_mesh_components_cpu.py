"""Mesh components without a GPU: the reference (tests/mesh_components_ref.py) against closed forms on the meshes of
tests/mesh_components_cases.py — areas, volumes and closedness of the tetrahedron, the icosahedron and the five pieces of the
hollow scene, a reversed piece's volume, the label as the smallest face index under renumbering, edge against vertex
connectivity; the header, the ctypes table and the library agree on the six entry points, which refuse bad arguments with their
status codes before any device work; the new keywords default to off; the operators fail loudly without GPU tensors."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import loop_subdiv_cases as LK
from tests import mesh_components_cases as K
from tests import mesh_components_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("deftet_mesh_components_workspace_bytes", "deftet_mesh_components_i64", "deftet_mesh_cleanup_count_i64",
           "deftet_mesh_cleanup_fill_i64", "deftet_mesh_gather_fwd_f32", "deftet_mesh_gather_bwd_f32")


# ---------------------------------------------------------------------------- the reference against closed forms
def test_tetrahedron_and_icosahedron():
    c = K.reference("tetrahedron")                                       # edge 2 sqrt 2: area 4 * sqrt(3)/4 * 8, volume 8/3
    assert c.labels.tolist() == [0] * 4 and c.count.tolist() == [1] and c.closed[0] and c.n_face[0] == 4
    assert abs(c.area[0] - 8 * np.sqrt(3)) < 1e-13 and abs(c.volume[0] - 8.0 / 3.0) < 1e-14
    v, f = LK.case("icosahedron")
    c = ref.components(f, 12, v)
    a = 2.0                                                               # its edge length; 5 sqrt 3 a^2 and 5 (3 + sqrt 5) / 12 a^3
    assert c.closed[0] and c.n_face[0] == 20 and (c.labels == 0).all()
    assert abs(c.area[0] - 5 * np.sqrt(3) * a * a) < 1e-5 and abs(c.volume[0] - 5 * (3 + np.sqrt(5)) / 12 * a ** 3) < 1e-5   # (fp32 vertices)


def test_hollow_has_the_five_pieces():
    v, f = K.case("hollow")
    c = K.reference("hollow")
    assert v.shape[0] == 4130 and f.shape[0] == 8240
    _fe, cnt, same = ref.edge_table(f, v.shape[0])
    assert (cnt == 2).all() and not same.any()                            # every edge has two incidences, running opposite ways
    roots = np.nonzero(c.n_face)[0]
    assert c.count.tolist() == [5] and c.closed[roots].all() and (c.labels[roots] == roots).all()
    assert c.n_face[roots].tolist() == [n for n, _v in K.HOLLOW_ROWS]
    for r, (_n, vol) in zip(roots, K.HOLLOW_ROWS):
        assert abs(c.volume[r] - vol) <= 0.05 * abs(vol), (r, c.volume[r], vol)
    # what the selection leaves
    n = lambda **kw: np.unique(c.labels[ref.cleanup(f, v.shape[0], c, **kw).keep]).size
    assert n(drop_voids=True) == 4 and n(drop_voids=True, min_faces=100) == 3
    only = ref.cleanup(f, v.shape[0], c, keep_largest=True)
    assert only.face_map.size == 5960 and only.faces.max() == only.vertex_map.size - 1 and only.vertex_map.size == 5960 // 2 + 2


def test_reversing_a_piece_flips_its_volume():
    c = K.reference("two_copies")
    assert c.count.tolist() == [2] and c.closed[0] and c.closed[20]
    assert c.volume[0] > 0 and abs(c.volume[20] + c.volume[0] * 0.125) < 1e-5 and abs(c.area[20] - c.area[0] * 0.25) < 1e-5
    v, f = K.case("two_copies")
    drop = ref.cleanup(f, v.shape[0], c, drop_voids=True)
    assert drop.face_map.tolist() == list(range(20)) and drop.vertex_map.tolist() == list(range(12))


@pytest.mark.parametrize("connectivity", ("edge", "vertex"))
def test_label_is_the_smallest_face_under_renumbering(connectivity):
    v, f = K.case("chunks")
    base = ref.labels(f, v.shape[0], connectivity)
    assert sorted(np.bincount(base)[np.unique(base)].tolist()) == sorted(K.CHUNK_SIZES)
    rng = np.random.default_rng(3)
    for _ in range(3):
        perm = rng.permutation(f.shape[0])
        lab = ref.labels(f[perm], v.shape[0], connectivity)
        assert (lab <= np.arange(f.shape[0])).all() and (lab[lab] == lab).all()
        # the same partition, and the label is the smallest member
        for L in np.unique(lab):
            members = np.nonzero(lab == L)[0]
            assert members.min() == L and np.unique(base[perm[members]]).size == 1
        assert np.unique(lab).size == np.unique(base).size


def test_edge_versus_vertex_connectivity():
    v, f = K.case("bowtie")
    assert ref.labels(f, v.shape[0], "edge").tolist() == [0, 1] and ref.labels(f, v.shape[0], "vertex").tolist() == [0, 0]
    c = ref.components(f, v.shape[0], v, "vertex")
    assert c.boundary_edges.tolist() == [6, 0] and c.count.tolist() == [1] and not c.closed.any()
    book = K.reference("book")
    assert book.labels.tolist() == [0, 0, 0] and book.nonmanifold_edges[0] == 1 and book.boundary_edges[0] == 6
    same = K.reference("same_way")
    assert same.labels.tolist() == [0, 0] and same.misoriented_edges[0] == 1 and same.boundary_edges[0] == 4
    one = K.reference("single")
    assert one.boundary_edges.tolist() == [3] and one.area[0] == 0.5 and one.volume[0] == 0.0
    none = K.reference("empty")
    assert none.labels.size == 0 and none.count.tolist() == [0]
    big = K.reference("big_index")
    assert big.closed[0] and big.n_face[0] == 8 and abs(big.volume[0] - 4.0 / 3.0) < 1e-14


def test_selection_and_compaction_in_the_list_form():
    v, f = K.case("two_copies")
    c = ref.components(f, 24, v, face_offsets=[0, 0, 20, 40])
    assert c.count.tolist() == [0, 1, 1]
    out = ref.cleanup(f, 24, c, keep_largest=True, face_offsets=[0, 0, 20, 40], vertex_offsets=[0, 0, 12, 24])
    assert out.face_offsets.tolist() == [0, 0, 20, 40] and out.vertex_offsets.tolist() == [0, 0, 12, 24]
    assert out.faces[20:].min() == 0 and out.faces[20:].max() == 11        # numbered inside their shapes
    tie = ref.cleanup(f, 24, c, keep_largest=True)
    assert tie.face_map.tolist() == list(range(20))                       # equal face counts: the smaller label
    assert ref.cleanup(f, 24, c, keep_largest=True, largest_by="area").face_map.tolist() == list(range(20))
    assert ref.cleanup(f, 24, c, min_area=0.3 * c.area[0]).face_map.size == 20


# ---------------------------------------------------------------------------- the C ABI
def test_header_ctypes_table_and_library_agree():
    from deftet_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    note = re.search(r"^/\* 420:(.*?)\*/", txt, flags=re.S | re.M)
    assert note, "no 420: version note"
    for s in SYMBOLS:
        assert re.sub(r"_(fwd|bwd)_f32$", "", s) in note.group(1), s
    plain = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", plain))
    assert {s for s in declared if "_mesh_c" in s or "_mesh_g" in s} == set(SYMBOLS)      # every new declaration is named above
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % s, plain).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[s][1]), s                      # as many parameters as the table lists
    assert _lib.load().deftet_version() >= 420


def test_entry_points_refuse_bad_arguments():
    from deftet_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    buf = ctypes.create_string_buffer(1 << 20)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed
    err = lib.deftet_last_error
    size = lib.deftet_mesh_components_workspace_bytes
    need = size(6, 8, 1)
    assert need > 0 and need % 256 == 0 and size(6, 8, 3) >= need
    assert size(0, 8, 1) == 256 and size(6, 0, 1) == 256 and size(6, 8, 0) == 256 and size(6, 2 ** 30, 1) == 256
    comp, count, fill = lib.deftet_mesh_components_i64, lib.deftet_mesh_cleanup_count_i64, lib.deftet_mesh_cleanup_fill_i64
    outs, ints = [P] * 9, [P] * 5

    def components(F=8, V=6, verts=P, off=P, S=1, conn=0, outs=outs, ws=P, n=need):
        return comp(P, F, V, verts, off, S, conn, *outs, ws, n, None)
    assert components(F=0) == EINVAL and b"must be positive" in err()
    assert components(V=0) == EINVAL and b"must be positive" in err()
    assert components(F=2 ** 30) == EINVAL and b"31 bits" in err()
    assert components(S=0) == EINVAL and b"n_shape" in err()
    assert components(conn=2) == EINVAL and b"connectivity" in err()
    assert components(off=None) == EINVAL and b"null pointer" in err()
    assert components(outs=[None] + outs[1:]) == EINVAL and b"null pointer" in err()
    assert components(outs=ints + [P, None, P, P]) == EINVAL and b"go together" in err()
    assert components(verts=None) == EINVAL and b"verts goes with" in err()
    assert components(outs=ints + [None, None, P, P]) == EINVAL and b"verts goes with" in err()
    for ws, n in ((None, need), (P, need - 1), (ctypes.c_void_p(P.value + 16), need)):
        assert components(ws=ws, n=n) == EINVAL
        assert b"workspace null, misaligned or too small: need %d bytes" % need in err()

    def cleanup(verts=P, voff=P, keep=0, min_faces=0, min_area=0.0, voids=0, by=0, outs=outs, n=need):
        return count(P, 8, 6, verts, P, voff, 1, 0, keep, min_faces, min_area, voids, by, *outs, P, n, None)
    assert cleanup(voff=None) == EINVAL and b"vertex_offsets" in err()
    assert cleanup(min_faces=-1) == EINVAL and b"negative" in err()
    assert cleanup(min_area=-1.0) == EINVAL and b"negative" in err()
    assert cleanup(min_area=float("nan")) == EINVAL and b"negative" in err()
    assert cleanup(by=2) == EINVAL and b"largest_by" in err()
    no_measures = ints + [None, None, P, P]
    for kw in (dict(voids=1), dict(min_area=0.5), dict(keep=1, by=1)):
        assert cleanup(verts=None, outs=no_measures, **kw) == EINVAL and b"need verts" in err()
    assert cleanup(n=need - 1) == EINVAL and b"workspace" in err()
    assert fill(P, 8, 6, P, P, 1, 0, 3, P, P, P, P, need, None) == EINVAL and b"n_face_out" in err()
    assert fill(P, 8, 6, P, P, 1, 9, 3, P, P, P, P, need, None) == EINVAL and b"n_face_out" in err()
    assert fill(P, 8, 6, P, P, 1, 4, 7, P, P, P, P, need, None) == EINVAL and b"n_vertex_out" in err()
    assert fill(P, 8, 6, P, P, 1, 4, 3, P, None, P, P, need, None) == EINVAL and b"null pointer" in err()
    assert fill(P, 8, 6, P, P, 1, 4, 3, P, P, P, P, need - 1, None) == EINVAL and b"workspace" in err()
    fwd, bwd = lib.deftet_mesh_gather_fwd_f32, lib.deftet_mesh_gather_bwd_f32
    assert fwd(P, None, 0, P, 6, 0, P, None, None) == EINVAL and b"n_vertex_out" in err()
    assert fwd(P, None, 0, P, 6, 7, P, None, None) == EINVAL and b"n_vertex_out" in err()
    assert fwd(P, P, 9, P, 6, 3, P, P, None) == EINVAL and b"n_attr" in err()
    assert fwd(P, None, 3, P, 6, 3, P, P, None) == EINVAL and b"do not go together" in err()
    assert fwd(P, None, 0, None, 6, 3, P, None, None) == EINVAL and b"vertex_map" in err()
    assert fwd(None, None, 0, P, 6, 3, P, None, None) == EINVAL and b"null pointer" in err()
    assert bwd(None, None, 0, P, 6, 3, None, None, None) == EINVAL and b"every output" in err()
    assert bwd(P, None, 0, P, 6, 3, None, None, None) == EINVAL and b"goes with" in err()
    assert bwd(None, P, 0, P, 6, 3, None, P, None) == EINVAL and b"without attributes" in err()


# ---------------------------------------------------------------------------- the front ends
def test_new_keywords_default_to_off():
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    from deftet_amd.render import export, iso_surface
    for fn in (iso_surface.marching_tets, iso_surface.marching_tets_normals, DefTet.iso_surface):
        sig = inspect.signature(fn).parameters
        assert (sig["keep_largest"].default, sig["min_faces"].default, sig["drop_voids"].default) == (False, 0, False), fn
    sig = inspect.signature(export.save_surface_objs).parameters
    assert (sig["iso_keep_largest"].default, sig["iso_min_faces"].default, sig["iso_drop_voids"].default) == (False, 0, False)
    assert (sig["keep_largest"].default, sig["min_component"].default, sig["fill_voids"].default) == (False, 0, False)
    sig = inspect.signature(hip_ops.mesh_components).parameters
    assert list(sig)[:5] == ["faces", "n_vertex", "verts", "connectivity", "check"]
    assert (sig["verts"].default, sig["connectivity"].default, sig["check"].default) == (None, "edge", True)
    for fn, first in ((hip_ops.mesh_cleanup, ["verts", "faces", "attr"]), (hip_ops.mesh_cleanup_list, ["mesh_or_verts", "faces_list", "attr_list"])):
        sig = inspect.signature(fn).parameters
        assert list(sig)[:3] == first
        assert [sig[k].default for k in ("keep_largest", "min_faces", "min_area", "drop_voids", "largest_by", "connectivity")] == \
            [False, 0, 0.0, False, "faces", "edge"], fn
    assert inspect.signature(hip_ops.mesh_cleanup).parameters["return_components"].default is False
    assert hip_ops.MeshComponents._fields == ("labels", "count", "n_face", "area", "volume", "boundary_edges", "nonmanifold_edges",
                                              "misoriented_edges") and isinstance(hip_ops.MeshComponents.closed, property)
    assert hip_ops.CleanMesh._fields == ("verts", "faces", "attr", "vertex_map", "face_map", "components")


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from deftet_amd import _lib, hip_ops
    v, f = (torch.from_numpy(x.copy()) for x in LK.case("octahedron"))
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.mesh_components(f, 6)
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.mesh_components(f, 6, verts=v)
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.mesh_cleanup(v, f, keep_largest=True)
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.mesh_cleanup_list([v], [f], keep_largest=True)
    with pytest.raises(ValueError):
        hip_ops.mesh_components(f, 6, connectivity="face")
    with pytest.raises(ValueError):
        hip_ops.mesh_cleanup(v, f, largest_by="volume")
    with pytest.raises(ValueError):
        hip_ops.mesh_cleanup(v, f, min_faces=-1)
    with pytest.raises(RuntimeError):
        hip_ops.mesh_cleanup_list([v], [f, f])
    # a list without faces: handed back untouched, nothing of the library runs
    vs, fs = [torch.zeros(5, 3)], [torch.zeros(0, 3, dtype=torch.int64)]
    out = hip_ops.mesh_cleanup_list(vs, fs, keep_largest=True)
    assert out.verts[0] is vs[0] and out.faces[0] is fs[0] and out.vert_attr is None and out.edge_id is None
