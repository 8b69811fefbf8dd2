"""CPU tests of the ground-truth preparation operators: the numpy restatement (tests/dataprep_ref.py) checks
itself on shapes whose answer is known, the fp32 and fp64 voxelizations stay inside the cap the GPU test relies on, the C ABI
carries the new symbols, and the overlay resolves the six Kaolin names with Kaolin's parameter names."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import dataprep_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["deftet_mesh_voxelize_workspace_bytes", "deftet_mesh_voxelize_f32", "deftet_voxel_pack_u8", "deftet_voxel_unpack_u8",
               "deftet_extract_odms_u8", "deftet_project_odms_i32", "deftet_voxel_fill_workspace_bytes", "deftet_voxel_fill_b32",
               "deftet_voxel_surface_workspace_bytes", "deftet_voxel_surface_count_b32", "deftet_voxel_surface_fill_b32",
               "deftet_face_edges_workspace_bytes", "deftet_face_edges_i32"]
KAOLIN_NAMES = {"kaolin.ops.conversions": {"trianglemeshes_to_voxelgrids": ["vertices", "faces", "resolution", "origin", "scale", "return_sparse"],
                                           "voxelgrids_to_trianglemeshes": ["voxelgrids", "iso_value"]},
                "kaolin.ops.voxelgrid": {"extract_odms": None, "project_odms": ["odms", "voxelgrids", "votes"]},
                "kaolin.ops.mesh": {"adjacency_matrix": ["num_vertices", "faces", "sparse"], "face_normals": ["face_vertices", "unit"]}}


def test_one_axis_aligned_triangle_in_a_unit_voxel():
    v = np.array([[[0.25, 0.25, 0.5], [0.75, 0.25, 0.5], [0.25, 0.75, 0.5]]], np.float32)
    f = np.array([[0, 1, 2]])
    zero, one = np.zeros((1, 3), np.float32), np.ones(1, np.float32)
    assert ref.mesh_voxelize_f32(v, f, 1, zero, one).tolist() == [[[[1]]]]
    vox = ref.mesh_voxelize_f32(v, f, 4, zero, one)                    # q in [1,3] x [1,3] at z = 2: the lattice plane between k = 1, 2
    want = np.zeros((4, 4, 4), np.uint8)
    for i in range(4):
        for j in range(4):
            # closed boxes: voxel (i, j) touches the triangle x >= 1, y >= 1, x + y <= 4 iff its nearest corner does
            if i + 1 >= 1 and j + 1 >= 1 and max(i, 1) + max(j, 1) <= 4:
                want[i, j, 1:3] = 1
    assert np.array_equal(vox[0], want)
    v64, near = ref.mesh_voxelize_f64(v, f, 4, zero, one)
    assert np.array_equal(v64, vox) and near[0][want == 1].any()       # touching decisions have margin 0


def test_a_triangle_in_a_lattice_plane_sets_both_sides():
    v = np.array([[[0.125, 0.125, 0.5], [0.375, 0.125, 0.5], [0.125, 0.375, 0.5]]], np.float32)
    vox = ref.mesh_voxelize_f32(v, np.array([[0, 1, 2]]), 2, np.zeros((1, 3), np.float32), np.ones(1, np.float32))
    assert vox[0, 0, 0].tolist() == [1, 1] and vox.sum() == 2


def test_degenerate_nan_and_outside_triangles():
    zero, one = np.zeros((1, 3), np.float32), np.ones(1, np.float32)
    seg = np.array([[[0.125, 0.125, 0.125], [0.875, 0.125, 0.125], [0.5, 0.125, 0.125]]], np.float32)      # zero area: a segment
    assert ref.mesh_voxelize_f32(seg, np.array([[0, 1, 2]]), 4, zero, one)[0, :, 0, 0].tolist() == [1, 1, 1, 1]
    nan = seg.copy()
    nan[0, 1, 1] = np.nan
    assert ref.mesh_voxelize_f32(nan, np.array([[0, 1, 2]]), 4, zero, one).sum() == 0
    assert ref.mesh_voxelize_f32(seg + 2.0, np.array([[0, 1, 2]]), 4, zero, one).sum() == 0


def _block():
    v = np.zeros((1, 6, 6, 6), np.uint8)
    v[0, 1:3, 2:5, 1:5] = 1
    return v


def test_solid_block_gives_52_quads_and_its_volume():
    verts, faces = ref.voxel_surface_mesh(_block())
    assert faces[0].shape == (2 * 52, 3) and verts[0].shape == (3 * 4 * 5 - 1 * 2 * 3, 3)
    assert ref.signed_volume(verts[0], faces[0]) == 24.0
    assert ref.directed_edge_imbalance(faces[0]) == 0
    e = np.concatenate([faces[0][:, [0, 1]], faces[0][:, [1, 2]], faces[0][:, [2, 0]]])
    assert np.unique(e, axis=0).shape[0] == e.shape[0]                  # every directed edge once, its reverse once
    assert np.array_equal(np.unique(verts[0], axis=0), verts[0])        # ascending corner key
    # rows come in (voxel, direction) order: a quad lies between its lowest corner's voxel and the one below it along the
    # quad's normal axis; exactly one of the two is occupied, and that voxel's linear index never decreases
    g = np.pad(_block()[0], 1)                                          # (index + 1: the voxel below may be outside)
    quad = verts[0][faces[0].reshape(52, 6)].astype(np.int64)
    lo, flat = quad.min(axis=1), quad.min(axis=1) == quad.max(axis=1)
    assert (flat.sum(axis=1) == 1).all()
    below = lo - flat
    occ_lo, occ_below = g[tuple((lo + 1).T)] == 1, g[tuple((below + 1).T)] == 1
    assert (occ_lo != occ_below).all()
    vox = np.where(occ_lo[:, None], lo, below)
    lin = (vox[:, 0] * 6 + vox[:, 1]) * 6 + vox[:, 2]
    assert (np.diff(lin) >= 0).all() and np.unique(lin).shape[0] == 24
    d = 2 * np.argmax(flat, axis=1) + occ_below                         # towards +axis iff the occupied voxel is the lower one
    assert (np.diff(lin * 6 + d) > 0).all()


def test_edge_and_corner_contacts_stay_closed():
    for other in ((1, 1, 0), (1, 1, 1)):
        v = np.zeros((1, 3, 3, 3), np.uint8)
        v[0, 0, 0, 0] = v[0][other] = 1
        verts, faces = ref.voxel_surface_mesh(v)
        assert faces[0].shape[0] == 24 and ref.signed_volume(verts[0], faces[0]) == 2.0
        assert ref.directed_edge_imbalance(faces[0]) == 0
        assert verts[0].shape[0] == (14 if other == (1, 1, 0) else 15)


def test_projection_keeps_a_solid_box_and_fills_a_hollow_one():
    solid = _block()
    assert np.array_equal(ref.project_odms(ref.extract_odms(solid)), solid)
    hollow = np.zeros((1, 7, 7, 7), np.uint8)
    hollow[0, 1:6, 1:6, 1:6] = 1
    full = hollow.copy()
    hollow[0, 2:5, 2:5, 2:5] = 0
    assert np.array_equal(ref.project_odms(ref.extract_odms(hollow)), full)
    o = ref.extract_odms(solid)
    assert o.shape == (1, 6, 6, 6) and o[0, 0, 2, 1] == 1 and o[0, 1, 2, 1] == 3 and o[0, 4, 1, 2] == 1 and o[0, 5, 1, 2] == 1
    assert o[0, 2, 1, 1] == 2 and o[0, 3, 1, 1] == 1 and o[0, 0, 0, 0] == 6
    # votes = 6: only a voxel whose three rays all miss the block is carved six times; the union of the three shadows stays
    assert ref.project_odms(o, votes=6).sum() == 72 + 48 + 36 - 3 * 24 + 24 and ref.project_odms(o, votes=1, voxelgrids=np.zeros_like(solid)).sum() == 0


def test_edges_of_a_tetrahedron():
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    p = ref.face_edges(f, 4)
    assert p.tolist() == [[a, b] for a in range(4) for b in range(4) if a != b]
    offs, cols = ref.edge_csr(f, 5)
    assert offs.tolist() == [0, 3, 6, 9, 12, 12] and cols[:3].tolist() == [1, 2, 3]


def test_fp32_and_fp64_references_stay_inside_the_cap_on_the_icosphere():
    v, f = ref.icosphere(2, seed=5)
    for R in (33, 100):
        v32 = ref.mesh_voxelize_f32(v[None], f, R)
        v64, near = ref.mesh_voxelize_f64(v[None], f, R)
        assert not ((v32 != v64) & ~near).any()
        assert near.sum() <= 0.005 * v32.sum(), (R, int(near.sum()), int(v32.sum()))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(deftet_\w+)\s*\(", txt))


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from deftet_amd import _lib, build
    build.build()
    syms = header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s), s
    loaded = _lib.load()
    assert loaded.deftet_version() >= 310
    assert loaded.deftet_voxel_surface_workspace_bytes(1, 100) > 101 * 101 * 4 * 8
    st = loaded.deftet_mesh_voxelize_f32(None, None, None, None, 1, 0, 0, 0, None, None, None, None, 0, None)
    assert st == -1 and b"resolution" in loaded.deftet_last_error()
    st = loaded.deftet_project_odms_i32(None, None, 1, 4, 7, None, None)
    assert st == -1 and b"null pointer" in loaded.deftet_last_error()
    # the int32 tables: what the input could fill at most must fit, or the call is refused before anything is launched
    st = loaded.deftet_mesh_voxelize_f32(None, None, None, None, 1, 3, 16384, 1024, None, None, None, None, 0, None)
    assert st == -1 and b"wave tasks" in loaded.deftet_last_error()          # 16,384 triangles x 2^17 tasks = 2^31
    st = loaded.deftet_mesh_voxelize_f32(None, None, None, None, 1, 3, 16383, 1024, None, None, None, None, 0, None)
    assert st == -1 and b"null pointer" in loaded.deftet_last_error()        # one fewer passes that check
    st = loaded.deftet_voxel_surface_count_b32(None, 1, 710, None, None, 0, None)
    assert st == -1 and b"triangles at most" in loaded.deftet_last_error()   # 6 * 710^2 * 711 > 2^31
    st = loaded.deftet_voxel_surface_count_b32(None, 1, 709, None, None, 0, None)
    assert st == -1 and b"null pointer" in loaded.deftet_last_error()


def test_the_six_kaolin_names_resolve_with_kaolins_parameter_names():
    from deftet_amd import dataprep, overlay
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "kaolin" or k.startswith("kaolin.")}
    names = overlay.install(kaolin=True)
    try:
        import importlib
        for mod, funcs in KAOLIN_NAMES.items():
            assert mod in names
            m = importlib.import_module(mod)
            for name, params in funcs.items():
                fn = getattr(m, name)
                assert fn is getattr(dataprep, name), (mod, name)
                if params is not None:
                    assert list(inspect.signature(fn).parameters) == params, name
        from tests import dataprep_callers
        held = dataprep_callers.import_like_reference()
        assert all(held[k] is getattr(dataprep, k) for k in held) and len(held) == 6
        with pytest.raises(NotImplementedError):
            dataprep.trianglemeshes_to_voxelgrids(None, None, 4, return_sparse=True)
        with pytest.raises(NotImplementedError):
            dataprep.adjacency_matrix(4, None, sparse=False)
    finally:
        overlay.uninstall(names)
        sys.modules.update(saved)


def test_face_normals_restatement_and_cpu_refusal():
    from deftet_amd import _lib, dataprep, hip_ops
    fv = torch.tensor([[[[0.0, 0, 0], [2, 0, 0], [0, 3, 0]], [[1.0, 1, 1], [1, 1, 1], [1, 1, 1]]]])
    assert dataprep.face_normals(fv).tolist() == [[[0.0, 0.0, 6.0], [0.0, 0.0, 0.0]]]
    assert dataprep.face_normals(fv, unit=True).tolist() == [[[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]]
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.mesh_voxelize(torch.zeros(1, 3, 3), torch.zeros(1, 3, dtype=torch.long), 4)
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.voxel_fill(torch.zeros(1, 4, 4, 4))
    with pytest.raises(_lib.DefTetHipError):
        dataprep.make_surface_mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long))
