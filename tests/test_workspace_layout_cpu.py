"""Workspace sizes without a GPU.  Every *_workspace_bytes function below is `layout(shape, nullptr).bytes` of the layout function
its entry point carves the caller's buffer with ("Workspaces"), so the two cannot disagree; what is left to check on
the host is (a) that no size grew against what the library declared before the layouts (tests/golden/workspace_sizes.json,
written by tests/golden/gen_workspace_sizes.py from that library) and (b) that every entry point refuses a buffer one byte short
of its size with DEFTET_EINVAL, before any device call (on a host without a GPU a device call would fail with another status).

The eight tet builders share deftet_builder_workspace_bytes, the largest of their layouts: one byte short of it is refused by the
builder that sets it (the face adjacency, 12 records per tet).  The other builders' own sizes are not public, so for them this
file only proves that a check exists: each refuses one byte short of a single 256-byte line.  That each check compares against
the builder's own layout is by construction (the entry tests the `bytes` of the layout it takes its pointers from) and is what
tests/test_workspace_exact_gpu.py exercises.  No call here is one that could pass its check: the pointers are placeholders."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SIZES = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")))
ROWS = [(f, r) for f, rows in SIZES.items() for r in rows]
SMALL = [(f, r) for f, r in ROWS if not r.get("workload")]


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib
    return _lib.load()


_raw = ctypes.create_string_buffer(1 << 16)
P = ctypes.c_void_p((ctypes.addressof(_raw) + 255) // 256 * 256)      # stands for every device pointer: checked, never followed


def _ints(n, v):
    return (ctypes.c_int * n)(*([v] * n))


def _builders(lib, n_point, T, wsb):
    return [(lib.deftet_tet_adj_share_i32, (P, P, P, n_point, T, P, wsb, None)),
            (lib.deftet_tet_face_adj_i32, (P, P, 0, P, n_point, T, 0, P, wsb, None)),
            (lib.deftet_tet_point_adj_i32, (P, P, P, n_point, T, P, wsb, None)),
            (lib.deftet_colaps_v_f32, (P, P, P, P, n_point, P, wsb, None)),
            (lib.deftet_tet_to_face_i32, (P, P, P, P, P, P, n_point, T, 1, P, wsb, None)),
            (lib.deftet_tet_edges_i64, (P, P, P, P, P, n_point, T, P, wsb, None)),
            (lib.deftet_subdivide_f32, (P, P, P, P, P, P, P, P, P, P, n_point, T, 7, 0, P, wsb, None)),
            (lib.deftet_delete_tet_i64, (P, P, 0.5, P, P, T, 2, P, wsb, None))]


# function -> the (entry, arguments) calls that must be refused, given the shape of its size function and the workspace bytes on offer
ENTRIES = {
    "deftet_nn_index_workspace_bytes": lambda L, w, B, N, M: [
        (L.deftet_nn_index_f32, (P, P, P, B, N, M, P, w, None)), (L.deftet_nn_index_ragged_f32, (P, P, P, B, N, M, _ints(B, N), P, w, None))],
    "deftet_tri_dist_workspace_bytes": lambda L, w, B, Pn, F: [
        (L.deftet_tri_dist_fwd_f32, (P, P, P, P, P, B, Pn, F, P, w, None)), (L.deftet_tri_dist_fwd_order_f32, (P, P, P, P, P, P, B, Pn, F, P, w, None))],
    "deftet_face_edge_adj_workspace_bytes": lambda L, w, F: [(L.deftet_face_edge_adj_f32, (P, P, F, 10, P, w, None))],
    "deftet_face_edge_adj_ragged_workspace_bytes": lambda L, w, B, F: [(L.deftet_face_edge_adj_ragged_f32, (P, P, B, F, _ints(B, F), 10, P, w, None))],
    "deftet_tet_neighbours_workspace_bytes": lambda L, w, T: [(L.deftet_tet_neighbours_i64, (P, P, 2 * T, T, P, P, P, w, None))],
    "deftet_boundary_index_workspace_bytes": lambda L, w, B, Fi: [(L.deftet_boundary_index_i64, (P, P, P, P, P, B, 384, Fi, 1, P, w, None))],
    "deftet_tet_energies_workspace_bytes2": lambda L, w, B, T: [(L.deftet_tet_energies_fwd_f32, (P, P, P, P, B, T, 2, 2, 1.0, P, w, None))],
    "deftet_surface_extract_workspace_bytes": lambda L, w, B, T, ww: [
        (L.deftet_surface_extract_count_f32, (None if ww else P, P if ww else None, P, 300, P, B, T, 1, 0.25, P, P, w, None)),
        (L.deftet_surface_extract_fill_f32, (P, None, 0, None if ww else P, P, P, B, T, 1, 0.25, 4, P, None, P, P, P, w, None))],
    "deftet_surface_weld_workspace_bytes": lambda L, w, V: [(L.deftet_surface_weld_f32, (P, 1, P, None, 0, V, 3, P, P, P, None, P, P, w, None))],
    "deftet_marching_tets_workspace_bytes": lambda L, w, B, T, E: [
        (L.deftet_marching_tets_count_f32, (P, P, P, B, 125, T, E, 0.0, P, P, P, w, None)),
        (L.deftet_marching_tets_fill_f32, (P, P, None, 0, P, P, P, P, B, 125, T, E, 0.0, 5, 5, P, None, P, P, P, P, P, w, None))],
    "deftet_mesh_voxelize_workspace_bytes": lambda L, w, B, F: [(L.deftet_mesh_voxelize_f32, (P, P, P, P, B, 200, F, 33, P, P, P, P, w, None))],
    "deftet_voxel_surface_workspace_bytes": lambda L, w, B, R: [
        (L.deftet_voxel_surface_count_b32, (P, B, R, P, P, w, None)), (L.deftet_voxel_surface_fill_b32, (P, B, R, 4, 4, P, P, P, w, None))],
    "deftet_face_edges_workspace_bytes": lambda L, w, F: [(L.deftet_face_edges_i32, (P, F, 250, P, P, P, w, None))],
    "deftet_sample_points_workspace_bytes": lambda L, w, B, F: [(L.deftet_sample_points_f32, (P, P, P, P, B, F, 64, P, P, P, P, w, None))],
    "deftet_vertex_adjacency_workspace_bytes": lambda L, w, nnz, V: [
        (L.deftet_vertex_adjacency_csr_i32, (P, P, 8, P, nnz, V, 0, P, P, P, P, P, P, P, P, w, None))],
    "deftet_tet_vertex_csr_workspace_bytes": lambda L, w, Bi, V, T: [(L.deftet_tet_vertex_csr_i32, (P, P, P, P, Bi, V, T, P, w, None))],
    "deftet_face_vertex_csr_workspace_bytes": lambda L, w, V, F: [(L.deftet_face_vertex_csr_i32, (P, P, P, P, V, F, P, w, None))],
    "deftet_edge_vertex_csr_workspace_bytes": lambda L, w, V, E: [(L.deftet_edge_vertex_csr_i32, (P, P, P, P, V, E, P, w, None))],
    "deftet_tet_order_coherence_workspace_bytes": lambda L, w, T: [(L.deftet_tet_order_coherence_f32, (P, T, P, P, P, w, None))],
    "deftet_pointvoxel_workspace_bytes": lambda L, w, B, N, R: [
        (L.deftet_avg_voxelize_fwd_f32, (P, P, P, P, P, B, 3, N, R, P, w, None)),
        (L.deftet_voxel_cells_f32, (P, 0, P, P, P, B, N, R, P, w, None)),
        (L.deftet_voxel_cells_from_inds_i32, (P, P, P, P, P, P, B, N, R, P, w, None)),
        (L.deftet_voxel_sample_bwd_vol_f32, (P, P, P, P, None, P, B, 3, R, N, 0, 3, P, w, None)),
        (L.deftet_voxel_sample_bwd_vol_f32, (P, P, P, P, P, P, B, 3, R, N, 0, 3, P, w, None))],
    "deftet_image_sample_workspace_bytes": lambda L, w, B, N, H, W: [
        (L.deftet_image_cells_f32, (P, P, P, P, B, N, H, W, 0, 0, P, w, None)),
        (L.deftet_image_sample_bwd_map_f32, (P, P, P, P, P, B, 3, H, W, N, 0, 3, P, w, None))],
}


def _id(fr):
    return "%s%s" % (fr[0].replace("deftet_", "").replace("_workspace_bytes", ""), tuple(fr[1]["args"]))


@pytest.mark.parametrize("fr", ROWS, ids=_id)
def test_size_did_not_grow(lib, fr):
    name, row = fr
    now = getattr(lib, name)(*row["args"])
    assert now > 0 and now % 256 == 0, now
    if row.get("parent_too_small"):                                    # the library before the layouts declared less than it carved
        assert now >= row["parent"], (now, row)
    else:
        assert now <= row["parent"], (now, row)


def test_every_function_of_the_table_has_its_entries():
    assert set(SIZES) == set(ENTRIES) | {"deftet_builder_workspace_bytes"}


@pytest.mark.parametrize("fr", [fr for fr in SMALL if fr[0] != "deftet_builder_workspace_bytes"], ids=_id)
def test_entry_refuses_one_byte_less(lib, fr):
    name, row = fr
    need = getattr(lib, name)(*row["args"])
    for entry, args in ENTRIES[name](lib, need - 1, *row["args"]):
        assert entry(*args) == EINVAL, lib.deftet_last_error()
        assert b"workspace" in lib.deftet_last_error()


@pytest.mark.parametrize("fr", [fr for fr in SMALL if fr[0] == "deftet_builder_workspace_bytes"], ids=_id)
def test_builders_refuse_less_than_their_layout(lib, fr):
    n_point, T = fr[1]["args"]
    need = lib.deftet_builder_workspace_bytes(n_point, T)
    assert lib.deftet_tet_face_adj_i32(P, P, 0, P, n_point, T, 0, P, need - 1, None) == EINVAL      # the largest layout, not more
    assert b"workspace" in lib.deftet_last_error()
    for entry, args in _builders(lib, n_point, T, 255):
        assert entry(*args) == EINVAL, lib.deftet_last_error()
        assert b"workspace" in lib.deftet_last_error()
