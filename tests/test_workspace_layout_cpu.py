"""Workspace sizes without a GPU.  Every *_workspace_bytes function below is `layout(shape, nullptr).bytes` of the layout function
its entry point carves the caller's buffer with ("Workspaces"), so the two cannot disagree; what is left to check on
the host is (a) that no size grew against what the library declared before the layouts (tests/golden/workspace_sizes.json,
written by tests/golden/gen_workspace_sizes.py from that library) and (b) that every entry point refuses a buffer one byte short
of its size with DEFTET_EINVAL, before any device call (on a host without a GPU a device call would fail with another status).

Every refusal names the bytes the entry needed and the bytes it was given ("Workspaces": the one wording of
workspace_ok), so the tests read both back: `need` must be the entry's own size, which shows that the entry compared against
the layout it carves and not merely that some check exists, and `got` must be what was offered.  The same entries refuse a
buffer of enough bytes that is 16 bytes off the 256-byte line, and a null one, except where null is the documented selector of
the brute-force path (NULL_SELECTS below).

The eight tet builders share deftet_builder_workspace_bytes, the largest of their layouts (the face adjacency's, 12 records per
tet).  The other builders' own sizes are not public: each states its `need` in the refusal of a call that offers 0 bytes, and
must then refuse `need - 1` as well.  No call here is one that could pass its check: the pointers are placeholders."""
import ctypes
import json
import os
import re

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


def _builders(lib, n_point, T, ws, wsb):
    return [(lib.deftet_tet_adj_share_i32, (P, P, P, n_point, T, ws, wsb, None)),
            (lib.deftet_tet_face_adj_i32, (P, P, 0, P, n_point, T, 0, ws, wsb, None)),
            (lib.deftet_tet_point_adj_i32, (P, P, P, n_point, T, ws, wsb, None)),
            (lib.deftet_colaps_v_f32, (P, P, P, P, n_point, ws, wsb, None)),
            (lib.deftet_tet_to_face_i32, (P, P, P, P, P, P, n_point, T, 1, ws, wsb, None)),
            (lib.deftet_tet_edges_i64, (P, P, P, P, P, n_point, T, ws, wsb, None)),
            (lib.deftet_subdivide_f32, (P, P, P, P, P, P, P, P, P, P, n_point, T, 7, 0, ws, wsb, None)),
            (lib.deftet_delete_tet_i64, (P, P, 0.5, P, P, T, 2, ws, wsb, None))]


# function -> the (entry, arguments) calls that must be refused, given the shape of its size function and the workspace bytes on offer
ENTRIES = {
    "deftet_nn_index_workspace_bytes": lambda L, ws, w, B, N, M: [
        (L.deftet_nn_index_f32, (P, P, P, B, N, M, ws, w, None)), (L.deftet_nn_index_ragged_f32, (P, P, P, B, N, M, _ints(B, N), ws, w, None))],
    "deftet_tri_dist_workspace_bytes": lambda L, ws, w, B, Pn, F: [
        (L.deftet_tri_dist_fwd_f32, (P, P, P, P, P, B, Pn, F, ws, w, None)), (L.deftet_tri_dist_fwd_order_f32, (P, P, P, P, P, P, B, Pn, F, ws, w, None))],
    "deftet_face_edge_adj_workspace_bytes": lambda L, ws, w, F: [(L.deftet_face_edge_adj_f32, (P, P, F, 10, ws, w, None))],
    "deftet_face_edge_adj_ragged_workspace_bytes": lambda L, ws, w, B, F: [(L.deftet_face_edge_adj_ragged_f32, (P, P, B, F, _ints(B, F), 10, ws, w, None))],
    "deftet_tet_neighbours_workspace_bytes": lambda L, ws, w, T: [(L.deftet_tet_neighbours_i64, (P, P, 2 * T, T, P, P, ws, w, None))],
    "deftet_boundary_index_workspace_bytes": lambda L, ws, w, B, Fi: [(L.deftet_boundary_index_i64, (P, P, P, P, P, B, 384, Fi, 1, ws, w, None))],
    "deftet_tet_energies_workspace_bytes2": lambda L, ws, w, B, T: [(L.deftet_tet_energies_fwd_f32, (P, P, P, P, B, T, 2, 2, 1.0, ws, w, None))],
    "deftet_surface_extract_workspace_bytes": lambda L, ws, w, B, T, ww: [
        (L.deftet_surface_extract_count_f32, (None if ww else P, P if ww else None, P, 300, P, B, T, 1, 0.25, P, ws, w, None)),
        (L.deftet_surface_extract_fill_f32, (P, None, 0, None if ww else P, P, P, B, T, 1, 0.25, 4, P, None, P, P, ws, w, None))],
    "deftet_surface_weld_workspace_bytes": lambda L, ws, w, V: [(L.deftet_surface_weld_f32, (P, 1, P, None, 0, V, 3, P, P, P, None, P, ws, w, None))],
    "deftet_marching_tets_workspace_bytes": lambda L, ws, w, B, T, E: [
        (L.deftet_marching_tets_count_f32, (P, P, P, B, 125, T, E, 0.0, P, P, ws, w, None)),
        (L.deftet_marching_tets_fill_f32, (P, P, None, 0, P, P, P, P, B, 125, T, E, 0.0, 5, 5, P, None, P, P, P, P, ws, w, None))],
    "deftet_mesh_voxelize_workspace_bytes": lambda L, ws, w, B, F: [(L.deftet_mesh_voxelize_f32, (P, P, P, P, B, 200, F, 33, P, P, P, ws, w, None))],
    "deftet_voxel_surface_workspace_bytes": lambda L, ws, w, B, R: [
        (L.deftet_voxel_surface_count_b32, (P, B, R, P, ws, w, None)), (L.deftet_voxel_surface_fill_b32, (P, B, R, 4, 4, P, P, ws, w, None))],
    "deftet_face_edges_workspace_bytes": lambda L, ws, w, F: [(L.deftet_face_edges_i32, (P, F, 250, P, P, ws, w, None))],
    "deftet_sample_points_workspace_bytes": lambda L, ws, w, B, F: [(L.deftet_sample_points_f32, (P, P, P, P, B, F, 64, P, P, P, ws, w, None))],
    "deftet_vertex_adjacency_workspace_bytes": lambda L, ws, w, nnz, V: [
        (L.deftet_vertex_adjacency_csr_i32, (P, P, 8, P, nnz, V, 0, P, P, P, P, P, P, P, ws, w, None))],
    "deftet_tet_vertex_csr_workspace_bytes": lambda L, ws, w, Bi, V, T: [(L.deftet_tet_vertex_csr_i32, (P, P, P, P, Bi, V, T, ws, w, None))],
    "deftet_face_vertex_csr_workspace_bytes": lambda L, ws, w, V, F: [(L.deftet_face_vertex_csr_i32, (P, P, P, P, V, F, ws, w, None))],
    "deftet_edge_vertex_csr_workspace_bytes": lambda L, ws, w, V, E: [(L.deftet_edge_vertex_csr_i32, (P, P, P, P, V, E, ws, w, None))],
    "deftet_tet_order_coherence_workspace_bytes": lambda L, ws, w, T: [(L.deftet_tet_order_coherence_f32, (P, T, P, P, ws, w, None))],
    "deftet_pointvoxel_workspace_bytes": lambda L, ws, w, B, N, R: [
        (L.deftet_avg_voxelize_fwd_f32, (P, P, P, P, P, B, 3, N, R, ws, w, None)),
        (L.deftet_voxel_cells_f32, (P, 0, P, P, P, B, N, R, ws, w, None)),
        (L.deftet_voxel_cells_from_inds_i32, (P, P, P, P, P, P, B, N, R, ws, w, None)),
        (L.deftet_voxel_sample_bwd_vol_f32, (P, P, P, P, None, P, B, 3, R, N, 0, 3, ws, w, None)),
        (L.deftet_voxel_sample_bwd_vol_f32, (P, P, P, P, P, P, B, 3, R, N, 0, 3, ws, w, None))],
    "deftet_image_sample_workspace_bytes": lambda L, ws, w, B, N, H, W: [
        (L.deftet_image_cells_f32, (P, P, P, P, B, N, H, W, 0, 0, ws, w, None)),
        (L.deftet_image_sample_bwd_map_f32, (P, P, P, P, P, B, 3, H, W, N, 0, 3, ws, w, None))],
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


OFF = ctypes.c_void_p(P.value + 16)                                       # 16 bytes off the 256-byte line
# Entries that read a null workspace as "take the brute-force path" (include/deftet_hip.h), so null is no error for them; they
# still refuse a misaligned or short buffer that IS given.  Every entry of this file carves its workspace with an Arena, so none
# is exempt from the 256-byte rule (the plain-array entries that are, rowdot / sqrt_rowsum / radix_sort / scan, have no row here).
NULL_SELECTS = {"deftet_nn_index_f32", "deftet_nn_index_ragged_f32", "deftet_tri_dist_fwd_f32", "deftet_tri_dist_fwd_order_f32",
                "deftet_face_edge_adj_f32", "deftet_face_edge_adj_ragged_f32"}


def _refused(lib, entry, args):
    """the call is refused with the one wording; -> (need, got) as the message states them"""
    assert entry(*args) == EINVAL, lib.deftet_last_error()
    msg = lib.deftet_last_error()
    m = re.search(rb"workspace null, misaligned or too small: need (\d+) bytes, got (\d+) at", msg)
    assert m and b"workspace" in msg and b"misaligned" in msg and b"too small" in msg, msg
    return int(m.group(1)), int(m.group(2))


def _check_entry(lib, calls, need):
    """calls(ws, wsb) -> the (entry, args) list; every entry refuses one byte less than `need`, 16 bytes off, and null"""
    for k, (entry, _) in enumerate(calls(P, need)):
        assert _refused(lib, *calls(P, need - 1)[k]) == (need, need - 1), entry.__name__
        assert _refused(lib, *calls(OFF, need)[k]) == (need, need), entry.__name__          # enough bytes: refused for the alignment
        if entry.__name__ not in NULL_SELECTS:
            assert _refused(lib, *calls(None, need)[k]) == (need, need), entry.__name__     # enough bytes: refused for the null


@pytest.mark.parametrize("fr", [fr for fr in SMALL if fr[0] != "deftet_builder_workspace_bytes"], ids=_id)
def test_entry_refuses_one_byte_less(lib, fr):
    name, row = fr
    need = getattr(lib, name)(*row["args"])
    _check_entry(lib, lambda ws, w: ENTRIES[name](lib, ws, w, *row["args"]), need)


# What each builder's layout must hold besides the temporaries of its sort and scans (builders.hip, "one layout per builder"):
# a stated size at or below this is another builder's.  Per element: 8 a u64 key, 4 an owner / flag / position, 8 a 64-bit count.
ARRAY_BYTES = {
    "deftet_tet_adj_share_i32": lambda n_point, T: 4 * T * (2 * 8 + 4 * 4),               # 4T (key, owner) pairs twice, flag, position
    "deftet_tet_face_adj_i32": lambda n_point, T: 12 * T * (2 * 8 + 2 * 4 + 2 * 8) + 4 * T * 8,
    "deftet_tet_point_adj_i32": lambda n_point, T: 12 * T * (2 * 8 + 2 * 4),
    "deftet_colaps_v_f32": lambda n_point, T: n_point * (5 * 8 + 7 * 4),
    "deftet_tet_to_face_i32": lambda n_point, T: 4 * T * (2 * 8 + 10 * 4),
    "deftet_tet_edges_i64": lambda n_point, T: 6 * T * (2 * 8 + 4 * 4),
    "deftet_subdivide_f32": lambda n_point, T: T * 4 * 4,
    "deftet_delete_tet_i64": lambda n_point, T: T * 2 * 4,
}


@pytest.mark.parametrize("fr", [fr for fr in SMALL if fr[0] == "deftet_builder_workspace_bytes"], ids=_id)
def test_builders_refuse_less_than_their_layout(lib, fr):
    n_point, T = fr[1]["args"]
    largest = lib.deftet_builder_workspace_bytes(n_point, T)
    needs = []
    for k, (entry, args) in enumerate(_builders(lib, n_point, T, P, 0)):
        need, got = _refused(lib, entry, args)                             # the builder's own size, as it states it
        assert got == 0 and ARRAY_BYTES[entry.__name__](n_point, T) < need <= largest and need % 256 == 0, (entry.__name__, need)
        _check_entry(lib, lambda ws, w: _builders(lib, n_point, T, ws, w)[k:k + 1], need)
        needs.append(need)
    assert needs[1] == max(needs) == largest                               # the face adjacency sets the shared size, not more
