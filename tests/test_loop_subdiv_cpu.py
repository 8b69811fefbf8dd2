"""Loop subdivision without a GPU: the float64 restatement (tests/loop_subdiv_ref.py) on the meshes of
tests/loop_subdiv_cases.py has the properties of the scheme — rows that sum to one, affine invariance, closed stays closed with
its Euler characteristic, the regular stencils, the limit weights as the left eigenvector of the one-ring matrix — and a
sequential float32 evaluation stays inside the bound the GPU test asserts; the header, the ctypes table and the library agree
on the five entry points, which refuse bad arguments with their status codes before any device work; the new keywords default
to off."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import loop_subdiv_cases as K
from tests import loop_subdiv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("deftet_loop_topology_workspace_bytes", "deftet_loop_topology_count_i64", "deftet_loop_topology_fill_i64",
           "deftet_loop_subdivide_fwd_f32", "deftet_loop_subdivide_bwd_f32")
NAMES = tuple(K.CASES)


# ---------------------------------------------------------------------------- the scheme
@pytest.mark.parametrize("name", NAMES)
def test_rows_sum_to_one(name):
    _top, S, L = K.reference(name)
    for M in (S, L):
        assert np.abs(np.asarray(M.sum(1)).reshape(-1) - 1.0).max() <= 2.0 ** -50
        assert M.data.min() > 0                                          # a convex combination (1 - n beta = 5/8 or 7/16)


@pytest.mark.parametrize("name", NAMES)
def test_an_affine_map_commutes(name):
    v, _f = K.case(name)
    _top, S, L = K.reference(name)
    rng = np.random.default_rng(0)
    A, t = rng.normal(size=(3, 3)), rng.normal(size=3)
    x = v.astype(np.float64)
    for M in (S, L):
        lhs, rhs = M @ (x @ A.T + t), (M @ x) @ A.T + t
        assert np.abs(lhs - rhs).max() <= 1e-12 * max(1.0, np.abs(rhs).max())


@pytest.mark.parametrize("name", K.CLOSED)
def test_closed_stays_closed_over_three_levels(name):
    v, f = K.case(name)
    used = np.unique(f).shape[0]
    chi = used - ref.edge_face_counts(f).shape[0] + f.shape[0]
    assert (ref.edge_face_counts(f) == 2).all()
    verts, faces = v.astype(np.float64), f
    for level in range(3 if f.shape[0] < 500 else 2):                  # (the sphere's third level has 63 K faces: two are enough there)
        top = ref.topology(faces, verts.shape[0])
        assert (top.vertex_kind == 0).all() and (top.edge_opp >= 0).all()
        verts, faces = ref.subdivision_matrix(top) @ verts, top.child_faces
        assert faces.shape[0] == 4 ** (level + 1) * f.shape[0]
        assert (ref.edge_face_counts(faces) == 2).all()
        assert np.unique(faces).shape[0] - ref.edge_face_counts(faces).shape[0] + faces.shape[0] == chi
    assert chi == (4 if name == "two_copies" else 2)


def test_winding_is_kept():
    v, f = K.case("icosahedron")
    w, g, _S = ref.subdivide(v, f, 1)
    vol = lambda x, t: np.einsum("ij,ij->i", x[t[:, 0]], np.cross(x[t[:, 1]], x[t[:, 2]])).sum() / 6
    assert vol(v.astype(np.float64), f) > 0 and vol(w, g) > 0
    n0 = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n1 = np.cross(w[g[:, 1]] - w[g[:, 0]], w[g[:, 2]] - w[g[:, 0]])
    assert (np.einsum("ij,ij->i", np.repeat(n0, 4, axis=0), n1) > 0).all()            # children 4f..4f+3 face the way f did


def test_flat_regular_patch():
    v, _f = K.case("flat_patch")
    top, S, L = K.reference("flat_patch")
    inner = K.patch_interior()
    assert inner.sum() == 9 and (top.vertex_kind[inner] == 0).all() and (top.vertex_kind[~inner] == 1).all()
    n = np.diff(top.ev_offsets)
    assert (n[inner] == 6).all() and sorted(n[~inner])[:2] == [2, 2]
    x = v.astype(np.float64)
    assert np.abs((S @ x)[:25][inner] - x[inner]).max() <= 1e-15 and np.abs((L @ x)[inner] - x[inner]).max() <= 1e-15
    assert np.abs((S @ x)[:, 2]).max() == 0                              # the plane stays the plane
    for r in np.nonzero(inner)[0]:
        row = S.getrow(r)
        assert row.nnz == 7 and row[0, r] == 10.0 / 16.0 and sorted(row.data)[:6] == [1.0 / 16.0] * 6
        lim = L.getrow(r)
        assert lim.nnz == 7 and abs(lim[0, r] - 0.5) < 1e-16 and np.abs(np.sort(lim.data)[:6] - 1.0 / 12.0).max() < 1e-16


def test_limit_weights_are_the_left_eigenvector():
    """the limit position of a smooth vertex is l . (v, ring) with l the left eigenvector of the one-ring matrix to the eigenvalue
    1, normalised to sum 1: l = (1 - n gamma, gamma, ..., gamma)"""
    assert abs(ref.gamma(6) - 1.0 / 12.0) < 1e-16 and abs(ref.gamma(3) - 0.2) < 1e-16
    for n in range(3, 9):
        M = ref.one_ring_matrix(n)
        assert np.abs(M.sum(1) - 1).max() < 1e-15
        vals, vecs = np.linalg.eig(M.T)
        k = int(np.argmin(np.abs(vals - 1.0)))
        assert abs(vals[k] - 1.0) < 1e-12 and np.sort(np.abs(vals))[-2] < 1.0 - 1e-3      # 1 is simple and dominant
        left = np.real(vecs[:, k])
        left = left / left.sum()
        g = ref.gamma(n)
        assert np.abs(left - np.array([1 - n * g] + [g] * n)).max() < 1e-12, n


def test_kinds_of_the_singular_cases():
    book, bow = K.reference("book")[0], K.reference("bowtie")[0]
    assert book.vertex_kind.tolist() == [2, 2, 1, 1, 1] and book.edge_nface[0] == 3 and book.edge_opp[0].tolist() == [-1, -1]
    assert book.crease_nbr.tolist() == [[-1, -1], [-1, -1], [0, 1], [0, 1], [0, 1]]
    assert bow.vertex_kind.tolist() == [2, 1, 1, 1, 1] and (bow.edge_nface == 1).all()
    big = K.reference("big_index")[0]
    assert int(big.edges[0, 0]) * big.n_vertex + int(big.edges[0, 1]) > 2 ** 32
    assert (np.diff(big.ev_offsets) == 0).sum() == big.n_vertex - 6 and (big.vertex_kind == 0).all()
    S = K.reference("big_index")[1]
    assert S.getrow(5).nnz == 1 and S[5, 5] == 1.0                       # an isolated vertex: itself
    two = K.reference("two_copies")[0]
    assert (two.edges[:30] < 12).all() and (two.edges[30:] >= 12).all()  # shapes on ascending ranges own ascending edge ranges
    hub = K.reference("smooth_fan200")[0]
    assert hub.vertex_kind[0] == 0 and np.diff(hub.ev_offsets)[0] == 200
    assert K.reference("open_fan200")[0].vertex_kind[0] == 1 and K.reference("closed_fan70")[0].vertex_kind[0] == 0


def _sequential_f32(M, x):
    """every row's sum in float32, one term after the other in the matrix's column order, weights rounded to float32"""
    M = M.tocsr()
    out = np.zeros((M.shape[0], x.shape[1]), np.float32)
    for r in range(M.shape[0]):
        acc = np.zeros(x.shape[1], np.float32)
        for k in range(M.indptr[r], M.indptr[r + 1]):
            acc = (acc + np.float32(M.data[k]) * x[M.indices[k]]).astype(np.float32)
        out[r] = acc
    return out


@pytest.mark.parametrize("name", ("smooth_fan200", "open_fan200", "sphere20", "book"))
def test_sequential_float32_stays_inside_the_gpu_bound(name):
    v, _f = K.case(name)
    _top, S, L = K.reference(name)
    g = np.random.default_rng(1).normal(size=(S.shape[0], 3)).astype(np.float32)
    fwd = np.abs(_sequential_f32(S, v) - S @ v.astype(np.float64)) / np.maximum(ref.forward_bound(S, v), 1e-300)
    bwd = np.abs(_sequential_f32(S.T, g) - S.T @ g.astype(np.float64)) / np.maximum(ref.backward_bound(S, g), 1e-300)
    lim = np.abs(_sequential_f32(L, v) - L @ v.astype(np.float64)) / np.maximum(ref.forward_bound(L, v), 1e-300)
    print("%s: forward %.3f, backward %.3f, limit %.3f of the bound" % (name, fwd.max(), bwd.max(), lim.max()))
    assert fwd.max() < 0.6 and bwd.max() < 0.6 and lim.max() < 0.6     # room for another order of the same terms


# ---------------------------------------------------------------------------- the C ABI
def test_header_ctypes_table_and_library_agree():
    from deftet_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    note = re.search(r"^/\* 410:(.*?)\*/", txt, flags=re.S | re.M)
    assert note, "no 410: version note"
    for s in SYMBOLS:
        assert re.sub(r"_(fwd|bwd)_f32$", "", s) in note.group(1), s
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % s, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[s][1]), s                  # as many parameters as the table lists
    assert _lib.load().deftet_version() >= 410


def test_entry_points_refuse_bad_arguments():
    from deftet_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    buf = ctypes.create_string_buffer(1 << 20)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed
    err = lib.deftet_last_error
    need = lib.deftet_loop_topology_workspace_bytes(6, 8)
    assert need > 0 and need % 256 == 0 and lib.deftet_loop_topology_workspace_bytes(0, 8) == 256
    assert lib.deftet_loop_topology_workspace_bytes(6, 0) == 256 and lib.deftet_loop_topology_workspace_bytes(6, 2 ** 29) == 256
    count, fill, fwd, bwd = (lib.deftet_loop_topology_count_i64, lib.deftet_loop_topology_fill_i64, lib.deftet_loop_subdivide_fwd_f32,
                             lib.deftet_loop_subdivide_bwd_f32)
    assert count(P, 0, 6, None, 0, P, P, need, None) == EINVAL and b"must be positive" in err()
    assert count(P, 8, 0, None, 0, P, P, need, None) == EINVAL and b"must be positive" in err()
    assert count(P, 2 ** 29, 6, None, 0, P, P, need, None) == EINVAL and b"31 bits" in err()
    assert count(None, 8, 6, None, 0, P, P, need, None) == EINVAL and b"null pointer" in err()
    assert count(P, 8, 6, None, 0, None, P, need, None) == EINVAL and b"null pointer" in err()
    assert count(P, 8, 6, None, 2, P, P, need, None) == EINVAL and b"do not go together" in err()
    for ws, n in ((None, need), (P, need - 1), (ctypes.c_void_p(P.value + 16), need)):
        assert count(P, 8, 6, None, 0, P, ws, n, None) == EINVAL
        assert b"workspace null, misaligned or too small: need %d bytes" % need in err()
    tables = [P] * 11
    assert fill(P, 8, 6, 0, *tables, P, need, None) == EINVAL and b"n_edge" in err()
    assert fill(P, 8, 6, 25, *tables, P, need, None) == EINVAL and b"n_edge" in err()
    assert fill(P, 8, 6, 12, *(tables[:4] + [None] + tables[5:]), P, need, None) == EINVAL and b"null pointer" in err()
    assert fill(P, 8, 6, 12, *tables, P, need - 1, None) == EINVAL and b"workspace" in err()
    top = [P] * 7
    assert fwd(P, None, 0, *top, 1, 6, 12, 2, P, None, None) == EINVAL and b"mode" in err()
    assert fwd(P, None, 0, *top, 0, 6, 12, 0, P, None, None) == EINVAL and b"must be positive" in err()
    assert fwd(P, P, 9, *top, 1, 6, 12, 0, P, P, None) == EINVAL and b"n_attr" in err()
    assert fwd(P, None, 3, *top, 1, 6, 12, 0, P, P, None) == EINVAL and b"do not go together" in err()
    assert fwd(P, P, 3, *top, 1, 6, 12, 0, P, None, None) == EINVAL and b"do not go together" in err()
    assert fwd(None, None, 0, *top, 1, 6, 12, 0, P, None, None) == EINVAL and b"null pointer" in err()
    assert fwd(P, None, 0, *([None] + top[1:]), 1, 6, 12, 0, P, None, None) == EINVAL and b"topology table" in err()
    assert fwd(P, None, 0, *([ctypes.c_void_p(P.value + 4)] + top[1:]), 1, 6, 12, 0, P, None, None) == EINVAL and b"8-byte aligned" in err()
    assert fwd(P, None, 0, *top, 1, 2 ** 30, 2 ** 30, 0, P, None, None) == EINVAL and b"31 bits" in err()
    more = [P] * 3
    assert bwd(P, None, 0, *top, *more, 1, 6, 12, 8, 3, P, None, None) == EINVAL and b"mode" in err()
    assert bwd(P, None, 0, *top, *more, 1, 6, 12, 0, 0, P, None, None) == EINVAL and b"n_face" in err()
    assert bwd(None, None, 0, *top, *more, 1, 6, 12, 8, 0, None, None, None) == EINVAL and b"every output" in err()
    assert bwd(P, None, 0, *top, *more, 1, 6, 12, 8, 0, None, None, None) == EINVAL and b"goes with" in err()
    assert bwd(None, P, 0, *top, *more, 1, 6, 12, 8, 0, None, P, None) == EINVAL and b"without attributes" in err()
    assert bwd(P, None, 0, *top, *[None, P, P], 1, 6, 12, 8, 0, P, None, None) == EINVAL and b"topology table" in err()


# ---------------------------------------------------------------------------- the front ends
def test_new_keywords_default_to_off():
    from deftet_amd import hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    from deftet_amd.render import export, iso_surface
    for fn in (iso_surface.marching_tets, iso_surface.marching_tets_normals, DefTet.iso_surface, export.save_surface_objs):
        assert inspect.signature(fn).parameters["subdivide"].default == 0, fn
    sig = inspect.signature(hip_ops.loop_subdivide_mesh).parameters
    assert sig["levels"].default == 1 and sig["limit"].default is False and sig["attr"].default is None
    sig = inspect.signature(hip_ops.loop_subdivide_list).parameters
    assert sig["levels"].default == 1 and sig["limit"].default is False and sig["attr_list"].default is None
    assert list(inspect.signature(hip_ops.LoopTopology.__init__).parameters)[1:4] == ["faces_fx3", "n_vertex", "device"]
    assert (hip_ops.LOOP_SUBDIVIDE, hip_ops.LOOP_LIMIT) == (0, 1)


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from deftet_amd import _lib, hip_ops
    from deftet_amd.render import iso_surface
    v, f = K.case("octahedron")
    with pytest.raises(_lib.DefTetHipError):
        hip_ops.LoopTopology(torch.from_numpy(f.copy()), 6)
    with pytest.raises(RuntimeError):
        hip_ops.LoopTopology(torch.zeros(4, 4, dtype=torch.int64), 6)
    with pytest.raises(TypeError):
        hip_ops.loop_subdivide(torch.zeros(6, 3), object())
    with pytest.raises(TypeError):
        hip_ops.loop_limit(torch.zeros(6, 3), None)
    with pytest.raises(ValueError):
        hip_ops.loop_subdivide_mesh(torch.zeros(6, 3), torch.from_numpy(f.copy()), levels=-1)
    with pytest.raises(ValueError):
        iso_surface.marching_tets(None, 0.5, None, return_index=True, subdivide=1)
    with pytest.raises(ValueError):
        iso_surface.marching_tets_normals(None, 0.5, None, subdivide=-1)
    # a list without faces, or zero levels: handed back untouched, nothing of the library runs
    vs, fs = [torch.zeros(0, 3)], [torch.zeros(0, 3, dtype=torch.int64)]
    out = hip_ops.loop_subdivide_list(vs, fs)
    assert out[0][0] is vs[0] and out[2] is None
    vs, fs = [torch.from_numpy(v.copy())], [torch.from_numpy(f.copy())]
    out = hip_ops.loop_subdivide_list(vs, fs, levels=0)
    assert out[0][0] is vs[0] and torch.equal(out[1][0], fs[0])
