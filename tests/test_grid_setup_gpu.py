"""csrc/grid_setup.hpp — the box / sum reduction and the cell function that the binned operators share.  Every operator's grid
path against its own exhaustive path, with exact equality, at the element counts where the reduction itself can go wrong:

    one           1 element: one lane of one block is live, every other partial record is the +-inf identity
    two_blocks    257: two blocks, a ragged last wave
    second_trip   64 * 256 + 77: every block takes a second strided trip, the last one partial
    empty_second  a batch whose second shape has no valid element: the hi < lo branch of the grid kernels
    flat_x        every element on the plane x = 0.25: a flat axis (inv = 0) where x is a grid axis and the elements stay regular
    flat_z        the same on z = 0.25 (faces in a plane x = const are edge-on for the tri-distance grid and leave it empty)

For check_sign an element is one tetrahedron of a soup, i.e. four faces: a closed mesh has an even number of faces.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {"one": 1, "two_blocks": 257, "second_trip": 64 * 256 + 77, "empty_second": 257, "flat_x": 257, "flat_z": 257}
N_QUERY = 1000


def _batch(case):
    return 2 if case == "empty_second" else 1


def _flatten(case, xyz):
    if case.startswith("flat"):
        xyz[..., "xyz".index(case[-1])] = 0.25
    return xyz


@pytest.fixture(scope="module")
def queries():
    rng = np.random.default_rng(7)
    q = (rng.random((2, N_QUERY, 3)) * 1.2 - 0.1).astype(np.float32)          # the elements live in [0, 1]^3
    q[:, :4] = np.float32([[3.0, 0.5, 0.5], [-2.0, -2.0, -2.0], [0.5, 0.5, 7.0], [0.25, 1.5, 0.25]])   # well outside their box
    assert np.isfinite(q).all()
    return q


def _triangles(case, seed):
    """[B, F, 3, 3] small random triangles (no shared vertices: no exact ties between faces) and their counts"""
    rng = np.random.default_rng(seed)
    B, F = _batch(case), CASES[case]
    face = (rng.random((B, F, 1, 3)) * 0.9 + 0.05 + (rng.random((B, F, 3, 3)) - 0.5) * 0.08).astype(np.float32)
    face = _flatten(case, face)
    n = np.full(B, F, np.int32)
    if case == "empty_second":
        n[1] = 0
    assert np.isfinite(face).all() and (0 <= n).all() and (n <= F).all() and face.min() >= 0.0 and face.max() <= 1.0
    return face, n


def _tet_soup(case, seed):
    """verts [B, 4 N, 3], faces [4 N, 3]: N seeded tetrahedra, each a closed, consistently wound surface of its own"""
    rng = np.random.default_rng(seed)
    B, N = _batch(case), CASES[case]
    verts = (rng.random((B, N, 1, 3)) * 0.8 + 0.1 + (rng.random((B, N, 4, 3)) - 0.5) * 0.1).astype(np.float32)
    verts = _flatten(case, verts).reshape(B, 4 * N, 3)
    faces = (np.arange(N)[:, None, None] * 4 + np.int64([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])[None]).reshape(-1, 3)
    # closed and consistently wound: every directed edge occurs once, and so does its reverse
    a, b = faces[:, [0, 1, 2]].ravel(), faces[:, [1, 2, 0]].ravel()
    fwd, rev = a * (4 * N) + b, b * (4 * N) + a
    assert np.unique(fwd).size == fwd.size and np.array_equal(np.sort(fwd), np.sort(rev))
    assert np.isfinite(verts).all() and faces.min() == 0 and faces.max() == 4 * N - 1
    if case == "empty_second":
        verts[1] = np.nan                                                     # the face list is shared: no face of shape 1 is regular
    return verts, faces


@pytest.mark.parametrize("case", list(CASES))
def test_nn_index(cuda, queries, case):
    from deftet_amd import hip_ops
    rng = np.random.default_rng(11)
    B = _batch(case)
    pts = _flatten(case, rng.random((B, CASES[case], 3)).astype(np.float32))
    assert np.isfinite(pts).all()
    if case == "empty_second":
        pts[1] = np.nan                                                       # never nearest: both paths answer index 0
    q, p = torch.from_numpy(queries[:B]).to(cuda), torch.from_numpy(pts).to(cuda)
    got, want = hip_ops.nn_index(q, p), hip_ops.nn_index(q, p, brute=True)
    assert torch.equal(got, want)
    if case == "empty_second":
        assert (want[1] == 0).all() and want[0].max() > 0


@pytest.mark.parametrize("case", list(CASES))
def test_tri_dist_fwd(cuda, queries, case):
    from deftet_amd import hip_ops
    face, n = _triangles(case, 13)
    B = _batch(case)
    q, f, nfb = torch.from_numpy(queries[:B]).to(cuda), torch.from_numpy(face).to(cuda), torch.from_numpy(n.astype(np.float32)).to(cuda)
    d, i, order = hip_ops.tri_dist_fwd(q, f, nfb, want_order=True)
    wd, wi = hip_ops.tri_dist_fwd(q, f, nfb, brute=True)
    assert torch.equal(i, wi) and torch.equal(d, wd)
    assert torch.equal(order.long().sort(1).values, torch.arange(N_QUERY, device=cuda).expand(B, -1))   # a permutation per shape
    if case == "empty_second":
        assert (wi[1] == -1).all() and (wi[0] >= 0).all()


@pytest.mark.parametrize("case", list(CASES))
def test_point_mesh_distance(cuda, queries, case):
    from deftet_amd import metrics
    face, n = _triangles(case, 17)
    B = _batch(case)
    q, f, nf = torch.from_numpy(queries[:B]).to(cuda), torch.from_numpy(face).to(cuda), torch.from_numpy(n).to(cuda)
    got = metrics.point_to_mesh_distance(q, f, nf)
    want = metrics.point_to_mesh_distance(q, f, nf, brute=True)
    for g, w in zip(got, want):                                               # squared distance, face, feature type
        assert torch.equal(g, w)
    assert (want[1][0] >= 0).all()


@pytest.mark.parametrize("case", list(CASES))
def test_check_sign(cuda, queries, case):
    from deftet_amd import hip_ops
    verts, faces = _tet_soup(case, 19)
    B = _batch(case)
    q, v, f = torch.from_numpy(queries[:B]).to(cuda), torch.from_numpy(verts).to(cuda), torch.from_numpy(faces).to(cuda)
    got, cg = hip_ops.check_sign(v, f, q, return_count=True)
    want, cw = hip_ops.check_sign(v, f, q, brute=True, return_count=True)
    assert torch.equal(cg, cw) and torch.equal(got, want)                     # crossing counts, not only their parity
    if case == "empty_second":
        assert (cw[1] == 0).all()
    if case == "second_trip":
        assert cw[0].max() >= 2
