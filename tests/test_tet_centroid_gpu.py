"""GPU tests of tet-centroid feature sampling (tet_centroid_sample.hip): bit for bit against the operators it
replaces (hip_ops.voxel_sample on the same centroids) and against the fp32 restatements of tests/tet_centroid_ref.py, within the
standing 1e-5 max-norm bound of the fp64 restatement, the reduction's edge cases, the empty and partial forms, determinism, the
bad-index rule, the module routes and the argument errors."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_occ_callers as callers
from tests import tet_centroid_ref as ref
from tests.tol import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5
V, T = 300, 1500
VOLUMES = ((5, 32), (3, 16), (4, 16), (130, 8))    # mixed resolutions, two volumes on one sort, 130: no multiple of a channel chunk
C_FEAT = sum(c for c, _ in VOLUMES)


def bits(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def rng(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def volumes(B):
    return tuple(torch.randn(B, c, r, r, r, generator=rng(10 * B + k)) for k, (c, r) in enumerate(VOLUMES))


@functools.lru_cache(maxsize=None)
def mesh(seed=1, n_vertex=V, n_tet=T):
    return torch.from_numpy(ref.random_tets(n_tet, n_vertex, seed))


def gpu_volumes(B, grad=True):
    return [v.to(DEV).requires_grad_(grad) for v in volumes(B)]


def csr_of(tets, n_vertex=V):
    from deftet_amd import hip_ops
    return hip_ops.tet_vertex_csr(tets.to(DEV), n_vertex)


def run(B, pos, tets, sel, csr=None, vols=None, gout_seed=11, n_vertex=V):
    """forward + backward of the operator: (out, centroids, gout, volume grads, gcent, pos.grad)"""
    from deftet_amd import hip_ops
    vols = gpu_volumes(B) if vols is None else vols
    p = pos.to(DEV).requires_grad_(True)
    t = tets.to(DEV)
    sel = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in sel.items()}
    out, cent = hip_ops.tet_centroid_sample(vols, p, t, csr=csr_of(tets, n_vertex) if csr is None else csr, return_centroids=True, **sel)
    gout = torch.randn(out.shape, generator=rng(gout_seed)).to(DEV)
    out.backward(gout)
    gcent = hip_ops.tet_centroid_sample_bwd_pos([v.detach() for v in vols], cent, gout, append_pos=True)
    return out.detach(), cent, gout, [v.grad for v in vols], gcent, p.grad


SELECTIONS = [("K%d" % k, k) for k in (1, 63, 64, 65, 257)] + [("all", None), ("range", (37, 200))]


def selection(what):
    if what is None:
        return {}
    if isinstance(what, tuple):
        return {"first": what[0], "count": what[1]}
    return {"select": torch.randperm(T, generator=rng(what))[:what]}             # an unsorted prefix of a permutation


# ---------------------------------------------------------------------------- 1. bit-exact against the existing operators
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,what", SELECTIONS, ids=[s[0] for s in SELECTIONS])
def test_bit_identical_to_the_operators_it_replaces(B, name, what):
    from deftet_amd import hip_ops
    pos, tets, sel = ref.uniform_vertices(B, V, 5 + B), mesh(), selection(what)
    out, cent, gout, gvols, gcent, gpos = run(B, pos, tets, sel)
    K = cent.shape[1]
    assert out.shape == (B, C_FEAT + 3, K) and out.is_contiguous() and cent.shape == (B, K, 3)
    assert same_bits(cent, ref.centroids(pos, tets, **sel))
    # the existing chain on the same centroids: values, volume gradients and the gradient on the centroids
    v2, c2 = gpu_volumes(B), cent.clone().requires_grad_(True)
    out2 = hip_ops.voxel_sample(v2, c2, append_pos=True)
    assert same_bits(out, out2)
    out2.backward(gout)
    for k, (a, b) in enumerate(zip(gvols, v2)):
        assert same_bits(a, b.grad), "volume %d" % k
    assert same_bits(gcent, c2.grad)
    # and the reduction onto the vertices against its restatement
    assert same_bits(gpos, ref.vertex_reduction(gcent, tets, V, select=sel.get("select"), first=sel.get("first", 0)))


# ---------------------------------------------------------------------------- 2. against fp64
def fp64_run(B, pos, tets, sel, gout):
    vols = [v.double().requires_grad_(True) for v in volumes(B)]
    p = pos.double().requires_grad_(True)
    want = ref.occ_feature(vols, p, tets, **sel)
    want.backward(gout.cpu().double())
    return want.detach(), [v.grad for v in vols], p.grad


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("what", [257, (37, 200)], ids=["K257", "range"])
def test_values_and_volume_gradients_match_the_fp64_restatement(B, what):
    pos, tets, sel = ref.uniform_vertices(B, V, 20 + B), mesh(), selection(what)
    out, cent, gout, gvols, gcent, gpos = run(B, pos, tets, sel)
    want, want_gvols, _ = fp64_run(B, pos, tets, sel, gout)
    check_close("tcs.B%d.values" % B, out, want, BOUND)
    for k, (a, b) in enumerate(zip(gvols, want_gvols)):
        check_close("tcs.B%d.grad_vol%d" % (B, k), a, b, BOUND)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("what", [257, None], ids=["K257", "all"])
def test_position_gradient_matches_the_fp64_restatement_on_lattice_inputs(B, what):
    """the gradient jumps at integer voxel coordinates: checked where every chosen centroid keeps 0.01 from them (asserted)"""
    pos, tets, sel = ref.lattice_vertices(B, V, 30 + B), mesh(), selection(what)
    cent64 = ref.centroids64(pos, tets, **sel)
    for R in (32, 16, 8):
        margin, inside = ref.lattice_margin(cent64, R)
        assert inside and margin >= 0.01, (R, margin)
    out, cent, gout, gvols, gcent, gpos = run(B, pos, tets, sel)
    want, want_gvols, want_gpos = fp64_run(B, pos, tets, sel, gout)
    check_close("tcs.lattice.B%d.values" % B, out, want, BOUND)
    check_close("tcs.lattice.B%d.grad_pos" % B, gpos, want_gpos, BOUND)
    for k, (a, b) in enumerate(zip(gvols, want_gvols)):
        check_close("tcs.lattice.B%d.grad_vol%d" % (B, k), a, b, BOUND)


# ---------------------------------------------------------------------------- 3. the reduction's edge cases
def test_every_chosen_tet_three_times_shuffled():
    B, tets = 3, mesh()
    once = torch.randperm(T, generator=rng(1))[:200]
    sel = {"select": torch.cat([once, once, once])[torch.randperm(600, generator=rng(2))]}
    out, cent, gout, gvols, gcent, gpos = run(B, ref.uniform_vertices(B, V, 3), tets, sel)
    assert same_bits(cent, ref.centroids(ref.uniform_vertices(B, V, 3), tets, **sel))
    assert same_bits(gpos, ref.vertex_reduction(gcent, tets, V, select=sel["select"]))


def test_fan_mesh_six_hundred_slots_on_one_vertex():
    B, n_vertex, n_tet = 2, 70, 300
    tets = torch.from_numpy(ref.fan_tets(n_tet, n_vertex, 4))
    sel = {"select": torch.cat([torch.arange(n_tet), torch.arange(n_tet)])[torch.randperm(2 * n_tet, generator=rng(5))]}
    out, cent, gout, gvols, gcent, gpos = run(B, ref.uniform_vertices(B, n_vertex, 6), tets, sel, n_vertex=n_vertex)
    want = ref.vertex_reduction(gcent, tets, n_vertex, select=sel["select"])
    assert same_bits(gpos, want) and np.all(want[:, 0] != 0)


def test_per_shape_tet_lists():
    B = 3
    tets = torch.from_numpy(ref.random_tets(T, V, 7, B=B))
    pos, sel = ref.uniform_vertices(B, V, 8), selection(257)
    out, cent, gout, gvols, gcent, gpos = run(B, pos, tets, sel)
    assert same_bits(cent, ref.centroids(pos, tets, **sel))
    assert same_bits(gpos, ref.vertex_reduction(gcent, tets, V, select=sel["select"]))
    assert not same_bits(cent[0], ref.centroids(pos, tets[1], **sel)[0])         # the shapes do read their own lists


def test_vertices_without_a_chosen_tet_get_exact_zeros_and_accumulate_adds():
    from deftet_amd import hip_ops
    B, used = 3, 250
    tets = torch.from_numpy(ref.random_tets(T, used, 9))               # vertices 250 .. 299 are in no tet
    sel = selection(64)
    pos = ref.uniform_vertices(B, V, 10)
    out, cent, gout, gvols, gcent, gpos = run(B, pos, tets, sel)
    want = ref.vertex_reduction(gcent, tets, V, select=sel["select"])
    assert same_bits(gpos, want)
    csr, select32 = csr_of(tets), sel["select"].to(DEV).int()
    junk = torch.full((B, V, 3), float("nan"), device=DEV)            # freed: the next tensor of this size takes its place, and a
    del junk                                                           # store the kernel left out would show as a NaN
    gpos = hip_ops.tet_centroid_sample_bwd_vertices(gcent, csr, V, T, select=select32)
    assert same_bits(gpos, want)
    chosen = np.unique(tets[sel["select"]].numpy())
    idle = np.setdiff1d(np.arange(V), chosen)
    assert len(idle) >= 50 and np.all(bits(gpos)[:, idle] == 0) and np.all(bits(gpos)[:, chosen].any(axis=2))
    base = torch.randn(B, V, 3, generator=rng(12))
    acc = base.to(DEV)
    got = hip_ops.tet_centroid_sample_bwd_vertices(gcent, csr_of(tets), V, T, select=sel["select"].to(DEV).int(), out=acc)
    assert got is acc and same_bits(acc, ref.vertex_reduction(gcent, tets, V, select=sel["select"], base=base))
    acc = base.to(DEV)                                                 # and the range form, which needs no workspace
    hip_ops.tet_centroid_sample_bwd_vertices(gcent, csr_of(tets), V, T, first=100, out=acc)
    assert same_bits(acc, ref.vertex_reduction(gcent, tets, V, first=100, base=base))


# ---------------------------------------------------------------------------- 4. empty and partial
@pytest.mark.parametrize("sel", [{"select": torch.zeros(0, dtype=torch.long)}, {"first": 40, "count": 0}], ids=["select", "range"])
def test_no_slot(sel):
    B = 2
    out, cent, gout, gvols, gcent, gpos = run(B, ref.uniform_vertices(B, V, 1), mesh(), sel)
    assert out.shape == (B, C_FEAT + 3, 0) and cent.shape == (B, 0, 3) and gcent.shape == (B, 0, 3)
    assert gpos.shape == (B, V, 3) and not bits(gpos).any()
    for g, v in zip(gvols, volumes(B)):
        assert g.shape == v.shape and not bits(g).any()


def test_no_volume_returns_the_position_rows():
    from deftet_amd import hip_ops
    B, tets, sel = 2, mesh(), selection(65)
    pos = ref.uniform_vertices(B, V, 2).to(DEV).requires_grad_(True)
    out, cent = hip_ops.tet_centroid_sample([], pos, tets.to(DEV), csr=csr_of(tets), select=sel["select"].to(DEV), return_centroids=True)
    assert out.shape == (B, 3, 65) and torch.equal(out.detach(), cent.permute(0, 2, 1))
    gout = torch.randn(B, 3, 65, generator=rng(3)).to(DEV)
    out.backward(gout)
    assert same_bits(pos.grad, ref.vertex_reduction((0.0 + gout).permute(0, 2, 1), tets, V, select=sel["select"]))
    bare = hip_ops.tet_centroid_sample(list(gpu_volumes(B, grad=False)), pos.detach(), tets.to(DEV), select=sel["select"].to(DEV), append_pos=False)
    assert bare.shape == (B, C_FEAT, 65)


def test_no_csr_is_asked_for_when_pos_needs_no_gradient(monkeypatch):
    from deftet_amd import hip_ops
    B, tets, sel = 2, mesh(), selection(257)
    pos = ref.uniform_vertices(B, V, 4)
    want = run(B, pos, tets, sel)
    calls = []
    real = hip_ops.tet_vertex_csr
    monkeypatch.setattr(hip_ops, "tet_vertex_csr", lambda *a, **k: calls.append(1) or real(*a, **k))
    vols, p = gpu_volumes(B), pos.to(DEV)
    out = hip_ops.tet_centroid_sample(vols, p, tets.to(DEV), select=sel["select"].to(DEV))
    out.backward(want[2])
    assert not calls and p.grad is None and same_bits(out, want[0])
    for a, b in zip(vols, want[3]):
        assert same_bits(a.grad, b)
    p.requires_grad_(True)                                             # without a CSR the backward builds one: the slow path, the same bits
    hip_ops.tet_centroid_sample(gpu_volumes(B), p, tets.to(DEV), select=sel["select"].to(DEV)).backward(want[2])
    assert calls == [1] and same_bits(p.grad, want[5])


def test_ranges_of_500_concatenate_to_one_call_over_all_tets():
    from deftet_amd import hip_ops
    B, tets = 3, mesh()
    pos, vols = ref.uniform_vertices(B, V, 5).to(DEV), gpu_volumes(B, grad=False)
    with torch.no_grad():
        whole = hip_ops.tet_centroid_sample(vols, pos, tets.to(DEV))
        parts = [hip_ops.tet_centroid_sample(vols, pos, tets.to(DEV), first=f, count=500) for f in range(0, T, 500)]
    assert not whole.requires_grad and whole.shape == (B, C_FEAT + 3, T) and torch.equal(torch.cat(parts, 2), whole)


# ---------------------------------------------------------------------------- 5. determinism
def test_two_runs_give_the_same_bits():
    B, tets = 3, mesh()
    once = torch.randperm(T, generator=rng(6))[:400]
    sel = {"select": torch.cat([once, once[:100]])}
    pos, csr = ref.uniform_vertices(B, V, 7), csr_of(tets)
    a, b = run(B, pos, tets, sel, csr=csr), run(B, pos, tets, sel, csr=csr)
    for x, y in zip([a[0], a[1], a[4], a[5]] + a[3], [b[0], b[1], b[4], b[5]] + b[3]):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------- 6. bad indices
def test_a_tet_index_past_the_list_is_flagged_or_nan():
    from deftet_amd import hip_ops
    B, tets = 2, mesh()
    pos = ref.uniform_vertices(B, V, 8)
    clean = selection(65)["select"]
    dirty = clean.clone()
    dirty[[3, 40]] = torch.tensor([T, -1])
    with pytest.raises(RuntimeError, match="outside"):
        hip_ops.tet_centroid_sample(gpu_volumes(B), pos.to(DEV), tets.to(DEV), select=dirty.to(DEV), check=True)
    hip_ops.tet_centroid_sample(gpu_volumes(B), pos.to(DEV), tets.to(DEV), select=clean.to(DEV), check=True)
    good = run(B, pos, tets, {"select": clean})
    out, cent, gout, gvols, gcent, gpos = run(B, pos, tets, {"select": dirty})
    keep = np.setdiff1d(np.arange(65), [3, 40])
    assert torch.isnan(out[:, :, [3, 40]]).all() and torch.isnan(cent[:, [3, 40]]).all()
    assert same_bits(out[:, :, keep], good[0][:, :, keep]) and same_bits(cent[:, keep], good[1][:, keep])
    assert not bits(gcent[:, [3, 40]]).any() and same_bits(gcent[:, keep], good[4][:, keep])
    assert all(torch.isfinite(g).all() for g in gvols) and torch.isfinite(gpos).all()
    assert same_bits(gpos, ref.vertex_reduction(gcent, tets, V, select=dirty))            # the two slots add to no vertex


def test_a_vertex_index_past_the_positions_is_flagged_or_nan():
    from deftet_amd import hip_ops
    B = 2
    tets = mesh().clone()
    tets[[7, 900], [2, 0]] = torch.tensor([V, -5])
    pos = ref.uniform_vertices(B, V, 9).to(DEV)
    with pytest.raises(RuntimeError, match="outside"):
        hip_ops.tet_centroid_sample(gpu_volumes(B), pos, tets.to(DEV), check=True)
    vols = gpu_volumes(B)
    out, cent = hip_ops.tet_centroid_sample(vols, pos, tets.to(DEV), return_centroids=True)
    good = hip_ops.tet_centroid_sample(gpu_volumes(B), pos, mesh().to(DEV))
    keep = np.setdiff1d(np.arange(T), [7, 900])
    assert torch.isnan(out[:, :, [7, 900]]).all() and torch.isnan(cent[:, [7, 900]]).all()
    assert same_bits(out[:, :, keep], good[:, :, keep])
    gout = torch.randn(out.shape, generator=rng(1)).to(DEV)
    out.backward(gout)
    gcent = hip_ops.tet_centroid_sample_bwd_pos([v.detach() for v in vols], cent, gout)
    assert all(torch.isfinite(v.grad).all() for v in vols) and torch.isfinite(gcent).all() and not bits(gcent[:, [7, 900]]).any()


# ---------------------------------------------------------------------------- 7. the module routes
def test_module_routes_agree_with_the_torch_composition_on_the_gpu():
    from deftet_amd.layers.DefTet.deftet import TetTopology
    B, tets = 3, mesh()
    tet_bxfx4 = tets.to(DEV)[None].expand(B, -1, -1).contiguous()
    pos0 = ref.lattice_vertices(B, V, 40)
    center_idx = torch.randperm(T, generator=rng(41))[:257].to(DEV)
    res = {}
    for name in ("torch", "topology", "pointvoxel"):
        vols, pos = gpu_volumes(B), pos0.to(DEV).requires_grad_(True)
        if name == "torch":
            out = ref.decode_occ_composition(pos, tet_bxfx4, vols, center_idx=center_idx)
        elif name == "topology":
            out = TetTopology(tet_bxfx4, V).centroid_sample(vols, pos, select=center_idx)
        else:
            out, idx = callers.decode_occ_input(pos, vols, tet_bxfx4, use_mask=True, n_select=257, generator=rng(41))
            assert torch.equal(idx, center_idx)
        out.backward(torch.randn(out.shape, generator=rng(42)).to(DEV))
        assert pos.is_leaf and pos.grad is not None and all(v.grad is not None for v in vols)
        res[name] = [out.detach(), pos.grad] + [v.grad for v in vols]
    for name in ("topology", "pointvoxel"):
        for k, (a, b) in enumerate(zip(res[name], res["torch"])):
            check_close("tcs.route.%s.%d" % (name, k), a, b, BOUND)
    for a, b in zip(res["topology"], res["pointvoxel"]):
        assert torch.equal(a, b)
    # split_decode_occ's walk: ranges of 400 and the remainder of 300, against the composition on the sliced list
    with torch.no_grad():
        vols, pos = gpu_volumes(B, grad=False), pos0.to(DEV)
        feats = callers.split_decode_occ_inputs(pos, vols, tet_bxfx4, 400)
        assert [f.shape[2] for f in feats] == [400, 400, 400, 300]
        want = ref.decode_occ_composition(pos, tet_bxfx4, vols)
        check_close("tcs.route.split", torch.cat(feats, 2), want, BOUND)


# ---------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_raise():
    from deftet_amd import hip_ops
    B = 2
    vol, pos, tets = torch.zeros(B, 3, 4, 4, 4, device=DEV), torch.zeros(B, 10, 3, device=DEV), mesh(n_vertex=10, n_tet=20).to(DEV)
    sel = torch.arange(5, device=DEV)
    f = hip_ops.tet_centroid_sample
    bad = [lambda: f([vol.double()], pos, tets), lambda: f([vol], pos.half(), tets), lambda: f([vol], pos, tets.float()),
           lambda: f([vol], pos, tets, select=sel.float()),
           lambda: f([vol], pos[:, :, :2], tets), lambda: f([vol], pos[0], tets), lambda: f([vol], pos, tets[:, :3]),
           lambda: f([vol[:1]], pos, tets), lambda: f([vol[:, :, :, :, :3]], pos, tets), lambda: f([vol] * 9, pos, tets),
           lambda: f([vol], pos, tets, select=sel, count=5), lambda: f([vol], pos, tets, select=sel, first=2),
           lambda: f([vol], pos, tets, first=16, count=5), lambda: f([vol], pos, tets, first=-1),
           lambda: f([vol], pos, tets, csr=hip_ops.tet_vertex_csr(tets[:10], 10)),
           lambda: f([vol.cpu()], pos, tets), lambda: f([vol], pos, tets.cpu())]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail("case %d did not raise" % k)
    assert f([vol] * 8, pos, tets, select=sel).shape == (B, 27, 5)
