"""Connected tet components and the occupancy clean-up on the GPU against the numpy restatement (tests/tet_components_ref.py):
every output of every shape with array_equal — all of them are integers, there is no tolerance — and nothing is compared against
the library itself.  The figures of the masks (sizes, counts, the 399-step chain) are asserted on the reference side in
tests/test_tet_components_cpu.py."""
import os

import numpy as np
import pytest
import torch

from tests import surface_extract_ref as SX
from tests import tet_components_ref as R

pytestmark = pytest.mark.gpu
_grids = {}


def grid(res):
    if res not in _grids:
        _grids[res] = R.grid(res)
    return _grids[res]


def table(cuda, nbr):
    from deftet_amd import hip_ops
    t32 = torch.from_numpy(np.ascontiguousarray(nbr, np.int32)).to(cuda)
    return hip_ops.TetFaceNeighbours(t32.long(), t32)


def np_(x):
    return x.cpu().numpy()


def check_components(cuda, masks, nbr, dev_nbr=None, dtype=torch.bool, want=None):
    """hip_ops.tet_components of the batch `masks` [B,T] against the restatement, shape by shape; returns the restated shapes"""
    from deftet_amd import hip_ops
    masks = np.asarray(masks)
    dev_nbr = dev_nbr or table(cuda, nbr)
    c = hip_ops.tet_components(torch.from_numpy(masks).to(cuda).to(dtype), dev_nbr)
    assert c.labels.dtype == torch.int32 and c.sizes.dtype == torch.int32 and c.open.dtype == torch.bool and c.count.dtype == torch.int32
    assert c.labels.shape == masks.shape and c.sizes.shape == masks.shape and c.open.shape == masks.shape and c.count.shape == masks.shape[:1]
    want = want or [R.components(m, nbr) for m in masks]
    for b, w in enumerate(want):
        assert np.array_equal(np_(c.labels[b]), w["labels"]), b
        assert np.array_equal(np_(c.sizes[b]), w["sizes"]), b
        assert np.array_equal(np_(c.open[b]), w["open"]), b
        assert int(c.count[b]) == w["count"], b
    return want


OPTIONS = [dict(), dict(keep_largest=True), dict(min_size=3), dict(fill_voids=True), dict(keep_largest=True, min_size=5, fill_voids=True)]


def check_cleanup(cuda, masks, nbr, dev_nbr=None, options=OPTIONS):
    from deftet_amd import hip_ops
    masks = np.asarray(masks)
    dev_nbr = dev_nbr or table(cuda, nbr)
    m = torch.from_numpy(masks).to(cuda)
    for opt in options:
        keep = hip_ops.occupancy_cleanup(m, dev_nbr, **opt)
        assert keep.dtype == torch.bool and keep.shape == masks.shape
        for b in range(masks.shape[0]):
            assert np.array_equal(np_(keep[b]), R.cleanup(masks[b], nbr, **opt)), (opt, b)


@pytest.mark.parametrize("res", [4, 10])
def test_random_masks_on_small_grids(cuda, res):
    """T = 48 is less than one wave, T = 750 no multiple of 64 or 256"""
    _tets, _V, nbr, _cen = grid(res)
    T = nbr.shape[0]
    masks = np.stack([R.random_mask(T, 0.3, res), R.random_mask(T, 0.5, res + 1)])
    check_components(cuda, masks, nbr)
    check_cleanup(cuda, masks, nbr)
    # uint8 and float inputs: non-zero is inside; one shape without the batch dimension
    from deftet_amd import hip_ops
    check_components(cuda, masks * 7, nbr, dtype=torch.uint8)
    check_components(cuda, masks * -0.25, nbr, dtype=torch.float32)
    one = hip_ops.tet_components(torch.from_numpy(masks[0]).to(cuda), table(cuda, nbr))
    w = R.components(masks[0], nbr)
    assert one.labels.shape == (T,) and one.count.shape == (1,) and np.array_equal(np_(one.labels), w["labels"])
    assert np.array_equal(np_(one.sizes), w["sizes"]) and np.array_equal(np_(one.open), w["open"]) and int(one.count[0]) == w["count"]
    keep = hip_ops.occupancy_cleanup(torch.from_numpy(masks[1]).to(cuda), table(cuda, nbr), keep_largest=True)
    assert keep.shape == (T,) and np.array_equal(np_(keep), R.cleanup(masks[1], nbr, keep_largest=True))


def masks16():
    _tets, _V, nbr, cen = grid(16)
    T = nbr.shape[0]
    named = dict(shell=R.shell(cen), balls=R.two_balls(cen), snake=R.snake(16), r30=R.random_mask(T, 0.3), r50=R.random_mask(T, 0.5),
                 full=np.ones(T, bool), empty=np.zeros(T, bool))
    for k in range(6):
        named["sixth%d" % k] = R.every_sixth(T, k)
    return named


def test_res16_masks(cuda):
    """twelve 256-tet workgroups per shape; every mask as one shape of one batch"""
    _tets, _V, nbr, _cen = grid(16)
    named = masks16()
    masks = np.stack(list(named.values()))
    want = dict(zip(named, check_components(cuda, masks, nbr)))
    assert want["shell"]["count"] == 1 and want["shell"]["sizes"].max() == 696
    assert sorted(want["balls"]["sizes"][want["balls"]["sizes"] > 0].tolist()) == [48, 48]
    assert want["snake"]["count"] == 1 and want["snake"]["sizes"].max() == 888
    assert all(want["sixth%d" % k]["count"] == 512 for k in range(6))
    assert want["r30"]["count"] == 444 and want["r50"]["count"] == 213
    assert want["full"]["count"] == 1 and want["full"]["sizes"][0] == 3072 and want["empty"]["count"] == 0
    check_cleanup(cuda, masks, nbr)


def test_res16_selection(cuda):
    from deftet_amd import hip_ops
    _tets, _V, nbr, cen = grid(16)
    dn = table(cuda, nbr)
    shell, balls = R.shell(cen), R.two_balls(cen)
    filled = hip_ops.occupancy_cleanup(torch.from_numpy(shell).to(cuda), dn, fill_voids=True)
    assert int(filled.sum()) == 696 + 108 and np.array_equal(np_(filled), R.cleanup(shell, nbr, fill_voids=True))
    keep, comps = hip_ops.occupancy_cleanup(torch.from_numpy(balls).to(cuda), dn, keep_largest=True, return_components=True)
    roots = np.nonzero(R.components(balls, nbr)["sizes"])[0]
    assert int(keep.sum()) == 48 and np.array_equal(np_(keep), R.components(balls, nbr)["labels"] == roots[0])
    w = R.components(balls, nbr)                                       # the components the selection was made on
    assert np.array_equal(np_(comps.labels), w["labels"]) and np.array_equal(np_(comps.sizes), w["sizes"])
    assert np.array_equal(np_(comps.open), w["open"]) and int(comps.count[0]) == 2
    assert not bool(hip_ops.occupancy_cleanup(torch.from_numpy(balls).to(cuda), dn, min_size=49).any())
    assert np.array_equal(np_(hip_ops.occupancy_cleanup(torch.from_numpy(balls).to(cuda), dn, min_size=48)), balls)
    # with fill_voids the returned components are those of the filled mask
    _k, comps = hip_ops.occupancy_cleanup(torch.from_numpy(shell).to(cuda), dn, fill_voids=True, return_components=True)
    w = R.components(R.cleanup(shell, nbr, fill_voids=True), nbr)
    assert np.array_equal(np_(comps.labels), w["labels"]) and np.array_equal(np_(comps.sizes), w["sizes"]) and w["sizes"].max() == 804


@pytest.mark.parametrize("name", ["shell", "balls", "snake", "r30", "r50", "sixth2", "full"])
def test_permuted_numbering(cuda, name):
    """the tet list in a random order: the partition is the unpermuted one carried through the permutation, the labels are the
    restatement's on the permuted input; every component's smallest index now lies far from its neighbours"""
    tets, _V, nbr, _cen = grid(16)
    mask = masks16()[name]
    _tets_p, nbr_p, mask_p, perm = R.permuted(tets, mask, 16)
    want = check_components(cuda, mask_p[None], nbr_p)[0]
    assert np.array_equal(want["labels"], R.labels_through(R.components(mask, nbr)["labels"], perm))
    check_cleanup(cuda, mask_p[None], nbr_p, options=[dict(keep_largest=True, fill_voids=True)])


def test_three_shapes_in_one_call_and_repeatability(cuda):
    from deftet_amd import hip_ops
    _tets, _V, nbr, cen = grid(16)
    dn = table(cuda, nbr)
    masks = np.stack([R.shell(cen), R.two_balls(cen), R.random_mask(nbr.shape[0], 0.5, 3)])
    m = torch.from_numpy(masks).to(cuda)
    batch = hip_ops.tet_components(m, dn)
    again = hip_ops.tet_components(m, dn)
    opt = dict(keep_largest=True, min_size=2, fill_voids=True)
    keep, keep2 = hip_ops.occupancy_cleanup(m, dn, **opt), hip_ops.occupancy_cleanup(m, dn, **opt)
    assert torch.equal(keep, keep2)
    for b in range(3):
        single = hip_ops.tet_components(m[b:b + 1], dn)
        for x, y, z in zip(batch, again, single):
            assert torch.equal(x[b], y[b]) and torch.equal(x[b], z[0])
        assert torch.equal(keep[b], hip_ops.occupancy_cleanup(m[b:b + 1], dn, **opt)[0])
    check_components(cuda, masks, nbr, dn)


def test_out_of_range_neighbour_raises_and_is_not_followed(cuda):
    from deftet_amd import hip_ops
    _tets, _V, nbr, cen = grid(16)
    T = nbr.shape[0]
    mask = R.two_balls(cen)
    roots = np.nonzero(R.components(mask, nbr)["sizes"])[0]
    dirty = nbr.copy()
    t = int(roots[1])                                                   # a tet of the second ball
    i = int(np.nonzero(dirty[t] >= 0)[0][0])
    dirty[t, i] = T
    dn = table(cuda, dirty)
    m = torch.from_numpy(mask).to(cuda)
    with pytest.raises(RuntimeError, match="a neighbour index is out of range"):
        hip_ops.tet_components(m, dn)
    with pytest.raises(RuntimeError, match="a neighbour index is out of range"):
        hip_ops.occupancy_cleanup(m, dn, keep_largest=True, fill_voids=True)
    c = hip_ops.tet_components(m, dn, check=False)                      # the entry is skipped: the restatement on the same table
    w = R.components(mask, dirty)
    assert np.array_equal(np_(c.labels), w["labels"]) and np.array_equal(np_(c.sizes), w["sizes"])
    first = R.components(mask, nbr)["labels"] == roots[0]               # the ball the entry does not touch
    assert np.array_equal(np_(c.labels)[first], np.full(48, roots[0], np.int32))
    torch.cuda.synchronize()


def test_full_size_two_shapes(cuda):
    """res 70, T = 257,250: the one case where a component spans thousands of workgroups"""
    from deftet_amd import hip_ops
    _tets, _V, nbr, cen = grid(70)
    assert nbr.shape[0] == 257250
    masks = np.stack([R.sphere_with_floaters(cen), R.shell(cen, 0.2, 0.35)])
    want = check_components(cuda, masks, nbr)
    assert want[0]["count"] == 4 and sorted(want[0]["sizes"][want[0]["sizes"] > 0].tolist()) == [120, 120, 120, 29178]
    assert want[1]["count"] == 1
    dn = table(cuda, nbr)
    keep = hip_ops.occupancy_cleanup(torch.from_numpy(masks).to(cuda), dn, keep_largest=True, fill_voids=True)
    for b in range(2):
        assert np.array_equal(np_(keep[b]), R.cleanup(masks[b], nbr, keep_largest=True, fill_voids=True)), b
    assert int(keep[0].sum()) == 29178 and int(keep[1].sum()) == 46206  # the floaters gone, the shell's cavity filled


# ---------------------------------------------------------------------------- callers
def test_clean_occupancy_feeds_binary_extraction(cuda):
    from deftet_amd import grids, hip_ops
    from deftet_amd.layers.DefTet.deftet import DefTet
    tets, V, nbr, cen = grid(16)
    verts, _ = grids.kuhn_grid(16)
    T = nbr.shape[0]
    dn = table(cuda, nbr)
    pos = grids.jittered_positions(verts, 16, 2)
    tet_p = grids.gather_tets(pos, tets)
    floater = R.balls(cen, [(0, 0, 0)], 0.3) | R.balls(cen, [(0.4, 0.4, 0.4)], 0.12)
    assert R.components(floater, nbr)["count"] == 2
    occ = np.stack([R.shell(cen), floater]).astype(np.float32)
    net = DefTet(device=cuda)
    for shape, opt in (((2, T), dict()), ((2, T, 1), dict(fill_voids=True)), ((2, T), dict(keep_largest=False, min_size=30))):
        full = dict(keep_largest=True, min_size=0, fill_voids=False)
        full.update(opt)
        clean = net.clean_occupancy(torch.from_numpy(occ.reshape(shape)).to(cuda), dn, **opt)
        assert clean.dtype == torch.float32 and tuple(clean.shape) == shape
        want = np.stack([R.cleanup(occ[b] > 0.5, nbr, **full) for b in range(2)]).astype(np.float32)
        assert np.array_equal(np_(clean).reshape(2, T), want)
        soup = hip_ops.surface_extract(torch.from_numpy(tet_p).to(cuda), clean, dn, "binary")
        for b in range(2):
            ref = SX.extract(tet_p[b], want[b], nbr.astype(np.int64), "binary")
            assert np.array_equal(np_(soup.face[b]), ref["face"]) and ref["face"].shape[0] > 0
    assert want[1].sum() == R.balls(cen, [(0, 0, 0)], 0.3).sum()        # (min_size = 30 dropped the floater, and only it)
    # soft values: a dropped tet gets 0, a filled one 1, the others keep their value
    soft = (occ * 0.8 + 0.1).astype(np.float32)
    clean = np_(net.clean_occupancy(torch.from_numpy(soft).to(cuda), dn, fill_voids=True))
    keep = np.stack([R.cleanup(soft[b] > 0.5, nbr, keep_largest=True, fill_voids=True) for b in range(2)])
    ins = soft > 0.5
    assert np.array_equal(clean, np.where(keep, np.where(ins, soft, 1), np.where(ins, 0, soft)).astype(np.float32))


def test_save_surface_objs_defaults_unchanged_and_cleaned(cuda, tmp_path):
    from deftet_amd import grids, hip_ops
    from deftet_amd.render import export
    tets, V, nbr, cen = grid(16)
    verts, _ = grids.kuhn_grid(16)
    dn = table(cuda, nbr)
    pos = (verts - 0.5).astype(np.float32)
    # per-vertex weights: high in a ball at the centre and in a small one in a corner, low elsewhere
    d0, d1 = np.linalg.norm(verts - 0.5, axis=1), np.linalg.norm(verts - 0.5 - 0.38, axis=1)
    rng = np.random.default_rng(1)
    w = (np.where((d0 < 0.3) | (d1 < 0.08), 0.9, 0.001) * (1 + 0.05 * rng.random(V))).astype(np.float32)
    col = rng.random((V, 3)).astype(np.float32)
    dev = lambda x: torch.from_numpy(x).to(cuda)
    thresholds = (0.05, 0.25)
    tet_p, tet_c = pos[tets.astype(np.int64)], col[:, ::-1][tets.astype(np.int64)]
    occ = SX.occ_from_weights(w, tets)

    def files(d):
        return {os.path.basename(p): open(p, "rb").read() for p in d}

    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
    plain = files(export.save_surface_objs(dev(pos), (dev(w), dev(col)), tets, dn, str(tmp_path / "a"), "x", thresholds=thresholds))
    cleaned = files(export.save_surface_objs(dev(pos), (dev(w), dev(col)), tets, dn, str(tmp_path / "b"), "x", thresholds=thresholds,
                                             keep_largest=True))
    assert sorted(plain) == sorted(cleaned) and len(plain) == 4
    for h in thresholds:
        # defaults: the text of the extraction on the uncleaned occupancy, as before the keywords existed
        ref = SX.extract(tet_p, occ, nbr.astype(np.int64), "threshold", h, attr_tx4xc=tet_c)
        assert plain["tet-geo-x-thres-%.3f.obj" % h] == SX.obj_text(ref["face"]).encode()
        assert plain["tet-color-x-thres-%.3f.obj" % h] == SX.obj_color_text(ref["face"], ref["face_attr"]).encode()
        # keep_largest: the soup of the cleaned occupancy
        ins = occ > np.float32(2 * h)
        keep = R.cleanup(ins, nbr, keep_largest=True)
        assert R.components(ins, nbr)["count"] >= 2 and 0 < keep.sum() < ins.sum()
        occ_c = np.where(keep, occ, np.where(ins, np.float32(0), occ)).astype(np.float32)
        ref_c = SX.extract(tet_p, occ_c, nbr.astype(np.int64), "threshold", h, attr_tx4xc=tet_c)
        assert 0 < ref_c["face"].shape[0] < ref["face"].shape[0]
        assert cleaned["tet-geo-x-thres-%.3f.obj" % h] == SX.obj_text(ref_c["face"]).encode()
        assert cleaned["tet-color-x-thres-%.3f.obj" % h] == SX.obj_color_text(ref_c["face"], ref_c["face_attr"]).encode()
