"""GPU tests of the pixel-aligned image-feature operator (image_sample.hip) against the fp64 restatement of
tests/image_sample_ref.py: values and every gradient within the standing 1e-5 max-norm bound, the layout of the one result, long
and partially-outside segments, hostile coordinates, bit-reproducibility, the imagefeat front ends against the torch composition,
empty and non-contiguous inputs and the workspace check."""
import json
import os
import re
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_sample_ref as ref
from tests import tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5

# Every comparison is tests.tol.check_close at BOUND, one call per case.  The size grid alone makes some 1,300 of them, so with
# DEFTET_TOLERANCE_REPORT set the file gets one row per group of cases (the name without its batch, point count, padding and
# align_corners parts) instead of one per call: the largest measured errors of the group, the case they belong to and the count.
_worst = {}
_VARIANT = re.compile(r"^(B\d+|N\d+|G\d+|A\d+|a[01]|zeros|border)$")


def check_close(name, got, want, maxnorm):
    report = os.environ.get("DEFTET_TOLERANCE_REPORT")
    if not report:
        return tol.check_close(name, got, want, maxnorm)
    fd, one = tempfile.mkstemp(suffix=".jsonl")
    os.close(fd)
    os.environ["DEFTET_TOLERANCE_REPORT"] = one                      # tol.check_close writes its row before it asserts
    try:
        return tol.check_close(name, got, want, maxnorm)
    finally:
        os.environ["DEFTET_TOLERANCE_REPORT"] = report
        rows = [json.loads(line) for line in open(one)]
        os.unlink(one)
        for r in rows:
            group = ".".join(t for t in name.split(".") if not _VARIANT.match(t))
            w = _worst.setdefault(group, {"name": group, "calls": 0, "maxnorm_err": -1.0, "worst_case": None, "elem_rel_err": 0.0,
                                          "asserted_maxnorm": maxnorm})
            w["calls"] += 1
            w["elem_rel_err"] = max(w["elem_rel_err"], r["elem_rel_err"])
            if r["maxnorm_err"] > w["maxnorm_err"]:
                w["maxnorm_err"], w["worst_case"] = r["maxnorm_err"], name


@pytest.fixture(scope="module", autouse=True)
def _write_grouped_report():
    yield
    report = os.environ.get("DEFTET_TOLERANCE_REPORT")
    if report and _worst:
        with open(report, "a") as f:
            f.write("".join(json.dumps(_worst[k]) + "\n" for k in sorted(_worst)))


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy(), np.float32).view(np.uint32)


def rng(seed):
    return torch.Generator().manual_seed(seed)


def uniform_uv(B, N, seed):
    return 3.0 * torch.rand(B, N, 2, generator=rng(seed)) - 1.5


def run_gpu(maps, uv, glob=None, app=None, padding_mode="zeros", align=False, need_uv=True, gout=None):
    """(out, gout, grad_maps, grad_uv, grad_glob, grad_app) of hip_ops.image_sample on the GPU"""
    from deftet_amd import hip_ops
    m = [x.to(DEV).requires_grad_(True) for x in maps]
    u = uv.to(DEV).requires_grad_(need_uv)
    g = glob.to(DEV).requires_grad_(True) if glob is not None else None
    a = app.to(DEV).requires_grad_(True) if app is not None else None
    out = hip_ops.image_sample(m, u, global_features=g, append=a, padding_mode=padding_mode, align_corners=align)
    if gout is None:
        gout = torch.randn(out.shape, generator=rng(11))
    if out.requires_grad:
        out.backward(gout.to(DEV))
    return out, gout, [x.grad for x in m], u.grad, None if g is None else g.grad, None if a is None else a.grad


def check(name, maps, uv, glob=None, app=None, padding_mode="zeros", align=False, check_uv=False, only_uv=False):
    """the operator on the GPU against the fp64 restatement on the same fp32 inputs: values, every map's gradient, with check_uv
    the gradient to uv (only_uv: nothing else), the gradients to the global features and the appended rows where they are given"""
    out, gout, gm, guv, gg, ga = run_gpu(maps, uv, glob, app, padding_mode, align, need_uv=check_uv)
    m = [x.double().requires_grad_(True) for x in maps]
    u = uv.double().requires_grad_(True)
    g = glob.double().requires_grad_(True) if glob is not None else None
    a = app.double().requires_grad_(True) if app is not None else None
    want = ref.image_sample(m, u, g, a, padding_mode, align)
    assert out.shape == want.shape and out.is_contiguous() and out.dtype == torch.float32
    if not only_uv:
        check_close(name + ".values", out, want, BOUND)
    if want.requires_grad:
        want.backward(gout.double())
    for k, (x, y) in enumerate(zip(gm, m)):
        if not only_uv:
            check_close("%s.grad_map%d" % (name, k), x, y.grad, BOUND)
    if check_uv:
        check_close(name + ".grad_uv", guv, u.grad if u.grad is not None else torch.zeros_like(u), BOUND)
    if g is not None:
        check_close(name + ".grad_global", gg, g.grad, BOUND)
    if a is not None:
        assert np.array_equal(bits(ga), bits(gout[:, gout.shape[1] - app.shape[2]:, :].permute(0, 2, 1)))
    return out, gout, gm, guv


# ---------------------------------------------------------------------------- values and gradients over the size grid
@pytest.mark.parametrize("C", [1, 7, 64, 130])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4), (64, 64)])
def test_sampler_matches_the_fp64_restatement(H, W, C):
    """values and the map's gradient on uniform points over [-1.5, 1.5]^2, the gradient to uv on the interior construction (where
    it is continuous).  Measured on an MI355X, largest max-norm error over the 64 x 64 cases: 1.6e-7 (values), 1.4e-7 (grad_map),
    7.0e-6 (grad_uv); below 7e-7 at the smaller maps.  The pixel coordinate is itself an fp32 number: at ix in [32, 64) its last
    bit is 3.8e-6 of a pixel, and the interior construction (built in fp64, rounded to fp32) exercises every bit of it, where
    3 rand - 1.5 does not.  Values and grad_map on the interior points stay below 5.4e-6 with ONE exception, which is why they are
    not among the comparisons made here: a single value compared with itself where the four products cancel — one point, one
    channel, 64 x 64, interior seed 2 — is 0.0292648 against 0.0292664 in fp64: 1.6e-6 apart, 5.6e-5 of itself."""
    for B in (1, 3):
        m = torch.randn(B, C, H, W, generator=rng(C + B))
        for N in (1, 63, 64, 65, 1000):
            for padding_mode in ("zeros", "border"):
                for align in ((False, True) if (H, W) == (5, 4) else (False,)):
                    tag = "is.%dx%d.B%d.C%d.N%d.%s.a%d" % (H, W, B, C, N, padding_mode, align)
                    check(tag + ".uniform", [m], uniform_uv(B, N, N), padding_mode=padding_mode, align=align)
                    check(tag + ".interior", [m], ref.interior_uv(B, N, H, W, align, rng(N + 1)), padding_mode=padding_mode, align=align,
                          check_uv=True, only_uv=True)


# ---------------------------------------------------------------------------- layout of the one result
@pytest.mark.parametrize("with_append", [False, True])
@pytest.mark.parametrize("G", [0, 1, 5])
def test_rows_land_at_their_offsets(G, with_append):
    B, N = 2, 257
    maps = [torch.randn(B, 3, 8, 8, generator=rng(1)), torch.randn(B, 5, 5, 4, generator=rng(2)), torch.randn(B, 2, 8, 8, generator=rng(3))]
    g = rng(4)
    # pixel fractions away from the integers at 8 x 8 and at 5 x 4 alike (there the gradient to uv jumps): the first N of a
    # larger uniform draw over [-1.2, 1.2]^2 that keep 0.01 of distance at both sizes
    cand = (2.4 * torch.rand(B, 8 * N, 2, generator=g) - 1.2)
    ok = torch.ones(B, 8 * N, dtype=torch.bool)
    for size in ((8, 8), (5, 4)):
        pix = torch.stack([ref.unnormalise(cand[..., 0].double(), size[1], False), ref.unnormalise(cand[..., 1].double(), size[0], False)], -1)
        frac = pix - torch.floor(pix)
        ok &= ((frac > 0.01) & (frac < 0.99)).all(-1)
    assert int(ok.sum(1).min()) >= N
    uv = torch.stack([cand[b][ok[b]][:N] for b in range(B)])
    glob = torch.randn(B, G, generator=g) if G else None
    app = torch.randn(B, N, 3, generator=g) if with_append else None
    out, gout, gm, guv = check("is.layout.G%d.A%d" % (G, with_append), maps, uv, glob, app, check_uv=True)
    assert out.shape == (B, G + 10 + (3 if with_append else 0), N)
    if G:
        assert np.array_equal(bits(out[:, :G]), bits(glob[:, :, None].expand(B, G, N)))
    if with_append:
        assert np.array_equal(bits(out[:, G + 10:]), bits(app.permute(0, 2, 1)))
    from deftet_amd import hip_ops
    for k, (lo, hi) in enumerate(((0, 3), (3, 8), (8, 10))):          # each map's rows are what the map gives alone
        alone = hip_ops.image_sample([maps[k].to(DEV)], uv.to(DEV))
        assert np.array_equal(bits(out[:, G + lo:G + hi]), bits(alone))


# ---------------------------------------------------------------------------- segments
def test_long_partial_and_sparse_segments():
    B, N, H, W = 2, 1000, 8, 8
    m = torch.randn(B, 7, H, W, generator=rng(3))
    one = (torch.full((B, N), 5), torch.full((B, N), 2))              # every point in one cell: a segment longer than a workgroup
    check("is.onecell", [m], ref.interior_uv(B, N, H, W, False, rng(4), cells=one), check_uv=True)
    for n in (32, 33, 64, 65, 129):                                   # either side of the length at which a wave takes the segment over
        cells = (one[0][:, :n], one[1][:, :n])
        check("is.onecell.N%d" % n, [m], ref.interior_uv(B, n, H, W, False, rng(n), cells=cells), check_uv=True)
    corner = (torch.full((B, N), -1), torch.full((B, N), -1))         # lo = (-1, -1): only texel (0, 0) is in the map
    out, gout, gm, _ = check("is.cornercell", [m], ref.interior_uv(B, N, H, W, False, rng(5), cells=corner), check_uv=True)
    assert bool(gm[0][:, :, 0, 0].abs().min() > 0) and not gm[0][:, :, 1:, :].any() and not gm[0][:, :, :, 1:].any()
    for cells in ((torch.full((B, N), W - 1), torch.full((B, N), H - 1)), (torch.full((B, N), -1), torch.full((B, N), 3))):
        for padding_mode in ("zeros", "border"):
            check("is.edgecell.%s" % padding_mode, [m], ref.interior_uv(B, N, H, W, False, rng(6), cells=cells), padding_mode=padding_mode,
                  check_uv=True)
    m64 = torch.randn(B, 3, 64, 64, generator=rng(7))                 # 1000 points over 65 x 65 cells: most cells empty
    check("is.sparse", [m64], ref.interior_uv(B, N, 64, 64, False, rng(8)), check_uv=True)
    check("is.sparse1500", [m64], ref.interior_uv(B, 1500, 64, 64, False, rng(9)), check_uv=True)


# ---------------------------------------------------------------------------- hostile coordinates
BAD = [1e30, -1e30, float("inf"), -float("inf"), float("nan")]


def hostile_uv(B, n_good, H, W, seed):
    """(uv [B, n_good + 15, 2], is_bad [n], bad_coord [n,2]): interior points with (bad, 0.1), (0.1, bad), (bad, bad) spread among them"""
    good = ref.interior_uv(B, n_good, H, W, False, rng(seed))
    rows = [[v, 0.1] for v in BAD] + [[0.1, v] for v in BAD] + [[v, v] for v in BAD]
    bad = torch.tensor(rows, dtype=torch.float32)[None].expand(B, -1, -1)
    uv = torch.cat([good, bad], 1)
    order = torch.randperm(uv.shape[1], generator=rng(seed + 1))
    is_bad = (torch.arange(uv.shape[1]) >= n_good)[order]
    uv = uv[:, order].contiguous()
    bad_coord = ~torch.isfinite(uv[0]) | (uv[0].abs() > 1e20)
    return uv, is_bad, bad_coord


def test_hostile_coordinates_under_zeros():
    B, H, W = 2, 8, 8
    m = torch.randn(B, 5, H, W, generator=rng(1))
    uv, is_bad, _ = hostile_uv(B, 300, H, W, 2)
    out, gout, gm, guv = check("is.hostile.zeros", [m], uv, check_uv=True)
    assert not out[:, :, is_bad.to(DEV)].any() and not guv[:, is_bad.to(DEV)].any()
    assert bool(torch.isfinite(gm[0]).all())
    keep = ~is_bad                                                    # the run without them: the same bits in the map's gradient
    gm2 = run_gpu([m], uv[:, keep].contiguous(), gout=gout[:, :, keep].contiguous())[2]
    assert np.array_equal(bits(gm[0]), bits(gm2[0]))


def test_hostile_coordinates_under_border():
    B, H, W = 2, 8, 8
    m = torch.randn(B, 5, H, W, generator=rng(3))
    uv, is_bad, bad_coord = hostile_uv(B, 300, H, W, 4)
    out, gout, gm, guv = check("is.hostile.border", [m], uv, padding_mode="border", check_uv=True)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gm[0]).all()) and bool(torch.isfinite(guv).all())
    assert not guv[:, bad_coord.to(DEV)].any()
    both = bad_coord.all(1)
    assert int(both.sum()) == 5 and not guv[:, both.to(DEV)].any()


# ---------------------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bits():
    B, N = 2, 1000
    for name, m, uv in (("onecell", torch.randn(B, 7, 8, 8, generator=rng(1)),
                         ref.interior_uv(B, N, 8, 8, False, rng(2), cells=(torch.full((B, N), 5), torch.full((B, N), 2)))),
                        ("64x64", torch.randn(B, 33, 64, 64, generator=rng(3)), uniform_uv(B, 5000, 4))):
        glob = torch.randn(B, 6, generator=rng(5))
        gout = torch.randn(B, 6 + m.shape[1], uv.shape[1], generator=rng(6))
        a = run_gpu([m], uv, glob, gout=gout)
        b = run_gpu([m], uv, glob, gout=gout)
        for x, y in ((a[0], b[0]), (a[2][0], b[2][0]), (a[3], b[3]), (a[4], b[4])):
            assert np.array_equal(bits(x), bits(y)), name


# ---------------------------------------------------------------------------- the front ends of imagefeat.py
def grid_camera():
    """the camera of grids.project_faces: rotation Rx Ry, radius 4 along z, the projection vector (f, f, -1)"""
    import inspect
    from deftet_amd import grids
    d = {k: v.default for k, v in inspect.signature(grids.project_faces).parameters.items() if v.default is not inspect.Parameter.empty}
    ax, ay = d["rot"]
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    R = Rx @ Ry
    cam_pos = R.T @ np.array([0.0, 0.0, d["cam_z"]])
    return (torch.from_numpy(R).float()[None], torch.from_numpy(cam_pos).float()[None],
            torch.tensor([[d["focal"]], [d["focal"]], [-1.0]], dtype=torch.float32), d["coef"])


def torch_composition(pos, feats, uv, append):
    parts = [feats[0][:, :, None].expand(-1, -1, pos.shape[1])] if feats[0] is not None else []
    parts += [F.grid_sample(m, uv.unsqueeze(2), mode="bilinear", padding_mode="zeros", align_corners=False).squeeze(3) for m in feats[1:]]
    feat = torch.cat(parts, 1)
    return torch.cat([feat, pos.permute(0, 2, 1)], 1) if append else feat


def test_sample_f_and_extract_point_image_features_match_the_torch_composition():
    from deftet_amd import grids, imagefeat
    B, N, G = 2, 257, 4
    rot, cam_pos, proj, coef = grid_camera()
    rot, cam_pos = rot.expand(B, 3, 3).contiguous(), cam_pos.expand(B, 3).contiguous()
    verts = grids.kuhn_grid(12)[0]
    g = rng(1)
    pick = torch.randperm(verts.shape[0], generator=g)[:N]
    pos0 = ((torch.from_numpy(np.asarray(verts, np.float32))[pick] - 0.5)[None] + 0.02 * torch.randn(B, N, 3, generator=g)) * coef
    maps0 = [torch.randn(B, 3, 8, 8, generator=g), torch.randn(B, 5, 8, 8, generator=g), torch.randn(B, 4, 4, 4, generator=g)]
    glob0 = torch.randn(B, G, generator=g)
    gout = torch.randn(B, G + 12 + 3, N, generator=g)
    # ours, fp32 on the GPU
    pos = pos0.to(DEV).requires_grad_(True)
    feats = [glob0.to(DEV).requires_grad_(True)] + [m.to(DEV).requires_grad_(True) for m in maps0]
    out = imagefeat.sample_f(pos, feats, cam_pos.to(DEV), rot.to(DEV), proj.to(DEV))
    assert out.shape == (B, G + 12 + 3, N) and out.is_contiguous()
    out.backward(gout.to(DEV))
    # the composition, fp64 on the same GPU inputs
    pos_d = pos0.to(DEV).double().requires_grad_(True)
    feats_d = [glob0.to(DEV).double().requires_grad_(True)] + [m.to(DEV).double().requires_grad_(True) for m in maps0]
    uv_d = imagefeat.project_to_image(pos_d, rot.to(DEV).double(), cam_pos.to(DEV).double(), proj.to(DEV).double())
    assert float(uv_d.detach().abs().max()) > 0.5                              # the points do spread over the image
    want = torch_composition(pos_d, feats_d, uv_d, True)
    want.backward(gout.to(DEV).double())
    check_close("is.sample_f.values", out, want, BOUND)
    check_close("is.sample_f.grad_pos", pos.grad, pos_d.grad, BOUND)
    for k, (a, b) in enumerate(zip(feats, feats_d)):
        assert a.grad is not None and bool(a.grad.abs().sum() > 0)
        check_close("is.sample_f.grad_feat%d" % k, a.grad, b.grad, BOUND)
    # DISN's function: a camera matrix that does the same projection (row vector times matrix, divided by component 2)
    M = torch.zeros(B, 4, 4, dtype=torch.float64)
    Rt = rot.double().permute(0, 2, 1)                                # cam = (p - c) R^T = p R^T - c R^T
    scale = torch.tensor([float(proj[0]), -float(proj[1]), float(proj[2])], dtype=torch.float64)
    M[:, :3, :3] = Rt * scale
    M[:, 3, :3] = -torch.einsum("bi,bij->bj", cam_pos.double(), Rt) * scale
    pos2 = pos0.to(DEV).requires_grad_(True)
    maps2 = [m.to(DEV).requires_grad_(True) for m in maps0]
    got = imagefeat.extract_point_image_features(maps2, pos2, M.float().to(DEV))
    assert got.shape == (B, N, 12)
    pos2_d = pos0.to(DEV).double().requires_grad_(True)
    maps2_d = [m.to(DEV).double().requires_grad_(True) for m in maps0]
    uv2 = imagefeat.project_with_matrix(pos2_d, M.float().double().to(DEV))
    want2 = torch_composition(pos2_d, [None] + maps2_d, uv2, False).permute(0, 2, 1)
    check_close("is.extract.values", got, want2, BOUND)
    g2 = torch.randn(B, N, 12, generator=g).to(DEV)
    got.backward(g2)
    want2.backward(g2.double())
    check_close("is.extract.grad_pos", pos2.grad, pos2_d.grad, BOUND)
    for k, (a, b) in enumerate(zip(maps2, maps2_d)):
        check_close("is.extract.grad_map%d" % k, a.grad, b.grad, BOUND)
    single = imagefeat.extract_point_image_features(maps0[0].to(DEV), pos0.to(DEV), M.float().to(DEV))      # a single tensor, as in disn.py
    assert np.array_equal(bits(single), bits(got[:, :, :3]))


# ---------------------------------------------------------------------------- empty and odd inputs
def test_empty_and_non_contiguous_inputs():
    from deftet_amd import hip_ops
    B = 2
    m = torch.randn(B, 3, 5, 4, generator=rng(1))
    glob, app0 = torch.randn(B, 2, generator=rng(2)), torch.zeros(B, 0, 3)
    out, gout, gm, guv, gg, ga = run_gpu([m], torch.zeros(B, 0, 2), glob, app0)                              # N = 0
    assert out.shape == (B, 2 + 3 + 3, 0) and not gm[0].any() and gm[0].shape == m.shape and guv.shape == (B, 0, 2)
    assert not gg.any() and ga.shape == (B, 0, 3)
    uv = ref.interior_uv(B, 70, 5, 4, False, rng(3))
    app = torch.randn(B, 70, 3, generator=rng(4))
    out, gout, gm, guv = check("is.nomaps", [], uv, glob, app, check_uv=True)                                # K = 0
    assert out.shape == (B, 5, 70) and not guv.any()
    assert hip_ops.image_sample([], uv.to(DEV)).shape == (B, 0, 70)
    # non-contiguous map (a channel-last view) and uv (every other point of a longer set): the values of their contiguous copies
    mt = m.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    uv2 = torch.stack([uv, -uv], 2).reshape(B, 140, 2).to(DEV)[:, ::2].requires_grad_(True)
    assert not mt.is_contiguous() and not uv2.is_contiguous()
    got = hip_ops.image_sample([mt], uv2)
    want, gout, gm, guv = check("is.noncontig", [m], uv, check_uv=True)
    assert np.array_equal(bits(got), bits(want))
    got.backward(gout.to(DEV))
    assert np.array_equal(bits(mt.grad), bits(gm[0])) and np.array_equal(bits(uv2.grad), bits(guv))
    for call in (lambda: hip_ops.image_sample([m.to(DEV)], torch.zeros(B, 5, 3, device=DEV)),
                 lambda: hip_ops.image_sample([m.to(DEV)], torch.zeros(B + 1, 5, 2, device=DEV)),
                 lambda: hip_ops.image_sample([m.to(DEV)[0]], torch.zeros(B, 5, 2, device=DEV)),
                 lambda: hip_ops.image_sample([m.to(DEV)], torch.zeros(B, 5, 2, device=DEV), padding_mode="reflection"),
                 lambda: hip_ops.image_sample([m.to(DEV)], torch.zeros(B, 5, 2, device=DEV), global_features=torch.zeros(B + 1, 2, device=DEV)),
                 lambda: hip_ops.image_sample([m.to(DEV)], torch.zeros(B, 5, 2, device=DEV), append=torch.zeros(B, 4, 3, device=DEV)),
                 lambda: hip_ops.image_sample([m], torch.zeros(B, 5, 2, device=DEV))):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------------------- workspace
def test_a_workspace_one_byte_short_is_refused():
    from deftet_amd import _lib
    lib = _lib.load()
    B, N, H, W, C = 2, 100, 5, 4, 3
    uv = ref.interior_uv(B, N, H, W, False, rng(1)).to(DEV)
    n_cells = (H + 1) * (W + 1)
    perm, seg = torch.empty(B * N, device=DEV, dtype=torch.int32), torch.empty(B * n_cells + 1, device=DEV, dtype=torch.int32)
    ws_w = torch.empty(4, B * N, device=DEV)
    gout, gmap = torch.randn(B, C, N, device=DEV), torch.empty(B, C, H, W, device=DEV)
    need = lib.deftet_image_sample_workspace_bytes(B, N, H, W)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    st = _lib.current_stream(uv.device)
    for nbytes, rc_want in ((need - 1, -1), (need, 0)):
        rc = lib.deftet_image_cells_f32(_lib.ptr(uv), _lib.ptr(perm), _lib.ptr(seg), _lib.ptr(ws_w), B, N, H, W, 0, 0, _lib.ptr(ws), nbytes, st)
        assert rc == rc_want and (rc == 0 or b"workspace" in lib.deftet_last_error())
    for nbytes, rc_want in ((need - 1, -1), (need, 0)):
        rc = lib.deftet_image_sample_bwd_map_f32(_lib.ptr(gout), _lib.ptr(perm), _lib.ptr(seg), _lib.ptr(ws_w), _lib.ptr(gmap), B, C, H, W, N, 0,
                                                 C, _lib.ptr(ws), nbytes, st)
        assert rc == rc_want and (rc == 0 or b"workspace" in lib.deftet_last_error())
    torch.cuda.synchronize()
    m = torch.randn(B, C, H, W, generator=rng(2)).double().requires_grad_(True)
    ref.sample_map(m, uv.cpu().double()).backward(gout.cpu().double())
    check_close("is.workspace.grad_map", gmap, m.grad, BOUND)
