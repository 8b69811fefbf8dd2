"""GPU tests of the fused rasterize-and-composite operator (deftet_sparse_render_composite): it must give what
alpha_composite(deftet_sparse_render(...)) gives — the same faces in the same order, the same images up to fp32 rounding — with
gradients checked against fp64 autograd of the same composition, at the clamp, for partial output gradients, at BASELINE
configs[4] and with less memory than the layer stack."""
import numpy as np
import pytest
import torch

from deftet_amd import grids

pytestmark = pytest.mark.gpu

NEAREST, FIRST = 0, 1


def projected_grid(res, **kw):
    from oracle import oracle as O
    verts, tets = grids.kuhn_grid(res)
    f3, _, _, _, _ = O.tet_to_face(tets, verts.shape[0], with_boundary=True)
    return grids.project_faces(verts, f3, **kw)


def scene(res, npix, D=4, B=1, scale=0.7, seed=0, lo=0.0, hi=1.0, copies=1):
    """[B,...] numpy inputs: the projected grid (batch b shifted a little; `copies` stacked copies of it, each a little further
    away, so that pixels collect more than one wave of hits), features uniform in [lo, hi)"""
    fz, fxy, _ = projected_grid(res)
    fz = np.concatenate([fz - np.float32(0.01 * k) for k in range(copies)], 1)
    fxy = np.concatenate([fxy + np.float32(0.37 * k) for k in range(copies)], 1)
    pix, rngs = grids.pixel_grid(npix)
    pix = pix * scale
    F = fz.shape[1]
    rng = np.random.default_rng(seed)
    fzs, fxys, ffs = [], [], []
    for b in range(B):
        fzs.append(fz[0])
        fxys.append(fxy[0] + np.float32(13.0 * b))
        ffs.append((lo + (hi - lo) * rng.random((F, 3, D))).astype(np.float32))
    return (np.repeat(pix, B, 0), np.repeat(rngs, B, 0), np.stack(fzs), np.stack(fxys).astype(np.float32), np.stack(ffs))


def to_dev(dev, *xs, grad=False):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad) for x in xs]


def unfused(pix, rngs, fz, xy, ff, knum, policy, depth, background=1.0, far_depth=-6.0):
    from deftet_amd.render import alpha_composite, deftet_sparse_render
    layers, face64 = deftet_sparse_render(pix, rngs, fz, xy, ff, knum=knum, policy=policy)
    if depth:
        c, v, d = alpha_composite(layers[..., 1:], layers[..., :1], background, far_depth)
    else:
        c, v, d = alpha_composite(layers, None, background, far_depth)
    return c, v, d, face64


def fused(pix, rngs, fz, xy, ff, knum, policy, depth, **kw):
    from deftet_amd.render import deftet_sparse_render_composite
    return deftet_sparse_render_composite(pix, rngs, fz, xy, ff, knum=knum, policy=policy, depth=depth, **kw)


def maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("policy", [NEAREST, FIRST])
@pytest.mark.parametrize("knum", [4, 48, 300])
def test_equals_the_composition(cuda, knum, policy, depth):
    for res, npix, D, B, copies in ((6, 24, 4, 1, 1), (8, 40, 3, 2, 1), (8, 40, 6, 1, 1), (6, 24, 6, 2, 1), (8, 24, 4, 1, 6)):
        pix, rngs, fz, xy, ff = to_dev(cuda, *scene(res, npix, D, B, seed=res + D + B, copies=copies))
        with torch.no_grad():
            c0, v0, d0, face64 = unfused(pix, rngs, fz, xy, ff, knum, policy, depth)
            c1, v1, d1, face = fused(pix, rngs, fz, xy, ff, knum, policy, depth)
        assert face.dtype == torch.int32 and face.shape == face64.shape
        assert torch.equal(face.long(), face64), (res, npix, D, B)
        assert c1.shape == c0.shape and v1.shape == v0.shape
        assert maxdiff(c1, c0) <= 1e-5 and maxdiff(v1, v0) <= 1e-5, (res, npix, D, B)
        if depth:
            assert maxdiff(d1, d0) <= 1e-5
        else:
            assert d1 is None
        if knum == 4:
            assert (face[..., -1] >= 0).any()                   # saturating
        if knum == 300 and copies > 1:
            assert (face >= 0).sum(-1).max().item() > 128                # three windows of 64 ranked slots


# ---------------------------------------------------------------------------------------------------------------- 2
def test_backward_matches_fp64_composition(cuda, oracle):
    from deftet_amd.render import alpha_composite
    from tests.tol import check_close
    pix, rngs, fz, xy, ff = scene(6, 24, D=5, scale=0.6, lo=0.05, hi=0.95)      # opacities away from the clamp
    tp, tr, tz = to_dev(cuda, pix, rngs, fz)
    txy, tff = to_dev(cuda, xy, ff, grad=True)
    c, v, d, face = fused(tp, tr, tz, txy, tff, 48, NEAREST, True)
    g = torch.Generator(device=cuda).manual_seed(0)
    R1 = torch.rand(c.shape, device=cuda, generator=g)
    R2 = torch.rand(v.shape, device=cuda, generator=g)
    R3 = torch.rand(d.shape, device=cuda, generator=g)
    ((c * R1).sum() + (v * R2).sum() + (d * R3).sum()).backward()
    xy64 = torch.from_numpy(xy).double().requires_grad_(True)
    ff64 = torch.from_numpy(ff).double().requires_grad_(True)
    layers = oracle.sparse_render_torch(torch.from_numpy(pix).double(), xy64, ff64, face.long().cpu())
    c64, v64, d64 = alpha_composite(layers[..., 1:], layers[..., :1])
    for got, want in ((c, c64), (v, v64), (d, d64)):
        assert (got.detach().cpu().double() - want.detach()).abs().max().item() <= 1e-5
    ((c64 * R1.cpu().double()).sum() + (v64 * R2.cpu().double()).sum() + (d64 * R3.cpu().double()).sum()).backward()
    for nm, got, want in (("xy", txy.grad, xy64.grad), ("feat", tff.grad, ff64.grad)):
        assert want.abs().max().item() > 0
        check_close("fused composite grad_%s, res6 24x24 k48 depth vs fp64 autograd" % nm, got, want, 6e-7, elem_rel=1.5e-4)
    hit = torch.zeros(xy.shape[1], dtype=torch.bool)
    f = face.long().cpu()
    hit[f[f >= 0]] = True
    assert (~hit).any()
    assert (txy.grad.cpu()[0][~hit] == 0).all() and (tff.grad.cpu()[0][~hit] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_opacity_at_the_clamp(cuda):
    pix, rngs, fz, xy, ff = scene(6, 24, D=4, scale=0.6, seed=3)
    F = ff.shape[1]
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 4, F)                           # 0: random, 1: opacity exactly 1.0, 2: exactly 0, 3: 1.5 (clamps to 1)
    ff[0, kind == 1, :, 0] = 1.0
    ff[0, kind == 2, :, 0] = 0.0
    ff[0, kind == 3, :, 0] = 1.5
    tp, tr, tz = to_dev(cuda, pix, rngs, fz)
    g = torch.Generator(device=cuda).manual_seed(2)
    grads = []
    for fn in (unfused, fused):
        txy, tff = to_dev(cuda, xy, ff, grad=True)
        c, v, _, face = fn(tp, tr, tz, txy, tff, 48, NEAREST, False)
        if not grads:
            R1 = torch.rand(c.shape, device=cuda, generator=g)
            R2 = torch.rand(v.shape, device=cuda, generator=g)
        ((c * R1).sum() + (v * R2).sum()).backward()
        grads.append((txy.grad, tff.grad, face.long()))
    for k in range(2):
        want, got = grads[0][k], grads[1][k]
        assert torch.isfinite(got).all()
        assert maxdiff(got, want) <= 1e-5 * want.abs().max().item()
    # Behind a layer whose composited opacity is exactly 1.0f nothing is seen: a face that is only ever hit behind such a layer gets
    # exactly zero gradient.  The layers' opacities are read from the layer-returning operator (same expression, same bits); the
    # occluders used are those interpolated to exactly 1.0f from corners of exactly 1.0 (not the 1.5 faces, which clamp to it).
    from deftet_amd.render import deftet_sparse_render
    txy, tff = to_dev(cuda, xy, ff)
    with torch.no_grad():
        layers, face = deftet_sparse_render(tp, tr, tz, txy, tff, knum=48, policy=NEAREST)
    face, alpha = face[0], layers[0, ..., 0]
    assert torch.equal(face, grads[1][2][0])
    exact = (face >= 0) & (alpha == 1.0)
    assert exact.any()
    K = face.shape[1]
    rank = torch.arange(K, device=cuda)[None].expand_as(face)
    first = torch.where(exact, rank, torch.full_like(rank, K)).min(-1).values
    seen = torch.zeros(F, dtype=torch.bool, device=cuda)
    seen[face[(face >= 0) & (rank <= first[:, None])]] = True
    hit = torch.zeros(F, dtype=torch.bool, device=cuda)
    hit[face[face >= 0]] = True
    behind_only = hit & ~seen
    assert behind_only.any()
    assert (grads[1][1][0][behind_only] == 0).all() and (grads[1][0][0][behind_only] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("which", ["colour", "coverage", "depth", "zero"])
def test_partial_output_gradients(cuda, oracle, which):
    """Only one of the outputs reaches the loss: the other gradients are absent (NULL) in the backward ("zero": the colour
    gradient is present and all zero).  The fused
    gradients agree with the unfused path's up to that path's own fp32 error (both measured against fp64 autograd of the
    composition: with coverage alone, dL/dalpha is a small difference of large terms in the unfused expression)."""
    from deftet_amd.render import alpha_composite
    pix, rngs, fz, xy, ff = scene(6, 24, D=4, scale=0.6, seed=4, lo=0.05, hi=0.95)
    tp, tr, tz = to_dev(cuda, pix, rngs, fz)
    res = []

    def pick(c, v, d):
        return {"colour": c, "coverage": v, "depth": d, "zero": c}[which]
    for fn in (unfused, fused):
        txy, tff = to_dev(cuda, xy, ff, grad=True)
        c, v, d, face = fn(tp, tr, tz, txy, tff, 48, NEAREST, True)
        out = pick(c, v, d)
        w = torch.linspace(0.5, 1.5, out.numel(), device=cuda).reshape(out.shape)
        loss = (out * w).sum() * (0.0 if which == "zero" else 1.0)
        res.append(torch.autograd.grad(loss, (txy, tff)))
    if which == "zero":
        assert all((g == 0).all() for g in res[1])
        return
    xy64 = torch.from_numpy(xy).double().requires_grad_(True)
    ff64 = torch.from_numpy(ff).double().requires_grad_(True)
    layers = oracle.sparse_render_torch(torch.from_numpy(pix).double(), xy64, ff64, face.long().cpu())
    out64 = pick(*alpha_composite(layers[..., 1:], layers[..., :1]))
    w64 = torch.linspace(0.5, 1.5, out64.numel(), dtype=torch.float64).reshape(out64.shape)
    want64 = torch.autograd.grad((out64 * w64).sum(), (xy64, ff64))
    for k in range(2):
        exact = want64[k].to(cuda)
        scale = exact.abs().max().item()
        assert scale > 0
        e_fu = maxdiff(res[1][k], res[0][k]) / scale
        e_f = maxdiff(res[1][k], exact) / scale
        e_u = maxdiff(res[0][k], exact) / scale
        assert e_f <= max(1.5 * e_u, 2e-6), (k, e_f, e_u)
        assert e_fu <= 1e-5 + e_u, (k, e_fu, e_u)


def test_all_output_gradients_absent(cuda):
    """No output gradient at all: the autograd backward returns no gradients without a library call, and the C backward with
    three NULL output gradients writes zero gradients (over buffers filled with NaN beforehand)."""
    from deftet_amd import _lib
    from deftet_amd.render.deftet_sparse_render import _SparseRenderComposite
    pix, rngs, fz, xy, ff = scene(6, 24, D=4, scale=0.6, seed=9)
    tp, tr, tz = to_dev(cuda, pix, rngs, fz)
    txy, tff = to_dev(cuda, xy, ff, grad=True)
    c, v, d, face = _SparseRenderComposite.apply(tp, tr, tz, txy, tff, 48, 1e-8, NEAREST, False, 1.0, -6.0)
    assert d is None
    assert all(g is None for g in c.grad_fn.apply(None, None, None, None))
    lib = _lib.load()
    B, P, K = face.shape
    F, D = xy.shape[1], ff.shape[3]
    gxy = torch.full_like(txy.detach(), float("nan"))
    gff = torch.full_like(tff.detach(), float("nan"))
    ws = _lib.workspace(cuda, lib.deftet_sparse_render_composite_bwd_workspace_bytes(B, P, F, D, K))
    _lib.check(lib.deftet_sparse_render_composite_bwd_f32(_lib.ptr(tp), _lib.ptr(txy), _lib.ptr(tff), _lib.ptr(face), None, None, None,
                                                          B, P, F, D, K, 1e-8, 0, 1.0, -6.0, _lib.ptr(gxy), _lib.ptr(gff), _lib.ptr(ws),
                                                          ws.numel(), _lib.current_stream(cuda)), "composite bwd")
    torch.cuda.synchronize()
    assert (gxy == 0).all() and (gff == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("policy", [NEAREST, FIRST])
def test_baseline_config(cuda, oracle, policy):
    from deftet_amd.render import alpha_composite
    fz, fxy, ff = projected_grid(70)
    pix, rngs = grids.pixel_grid(512)
    tp, tr, tz = to_dev(cuda, pix, rngs, fz)
    g = torch.Generator(device=cuda).manual_seed(1)
    R1 = torch.rand(tp.shape[0], tp.shape[1], 3, device=cuda, generator=g)
    R2 = torch.rand(tp.shape[0], tp.shape[1], 1, device=cuda, generator=g)
    out = {}
    for name, fn in (("unfused", unfused), ("fused", fused)):
        txy, tff = to_dev(cuda, fxy, ff, grad=True)
        c, v, _, face = fn(tp, tr, tz, txy, tff, 64, policy, False)
        gxy, gff = torch.autograd.grad((c * R1).sum() + (v * R2).sum(), (txy, tff))
        out[name] = (c.detach(), v.detach(), face, gxy, gff)
    c0, v0, face64, _, _ = out["unfused"]
    c1, v1, face, gxy, gff = out["fused"]
    assert torch.equal(face.long(), face64)
    assert maxdiff(c1, c0) <= 1e-5 and maxdiff(v1, v0) <= 1e-5
    with torch.no_grad():
        c2, v2, _, _ = fused(tp, tr, tz, *to_dev(cuda, fxy, ff), 64, policy, False)
    assert torch.equal(c2, c1) and torch.equal(v2, v1)                   # bit-reproducible forward
    xy64 = torch.from_numpy(fxy).to(cuda).double().requires_grad_(True)
    ff64 = torch.from_numpy(ff).to(cuda).double().requires_grad_(True)
    layers = oracle.sparse_render_torch(tp.double(), xy64, ff64, face64)
    c64, v64, _ = alpha_composite(layers)
    del layers
    wxy, wff = torch.autograd.grad((c64 * R1.double()).sum() + (v64 * R2.double()).sum(), (xy64, ff64))
    for k, want in ((3, wxy), (4, wff)):
        scale = want.abs().max().item()
        e_unf = maxdiff(out["unfused"][k], want) / scale
        e_fus = maxdiff(out["fused"][k], want) / scale
        assert e_fus <= 1.5 * e_unf + 1e-7, (k, e_fus, e_unf)


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("policy", [NEAREST, FIRST])
def test_baseline_forward_vs_oracle_layers(cuda, oracle, policy, depth):
    """test_baseline_config proves fused == unfused, and both start from the kernel's own faces.  Here the fused forward at
    BASELINE configs[4] is held against the CPU oracle on the 16,384 chosen pixels of tests/raster_scene.py: the same faces in the
    same order, and colour / coverage / depth against alpha_composite evaluated in fp64 on the ORACLE's fp32 layers.  The error
    bound is the unfused path's own error against that value (deftet_sparse_render + alpha_composite in fp32) times 1.5 plus
    1e-7 — the rule test_baseline_config uses for the gradients — and 1e-5 absolute on colour and coverage, which lie in
    [0, 1]; the depth (up to |far_depth| = 6 in magnitude) gets 1e-5 of its largest entry."""
    from deftet_amd.render import alpha_composite
    from tests import raster_scene as RS
    from tests.tol import check_close
    pix, rngs, fz, fxy, ff = RS.scene("baseline")
    sel = RS.selection("baseline").sel
    wfeat, wface, _ = RS.oracle_rows("baseline", 64, policy)
    assert len(sel) >= 16384 and (wface[0, :, -1] >= 0).mean() > 0.5 and (wface[0, :, 0] < 0).any()      # full rows and empty ones
    layers = torch.from_numpy(wfeat).double()
    want = alpha_composite(layers[..., 1:], layers[..., :1]) if depth else alpha_composite(layers)
    rows = torch.from_numpy(sel).to(cuda)
    t = to_dev(cuda, pix, rngs, fz, fxy, ff)
    with torch.no_grad():
        c0, v0, d0, _ = unfused(*t, 64, policy, depth)
        c1, v1, d1, face = fused(*t, 64, policy, depth)
    assert np.array_equal(face[0, rows].cpu().numpy(), wface[0])
    tag = "configs[4] 16 k chosen pixels k64 policy %d depth %d vs fp64 composite of the oracle's layers" % (policy, int(depth))
    for nm, w64, unf, fus in (("colour", want[0], c0, c1), ("coverage", want[1], v0, v1)) + ((("depth", want[2], d0, d1),) if depth else ()):
        scale = w64.abs().max().item()
        assert 0.5 < scale <= (1.0 if nm != "depth" else 6.0) + 1e-6
        bound = 1e-5 / scale if nm != "depth" else 1e-5                        # check_close measures relative to the largest entry
        e_unf = check_close("unfused %s, %s" % (nm, tag), unf[:, rows], w64, bound)[0] * scale
        e_fus = check_close("fused %s, %s" % (nm, tag), fus[:, rows], w64, bound)[0] * scale
        print("%s: fused %.3g, unfused %.3g (absolute, policy %d depth %d)" % (nm, e_fus, e_unf, policy, int(depth)))
        assert e_fus <= 1.5 * e_unf + 1e-7, (nm, e_fus, e_unf)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_memory_without_the_layer_stack(cuda):
    fz, fxy, ff = projected_grid(70)
    pix, rngs = grids.pixel_grid(512)
    tp, tr, tz = to_dev(cuda, pix, rngs, fz)
    txy, tff = to_dev(cuda, fxy, ff, grad=True)
    knum, D = 64, ff.shape[-1]
    P = tp.shape[1]
    stack = P * knum * D * 4
    for _ in range(2):                                                   # warm-up: the cached workspace
        c, v, _, face = fused(tp, tr, tz, txy, tff, knum, NEAREST, False)
        (c.sum() + v.sum()).backward()
        del c, v, face
    torch.cuda.synchronize()
    saved = []

    def pack(t):
        saved.append(t.numel())
        return t
    before = torch.cuda.memory_allocated(cuda)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        c, v, _, face = fused(tp, tr, tz, txy, tff, knum, NEAREST, False)
    torch.cuda.synchronize()
    rise = torch.cuda.memory_allocated(cuda) - before
    assert rise < stack, (rise, stack)
    assert saved and max(saved) < P * knum * D, saved
    del c, v, face
    # the unfused path keeps at least the layer stack
    before = torch.cuda.memory_allocated(cuda)
    o = unfused(tp, tr, tz, txy, tff, knum, NEAREST, False)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(cuda) - before >= stack
    del o


# ---------------------------------------------------------------------------------------------------------------- 7
def test_edge_cases(cuda):
    pix, rngs, fz, xy, ff = scene(6, 24, D=4, scale=0.6, seed=7)
    # F = 0: every pixel is background
    tp, tr = to_dev(cuda, pix, rngs)
    ez, exy, eff = to_dev(cuda, fz[:, :0], xy[:, :0], ff[:, :0])
    with torch.no_grad():
        c0, v0, _, f0 = unfused(tp, tr, ez, exy, eff, 8, NEAREST, False)
        c1, v1, _, f1 = fused(tp, tr, ez, exy, eff, 8, NEAREST, False)
    assert torch.equal(f1.long(), f0) and (c1 == 1.0).all() and maxdiff(v1, v0) <= 1e-12
    # P = 0
    ep, er = to_dev(cuda, pix[:, :0], rngs[:, :0])
    tz, txy, tff = to_dev(cuda, fz, xy, ff)
    with torch.no_grad():
        c1, v1, _, f1 = fused(ep, er, tz, txy, tff, 8, NEAREST, False)
    assert c1.shape == (1, 0, 3) and v1.shape == (1, 0, 1) and f1.shape == (1, 0, 8)
    # pixels no face covers: background colour, coverage as unfused (knum * 1e-10)
    far = pix + np.float32(1e5)
    tp2 = to_dev(cuda, far)[0]
    with torch.no_grad():
        c0, v0, _, _ = unfused(tp2, tr, tz, txy, tff, 8, NEAREST, False)
        c1, v1, _, f1 = fused(tp2, tr, tz, txy, tff, 8, NEAREST, False)
    assert (f1 == -1).all() and (c1 == 1.0).all() and maxdiff(v1, v0) <= 1e-12 and v1.max().item() > 0
    # NaN features: the same NaN mask as the unfused path
    ffn = ff.copy()
    ffn[0, ::7, 1, 2] = np.nan
    ffn[0, ::11, 0, 0] = np.nan
    tffn = to_dev(cuda, ffn)[0]
    with torch.no_grad():
        c0, v0, _, _ = unfused(tp, tr, tz, txy, tffn, 48, NEAREST, False)
        c1, v1, _, _ = fused(tp, tr, tz, txy, tffn, 48, NEAREST, False)
    assert torch.isnan(c0).any() and torch.isnan(v0).any()
    assert torch.equal(torch.isnan(c1), torch.isnan(c0)) and torch.equal(torch.isnan(v1), torch.isnan(v0))
    ok = ~torch.isnan(c0)
    assert maxdiff(c1[ok], c0[ok]) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("depth", [False, True])
def test_render_mesh_color_fused(cuda, depth):
    from oracle import oracle as O
    from deftet_amd.render import render_mesh_color
    verts, tets = grids.kuhn_grid(6)
    f3, _, _, _, _ = O.tet_to_face(tets, verts.shape[0], with_boundary=True)
    p = (np.asarray(verts, np.float64) - 0.5) * 2.5
    a = 0.35
    p = p @ np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]).T
    pc = p - np.array([0, 0, 4.0])
    p2 = pc[:, :2] / (-pc[:, 2:3]) * (1111.0 / 800.0 * 2.0) * 1000.0
    pix, rngs = grids.pixel_grid(24)
    pix = pix * 0.6
    feat = np.random.default_rng(8).standard_normal((1, len(verts), 5)).astype(np.float32)
    tp, tr = to_dev(cuda, pix, rngs)
    faces = torch.from_numpy(np.asarray(f3, np.int64)).to(cuda)
    res = []
    for fz in (False, True):
        p3, p2d, tf = to_dev(cuda, pc[None].astype(np.float32), p2[None].astype(np.float32), feat, grad=True)
        c, v, d = render_mesh_color(tp, tr, p3, p2d, tf, faces, depth=depth, knum=48, fused=fz)
        loss = (c * torch.linspace(0, 1, c.numel(), device=cuda).reshape(c.shape)).sum() + v.sum() + (d.sum() if depth else 0.0)
        loss.backward()
        res.append((c.detach(), v.detach(), d.detach() if depth else None, p2d.grad, tf.grad))
    for k, (want, got) in enumerate(zip(res[0], res[1])):
        if want is None:
            assert got is None
            continue
        scale = max(want.abs().max().item(), 1.0) if k < 3 else want.abs().max().item()
        assert maxdiff(got, want) <= 1e-5 * scale, k
