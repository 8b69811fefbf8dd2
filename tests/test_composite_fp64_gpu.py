"""The fused composite (k_pix_composite, k_pix_composite_bwd of csrc/raster.hip; DESIGN.md "Fused rasterize-and-composite", "What is
pinned") against fp64 across its windows of 64 ranked slots (tests/composite_cases.py; test_composite_ref_cpu.py is the CPU half and
says where K comes from and that the bounds can fail).  Per entry, with u = 2^-24 and K = composite_cases.K:

    layer gradient   K u n M + n 2^-126 S          forward output   K u (n + 1) M + (n + 1) 2^-126 S

n the pixel's used slots and M the value's own expression in absolute values (composite_ref.exact); carried to gfeat and gxy through
the fp64 face reduction in absolute values, plus the face-reduction bound of tests/raster_bwd_ref.py (composite_ref.face_bounds).

a backward   deftet_sparse_render_composite_bwd_f32 on the face lists of every case, gxy and gfeat pre-filled with NaN: within bound
             of fp64 autograd on every face of every pixel without a NaN; exactly zero on faces without a hit and on the opacity of
             slots outside the clamp; two runs bit-equal; shape 1 of the B = 2 case bit-equal to the same shape run alone (the
             layer-gradient workspace still holds shape 0's longer lists).
b forward    the same stacks with face depths that force the lists, through deftet_sparse_render_composite (NEAREST): per pixel the
             stack as a set in the first min(n, knum) slots and -1 behind; colour, coverage, depth within bound of fp64 on the
             returned order; autograd bit-equal to the by-construction call on the returned face; FIRST bit-equal to NEAREST where
             no pixel saturates; stacks of 320 under knum = 300 keep their 300 nearest.
c nan        one NaN opacity in one pixel: the NaN pattern of the outputs and of both gradients is the reference's, every other
             pixel's faces are within bound.

Worst error / bound of an MI355X run: profiles/composite_tolerances.jsonl.
"""
import functools

import numpy as np
import pytest
import torch

from tests import composite_cases as C
from tests import composite_ref as CR
from tests.tol import check_bound

pytestmark = pytest.mark.gpu

NEAREST, FIRST = 0, 1


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.array(x)).to(dev)                # (a copy: the cases' arrays are read-only)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def backward(dev, sp, shapes, face, g):
    """deftet_sparse_render_composite_bwd_f32 on the shapes as one batch, with `face` [B,P,knum] int32 and g = (g_colour [B,P,Dc],
    g_coverage [B,P,1], g_depth [B,P,1]) or None each -> (gxy [B,F,3,2], gfeat [B,F,3,D]) as numpy; the outputs are filled with NaN
    before the call (the entry clears them)"""
    from deftet_amd import _lib
    lib = _lib.load()
    B, P, knum = face.shape
    pix, fxy, feat = (np.stack([sh[k] for sh in shapes]) for k in ("pix", "fxy", "feat"))
    F, D = fxy.shape[1], feat.shape[3]
    assert face.dtype == np.int32 and face.min() >= -1 and face.max() < F and pix.shape == (B, P, 2)      # no index is out of range
    assert ((face >= 0) == (np.arange(knum) < (face >= 0).sum(2, keepdims=True))).all()                  # the used slots come first
    tp, txy, tff, tface = (_t(x, dev) for x in (pix, fxy, feat, face))
    gc, gv, gd = (_t(x, dev) for x in g)
    assert all(x is None or x.dtype == torch.float32 for x in (tp, txy, tff, gc, gv, gd))
    gxy = torch.full_like(txy, float("nan"))
    gff = torch.full_like(tff, float("nan"))
    with _lib.on_device(dev):
        ws = _lib.workspace(dev, lib.deftet_sparse_render_composite_bwd_workspace_bytes(B, P, F, D, knum))
        _lib.check(lib.deftet_sparse_render_composite_bwd_f32(_lib.ptr(tp), _lib.ptr(txy), _lib.ptr(tff), _lib.ptr(tface), _lib.ptr(gc), _lib.ptr(gv),
                                                              _lib.ptr(gd), B, P, F, D, knum, C.EPS, sp["depth"], sp["bg"], C.FAR_DEPTH, _lib.ptr(gxy),
                                                              _lib.ptr(gff), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)),
                   "deftet_sparse_render_composite_bwd_f32")
    torch.cuda.synchronize()
    return gxy.cpu().numpy(), gff.cpu().numpy()


def _reference(name, b, face):
    c = C.case(name)
    sp, sh = c["spec"], c["shapes"][b]
    args = (sh["pix"], sh["fxy"], sh["feat"], face, C.shape_grads(c, b), sp["depth"], sp["bg"])
    ex = CR.exact(*args)
    bxy, bfeat, nf, _ = CR.face_bounds(*args[:4], ex)
    return dict(ex=ex, an=CR.analytic(*args), bxy=bxy, bfeat=bfeat, nf=nf, fwd=CR.forward_bounds(ex))


@functools.lru_cache(maxsize=None)
def constructed_reference(name, b):
    """the fp64 values and bounds of a shape on its constructed lists: computed once, shared by the tests, left unchanged"""
    return _reference(name, b, C.case(name)["shapes"][b]["face"])


def reference(name, b, face):
    sh = C.case(name)["shapes"][b]
    return constructed_reference(name, b) if np.array_equal(face, sh["face"]) else _reference(name, b, face)


def hold_backward(tag, name, b, face, gxy, gfeat):
    """one shape's gradients against fp64 autograd, entry by entry; exact zeros where nothing arrives"""
    sp = C.case(name)["spec"]
    ref = reference(name, b, face)
    ex, an = ref["ex"], ref["an"]
    clean = np.isfinite(ref["bfeat"]).all((1, 2)) & np.isfinite(ref["bxy"]).all((1, 2))     # every face but those of a pixel with a NaN
    assert clean.all() or sp["profile"] == "nan"
    assert np.array_equal(np.isnan(gxy), np.isnan(an["gxy"])) and np.array_equal(np.isnan(gfeat), np.isnan(an["gfeat"]))
    check_bound(tag + ", gfeat", gfeat, an["gfeat"], ref["bfeat"], mask=clean[:, None, None])
    check_bound(tag + ", gxy", gxy, an["gxy"], ref["bxy"], mask=clean[:, None, None])
    none = ref["nf"] == 0
    assert none.sum() >= 3 and not gxy[none].any() and not gfeat[none].any()
    masked = face[ex["used"] & ~ex["passes"] & np.isfinite(ex["cov"])[:, None]]             # one hit each: the opacity gradient is this slot's
    assert not gfeat[masked][:, :, 1 if sp["depth"] else 0].any()
    return int(masked.size)


def batch(name):
    c = C.case(name)
    return c, c["spec"], c["shapes"], np.stack([sh["face"] for sh in c["shapes"]])


# ------------------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("name", [n for n in C.CASE_IDS if "nan" not in n])
def test_backward_by_construction(cuda, name):
    c, sp, shapes, face = batch(name)
    gxy, gfeat = backward(cuda, sp, shapes, face, c["g"])
    masked = 0
    for b in range(sp["B"]):
        masked += hold_backward("composite pin, %s[%d], backward" % (name, b), name, b, face[b], gxy[b], gfeat[b])
    assert (masked > 500) == (sp["profile"] == "clamp")
    gxy2, gfeat2 = backward(cuda, sp, shapes, face, c["g"])                                 # one hit per face (41 for the shared one): fixed order
    assert np.array_equal(_bits(gxy), _bits(gxy2)) and np.array_equal(_bits(gfeat), _bits(gfeat2))
    if sp["B"] > 1:
        g1 = tuple(None if x is None else x[1:] for x in c["g"])
        axy, afeat = backward(cuda, sp, shapes[1:], face[1:], g1)
        assert np.array_equal(_bits(axy[0]), _bits(gxy[1])) and np.array_equal(_bits(afeat[0]), _bits(gfeat[1]))
        assert not np.array_equal(gfeat[0], gfeat[1])


# ------------------------------------------------------------------------------------------------------------------------- b
def forward(dev, sp, shapes, g, policy):
    """deftet_sparse_render_composite on the stacks with their forcing depths -> the outputs, face, and the autograd gradients"""
    from deftet_amd.render import deftet_sparse_render_composite
    pix, fz, fxy, feat = (np.stack([sh[k] for sh in shapes]) for k in ("pix", "fz", "fxy", "feat"))
    rngs = np.tile(np.array([-1000.0, 0.0], np.float32), pix.shape[:2] + (1,))
    tp, tr, tz = (_t(x, dev) for x in (pix, rngs, fz))
    txy, tff = _t(fxy, dev).requires_grad_(True), _t(feat, dev).requires_grad_(True)
    c, v, d, face = deftet_sparse_render_composite(tp, tr, tz, txy, tff, knum=sp["knum"], eps=C.EPS, policy=policy, depth=bool(sp["depth"]),
                                                   background=sp["bg"], far_depth=C.FAR_DEPTH)
    grads = None
    if g is not None:
        loss = sum((out * _t(x, dev)).sum() for out, x in zip((c, v, d), g) if x is not None)
        grads = tuple(x.cpu().numpy() for x in torch.autograd.grad(loss, (txy, tff)))
    out = tuple(None if x is None else x.detach().cpu().numpy() for x in (c, v, d))
    return out, face.cpu().numpy(), grads


@pytest.mark.parametrize("name", [n for n in C.CASE_IDS if "nan" not in n])
def test_forward_from_a_scene_that_forces_the_lists(cuda, name):
    c, sp, shapes, _ = batch(name)
    (col, cov, dep), face, (gxy, gfeat) = forward(cuda, sp, shapes, c["g"], NEAREST)
    assert face.dtype == np.int32
    for b, sh in enumerate(shapes):
        stack, knum = sh["stack"], sp["knum"]
        want = np.sort(np.where(np.arange(stack.shape[1]) < knum, stack, -1), 1)[:, ::-1][:, :knum]     # the knum nearest: built nearest first
        assert np.array_equal(np.sort(face[b], 1)[:, ::-1], want)                                       # the stack as a set
        assert ((face[b] >= 0) == (np.arange(knum) < sh["n"][:, None])).all()                           # in the first n slots, -1 behind
        if not sp["shared"]:
            assert np.array_equal(face[b], sh["face"])                                                  # (and in the built order)
        ref = reference(name, b, face[b])
        an, fb = ref["an"], ref["fwd"]
        tag = "composite pin, %s[%d], forward" % (name, b)
        check_bound(tag + ", colour", col[b], an["colour"], fb[0])
        check_bound(tag + ", coverage", cov[b, :, 0], an["cov"], fb[1])
        if sp["depth"]:
            check_bound(tag + ", depth", dep[b, :, 0], an["dep"], fb[2])
        else:
            assert dep is None
        hold_backward("composite pin, %s[%d], autograd" % (name, b), name, b, face[b], gxy[b], gfeat[b])
    bxy, bfeat = backward(cuda, sp, shapes, face, c["g"])
    assert np.array_equal(_bits(bxy), _bits(gxy)) and np.array_equal(_bits(bfeat), _bits(gfeat))
    if sp["stack"]:
        assert all((sh["stack"][:, knum:] >= 0).all() for sh in shapes)                                 # 20 more faces cover every pixel
        return
    out1, face1, _ = forward(cuda, sp, shapes, None, FIRST)                                             # nothing saturates: the same bits
    assert np.array_equal(face1, face)
    for x, y in zip(out1, (col, cov, dep)):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------------------------------- c
def test_nan_opacity_stays_in_its_pixel(cuda):
    name = "k300-P41-nan"
    c, sp, shapes, face = batch(name)
    ref = constructed_reference(name, 0)
    an = ref["an"]
    bad = np.isnan(an["cov"])
    assert bad.sum() == 1
    gxy, gfeat = backward(cuda, sp, shapes, face, c["g"])
    hold_backward("composite pin, %s[0], backward" % name, name, 0, face[0], gxy[0], gfeat[0])
    touched = np.zeros(gxy.shape[1], bool)
    touched[face[0][bad][face[0][bad] >= 0]] = True
    assert np.isnan(gxy[0][touched]).all() and np.isfinite(gxy[0][~touched]).all() and np.isfinite(gfeat[0][~touched]).all()
    (col, cov, dep), face1, (axy, afeat) = forward(cuda, sp, shapes, c["g"], NEAREST)
    assert np.array_equal(face1, face)
    fb = ref["fwd"]
    for nm, got, want, bound in (("colour", col[0], an["colour"], fb[0]), ("coverage", cov[0, :, 0], an["cov"], fb[1]), ("depth", dep[0, :, 0], an["dep"], fb[2])):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[bad]).all()
        check_bound("composite pin, %s[0], forward, %s" % (name, nm), got[~bad], want[~bad], bound[~bad])
    assert np.array_equal(_bits(axy), _bits(gxy)) and np.array_equal(_bits(afeat), _bits(gfeat))
