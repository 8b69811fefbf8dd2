"""GPU tests of per-vertex field sampling at query points (tet_field_sample.hip): bit for bit against the fp32
restatements of tests/tet_field_ref.py on the library's own location, the position and point gradients against the existing
backward fed the restated grad_w, all of it within the standing 1e-5 max-norm bound of the fp64 chain, the reduction's edge
cases, determinism, accumulate, the bad-index rule, the no-grad mode, the module routes and the argument errors."""
import functools

import numpy as np
import pytest
import torch

from deftet_amd import grids
from tests import tet_field_ref as ref
from tests.tol import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5


def bits(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def host(a):
    return a.detach().cpu().numpy()


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def csr_of(R, B, per_shape):
    from deftet_amd import hip_ops
    pos, tets = ref.mesh(R, B, per_shape)
    return hip_ops.tet_vertex_csr(gpu(tets), pos.shape[1])


def run(R, B, C, Q, per_shape=False, pts=None, csr="mesh", fill=0.0):
    """forward + backward of the operator on the shared inputs: a dict of the inputs (numpy) and every output and gradient"""
    from deftet_amd import hip_ops
    pos, tets = ref.mesh(R, B, per_shape)
    V = pos.shape[1]
    pts = grids.random_queries(B, Q) if pts is None else pts
    Q = pts.shape[1]
    field, gout = ref.field_of(B, V, C), ref.gout_of(B, Q, C)
    f, p, x = gpu(field, True), gpu(pos, True), gpu(pts, True)
    out, cond, bary = hip_ops.tet_field_sample(f, p, gpu(tets), x, csr=csr_of(R, B, per_shape) if csr == "mesh" else csr, fill=fill,
                                               return_index=True)
    out.backward(gpu(gout))
    return dict(pos=pos, tets=tets, pts=pts, field=field, gout=gout, V=V, T=tets.shape[-2], out=out.detach(), cond=cond, bary=bary,
                gfield=f.grad, gpos=p.grad, gpts=x.grad)


# ---------------------------------------------------------------------------- 1. bit for bit against the fp32 restatement
@pytest.mark.parametrize("per_shape", [False, True], ids=["shared", "per_shape"])
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("C", [1, 3, 4, 5, 33])
@pytest.mark.parametrize("B", [1, 3])
def test_bit_identical_to_the_fp32_restatement(B, C, Q, per_shape):
    from deftet_amd import hip_ops
    R = 6 if Q == 1000 else 4
    r = run(R, B, C, Q, per_shape)
    cond, bary = host(r["cond"]), host(r["bary"])
    assert r["out"].shape == (B, Q, C) and cond.shape == (B, Q, 1) and bary.shape == (B, Q, 4)
    if Q == 1000:
        assert 0.05 < (cond < 0).mean() < 0.25
    direct = hip_ops.point_in_tet_indexed(gpu(r["pos"]), gpu(r["tets"]), gpu(r["pts"]), want_bary=True)
    assert same_bits(cond, direct[0]) and same_bits(bary, direct[1])
    assert same_bits(r["out"], ref.values(r["field"], r["tets"], cond, bary))
    gw = hip_ops.tet_field_sample_bwd_w(gpu(r["field"]), gpu(r["tets"]), r["cond"], gpu(r["gout"]))
    assert same_bits(gw, ref.grad_w(r["field"], r["tets"], cond, r["gout"]))
    assert same_bits(r["gfield"], ref.grad_field(r["gout"], cond, bary, r["tets"], r["V"]))
    # the raw forward on the same location, and a fill other than 0
    assert same_bits(hip_ops.tet_field_sample_fwd(gpu(r["field"]), gpu(r["tets"]), r["cond"], r["bary"], fill=-2.5),
                     ref.values(r["field"], r["tets"], cond, bary, fill=-2.5))


# ---------------------------------------------------------------------------- 2. the gradients the existing backward carries on
def existing_backward(r, R, B, per_shape, gw):
    """point_in_tet_indexed_bwd_to_vertices on the run's inputs and a given grad_w, with hit records of the same query when the
    backward reads them for this size (the records of any forward of the same query serve)"""
    from deftet_amd import hip_ops
    pos, tets, pts = gpu(r["pos"]), gpu(r["tets"]), gpu(r["pts"])
    hits = None
    if hip_ops.bwd_uses_records(r["T"], pts.shape[1]):
        cond, _bary, hits = hip_ops.point_in_tet_indexed(pos, tets, pts, want_bary=True, want_hits=True)
        assert same_bits(cond, r["cond"])
    return hip_ops.point_in_tet_indexed_bwd_to_vertices(pos, tets, pts, r["cond"], gpu(gw), csr_of(R, B, per_shape), want_grad_pts=True, hits=hits)


@pytest.mark.parametrize("per_shape", [False, True], ids=["shared", "per_shape"])
@pytest.mark.parametrize("R,Q", [(4, 1), (4, 65), (4, 96), (6, 300)])
@pytest.mark.parametrize("C", [1, 4, 33])
@pytest.mark.parametrize("B", [1, 3])
def test_position_and_point_gradients_are_the_existing_backward_on_the_restated_grad_w(B, C, R, Q, per_shape):
    """at most 2 queries per tet, where the existing backward reads the forward's hit records and adds in one order (DESIGN.md §4:
    beyond that its per-tet lists add in arrival order, and no bits can be asked of it)"""
    from deftet_amd import hip_ops
    r = run(R, B, C, Q, per_shape)
    assert hip_ops.bwd_uses_records(r["T"], Q)
    gpos, gpts = existing_backward(r, R, B, per_shape, ref.grad_w(r["field"], r["tets"], host(r["cond"]), r["gout"]))
    assert same_bits(r["gpos"], gpos) and same_bits(r["gpts"], gpts)
    assert Q == 1 or (bits(r["gpos"]).any() and bits(r["gpts"]).any())


# ---------------------------------------------------------------------------- 3. against the fp64 chain
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_values_and_all_three_gradients_match_the_fp64_chain(B, C):
    R, Q = 6, 1000
    r = run(R, B, C, Q)
    f64, p64, x64 = (torch.from_numpy(r[k]).double().requires_grad_(True) for k in ("field", "pos", "pts"))
    want = ref.chain64(f64, p64, x64, r["tets"], host(r["cond"]))
    want.backward(torch.from_numpy(r["gout"]).double())
    name = "tfs.R%d.B%d.C%d.Q%d." % (R, B, C, Q)
    check_close(name + "values", r["out"], want, BOUND)
    check_close(name + "grad_field", r["gfield"], f64.grad, BOUND)
    check_close(name + "grad_pos", r["gpos"], p64.grad, BOUND)
    check_close(name + "grad_pts", r["gpts"], x64.grad, BOUND)


# ---------------------------------------------------------------------------- 4. the reduction's edges
def test_every_query_misses():
    from deftet_amd import hip_ops
    R, B, C, Q = 4, 3, 4, 300
    pts = grids.random_queries(B, Q) + np.float32(3.0)                 # all of them far outside the grid
    junk = torch.full((B, ref.mesh(R, B)[0].shape[1], 3), float("nan"), device=DEV)     # freed: the gradient on pos takes its place,
    del junk                                                                            # and a store left out would show as a NaN
    r = run(R, B, C, Q, pts=pts, fill=1.5)
    assert (host(r["cond"]) == -1).all() and not bits(r["bary"]).any()
    assert same_bits(r["out"], np.full((B, Q, C), 1.5, np.float32))
    assert r["gfield"].shape == (B, r["V"], C) and not bits(r["gfield"]).any()
    assert r["gpos"].shape == (B, r["V"], 3) and not bits(r["gpos"]).any() and not bits(r["gpts"]).any()
    poisoned = torch.full((B, r["V"], C), float("nan"), device=DEV)
    got = hip_ops.tet_field_sample_bwd_field(gpu(r["gout"]), r["cond"], r["bary"], csr_of(R, B, False), r["V"], r["T"], out=poisoned)
    assert got is poisoned and not bits(poisoned).any()
    poisoned = torch.full((B, Q, 4), float("nan"), device=DEV)
    del poisoned
    assert not bits(hip_ops.tet_field_sample_bwd_w(gpu(r["field"]), gpu(r["tets"]), r["cond"], gpu(r["gout"]))).any()


def test_five_thousand_queries_inside_one_tet():
    R, B, C, Q = 4, 1, 4, 5000
    pos, tets = ref.mesh(R, B)
    corners = pos[0][tets[21]].astype(np.float64)                      # [4,3]
    w = np.random.default_rng(5).dirichlet(np.ones(4), Q)
    pts = (w @ corners).astype(np.float32)[None]
    r = run(R, B, C, Q, pts=pts)
    cond = host(r["cond"])
    assert (cond == 21).mean() > 0.99                                  # one long list, four loaded vertices
    assert same_bits(r["out"], ref.values(r["field"], tets, cond, host(r["bary"])))
    want = ref.grad_field(r["gout"], cond, host(r["bary"]), tets, r["V"])
    assert same_bits(r["gfield"], want)
    idle = np.setdiff1d(np.arange(r["V"]), np.unique(tets[np.unique(cond[cond >= 0]).astype(np.int64)]))
    assert len(idle) > 10 and not bits(r["gfield"])[:, idle].any() and np.abs(want[0, tets[21]]).min() > 0


@pytest.mark.parametrize("per_shape", [False, True], ids=["shared", "per_shape"])
def test_twenty_queries_per_tet_takes_the_backward_without_records(per_shape):
    """the dense route of the existing backward.  What this operator adds is checked bit for bit; grad_pos and grad_pts come from
    the existing backward's per-tet lists there, which add in arrival order and are not bit-reproducible, so they
    are held to the standing bound of the fp64 chain instead of to bits"""
    from deftet_amd import hip_ops
    R, B, C = 4, 3, 4
    T = ref.mesh(R, B)[1].shape[-2]
    Q = 20 * T
    assert not hip_ops.bwd_uses_records(T, Q)
    r = run(R, B, C, Q, per_shape)
    cond, bary = host(r["cond"]), host(r["bary"])
    assert same_bits(r["out"], ref.values(r["field"], r["tets"], cond, bary))
    assert same_bits(r["gfield"], ref.grad_field(r["gout"], cond, bary, r["tets"], r["V"]))
    gw = hip_ops.tet_field_sample_bwd_w(gpu(r["field"]), gpu(r["tets"]), r["cond"], gpu(r["gout"]))
    assert same_bits(gw, ref.grad_w(r["field"], r["tets"], cond, r["gout"]))
    p64, x64 = (torch.from_numpy(r[k]).double().requires_grad_(True) for k in ("pos", "pts"))
    ref.chain64(torch.from_numpy(r["field"]).double(), p64, x64, r["tets"], cond).backward(torch.from_numpy(r["gout"]).double())
    check_close("tfs.dense.R4.B3.C4.Q%d.grad_pos" % Q, r["gpos"], p64.grad, BOUND)
    check_close("tfs.dense.R4.B3.C4.Q%d.grad_pts" % Q, r["gpts"], x64.grad, BOUND)


def test_a_tet_that_lists_a_vertex_twice_counts_twice():
    """the raw kernels on a location taken from the clean list: the tets most often hit then name their first vertex twice"""
    from deftet_amd import hip_ops
    R, B, C, Q = 4, 3, 3, 1000
    r = run(R, B, C, Q)
    cond, bary = host(r["cond"]), host(r["bary"])
    busy = np.bincount(cond[cond >= 0].astype(np.int64)).argsort()[-3:]
    tets = r["tets"].copy()
    tets[busy, 2] = tets[busy, 0]
    csr, V, T = hip_ops.tet_vertex_csr(gpu(tets), r["V"]), r["V"], r["T"]
    assert same_bits(hip_ops.tet_field_sample_fwd(gpu(r["field"]), gpu(tets), r["cond"], r["bary"]), ref.values(r["field"], tets, cond, bary))
    assert same_bits(hip_ops.tet_field_sample_bwd_w(gpu(r["field"]), gpu(tets), r["cond"], gpu(r["gout"])),
                     ref.grad_w(r["field"], tets, cond, r["gout"]))
    got = hip_ops.tet_field_sample_bwd_field(gpu(r["gout"]), r["cond"], r["bary"], csr, V, T)
    assert same_bits(got, ref.grad_field(r["gout"], cond, bary, tets, V)) and not same_bits(got, r["gfield"])


# ---------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("R,Q", [(6, 300), (6, 1000)])
def test_two_runs_give_the_same_bits(R, Q):
    """every output and gradient up to 2 queries per tet; beyond, everything this operator computes (the existing backward's
    per-tet lists, which carry grad_pos and grad_pts there, add in arrival order: DESIGN.md §4)"""
    from deftet_amd import hip_ops
    a, b = run(R, 3, 4, Q, True), run(R, 3, 4, Q, True)
    keys = ("out", "cond", "bary", "gfield") + (("gpos", "gpts") if hip_ops.bwd_uses_records(a["T"], Q) else ())
    assert len(keys) == (6 if Q == 300 else 4)
    for k in keys:
        assert same_bits(a[k], b[k]), k


# ---------------------------------------------------------------------------- 6. accumulate
@pytest.mark.parametrize("C", [1, 4, 33])
def test_accumulate_adds_the_fresh_result_to_the_buffer(C):
    from deftet_amd import hip_ops
    R, B, Q = 4, 3, 1000
    r = run(R, B, C, Q)
    base = np.random.default_rng(9).standard_normal((B, r["V"], C)).astype(np.float32)
    acc = gpu(base)
    got = hip_ops.tet_field_sample_bwd_field(gpu(r["gout"]), r["cond"], r["bary"], csr_of(R, B, False), r["V"], r["T"], out=acc, accumulate=True)
    assert got is acc and same_bits(acc, base + host(r["gfield"]))
    assert same_bits(acc, ref.grad_field(r["gout"], host(r["cond"]), host(r["bary"]), r["tets"], r["V"], base=base))


# ---------------------------------------------------------------------------- 7. bad indices
def test_a_vertex_index_past_the_field_gives_nan_rows_and_no_fault():
    from deftet_amd import hip_ops
    R, B, C, Q = 4, 2, 4, 1000
    r = run(R, B, C, Q)
    cond, bary = host(r["cond"]), host(r["bary"])
    busy = np.bincount(cond[cond >= 0].astype(np.int64)).argsort()[-2:]
    tets = r["tets"].copy()
    tets[busy[0], 3], tets[busy[1], 0] = r["V"], -3
    named = np.isin(cond[..., 0], busy)
    assert named.sum() >= 4
    # the raw kernels on the clean location: the rows that name a dirty tet are NaN and flagged, the others keep their bits
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    out = hip_ops.tet_field_sample_fwd(gpu(r["field"]), gpu(tets), r["cond"], r["bary"], bad=bad)
    assert int(bad.item()) == 1 and torch.isnan(out[gpu(named)]).all() and same_bits(out[gpu(~named)], r["out"][gpu(~named)])
    assert same_bits(out, ref.values(r["field"], tets, cond, bary))
    hip_ops.tet_field_sample_fwd(gpu(r["field"]), gpu(r["tets"]), r["cond"], r["bary"], bad=bad.zero_())
    assert int(bad.item()) == 0
    gw = hip_ops.tet_field_sample_bwd_w(gpu(r["field"]), gpu(tets), r["cond"], gpu(r["gout"]))
    assert not bits(gw[gpu(named)]).any() and same_bits(gw, ref.grad_w(r["field"], tets, cond, r["gout"]))
    # the operator itself: whatever the query makes of a tet with a NaN corner, a row that names it is NaN and every other row is
    # finite; check=True raises
    f, p, x = gpu(r["field"], True), gpu(r["pos"]), gpu(r["pts"])
    out, cond2, bary2 = hip_ops.tet_field_sample(f, p, gpu(tets), x, return_index=True)
    named2 = gpu(np.isin(host(cond2)[..., 0], busy))
    assert torch.isnan(out[named2]).all() and torch.isfinite(out[~named2]).all()
    assert same_bits(out, ref.values(r["field"], tets, host(cond2), host(bary2)))
    with pytest.raises(RuntimeError, match="out of range|outside"):
        hip_ops.tet_field_sample(f, p, gpu(tets), x, check=True)
    hip_ops.tet_field_sample(f, p, gpu(r["tets"]), x, check=True)


# ---------------------------------------------------------------------------- 8. no-grad mode and the slow path
def test_no_grad_mode_saves_nothing_and_asks_for_no_csr(monkeypatch):
    from deftet_amd import hip_ops
    R, B, C, Q = 4, 3, 4, 65
    want = run(R, B, C, Q)
    calls, hits = [], []
    real_csr, real_query = hip_ops.tet_vertex_csr, hip_ops.point_in_tet_indexed
    monkeypatch.setattr(hip_ops, "tet_vertex_csr", lambda *a, **k: calls.append(1) or real_csr(*a, **k))
    monkeypatch.setattr(hip_ops, "point_in_tet_indexed", lambda *a, **k: hits.append(k.get("want_hits")) or real_query(*a, **k))
    f, p, x, t = gpu(want["field"], True), gpu(want["pos"], True), gpu(want["pts"], True), gpu(want["tets"])
    with torch.no_grad():
        out = hip_ops.tet_field_sample(f, p, t, x)
    assert not out.requires_grad and out.grad_fn is None and same_bits(out, want["out"]) and not calls and hits == [False]
    out = hip_ops.tet_field_sample(f.detach(), p.detach(), t, x.detach())             # nothing asks for a gradient: the same
    assert not out.requires_grad and not calls and hits == [False, False]
    out = hip_ops.tet_field_sample(f, p.detach(), t, x.detach())                      # the field alone: no hit records either
    out.backward(gpu(want["gout"]))
    assert calls == [1] and hits[-1] is False and same_bits(f.grad, want["gfield"])    # without a CSR the backward builds one
    f.grad = None
    hip_ops.tet_field_sample(f, p, t, x).backward(gpu(want["gout"]))
    assert calls == [1, 1] and hits[-1] is True
    assert same_bits(f.grad, want["gfield"]) and same_bits(p.grad, want["gpos"]) and same_bits(x.grad, want["gpts"])


def test_no_query_returns_empty_tensors_without_a_launch(monkeypatch):
    from deftet_amd import hip_ops
    B, C = 2, 3
    pos, tets = ref.mesh(4, B)
    monkeypatch.setattr(hip_ops, "point_in_tet_indexed", lambda *a, **k: pytest.fail("a launch for no query"))
    out, cond, bary = hip_ops.tet_field_sample(gpu(ref.field_of(B, pos.shape[1], C), True), gpu(pos), gpu(tets),
                                               torch.zeros(B, 0, 3, device=DEV), return_index=True)
    assert out.shape == (B, 0, C) and cond.shape == (B, 0, 1) and bary.shape == (B, 0, 4)


# ---------------------------------------------------------------------------- 9. the module routes and the argument errors
class StubModel:
    """the attributes and methods field_at_points reads of a render model (3_model/deftet.py)"""

    def __init__(self, points, tets):
        g = torch.Generator().manual_seed(5)
        self.coef = 1.25
        self.tfpoint_px3 = (torch.from_numpy(points.copy()) / self.coef).to(DEV)
        self.tfpointmov_px3 = (torch.randn(points.shape, generator=g) * 0.002).to(DEV).requires_grad_(True)
        self.tfpointfeat_pxd = torch.randn(points.shape[0], 4, generator=g).to(DEV).requires_grad_(True)
        self.tftet_tx4 = torch.from_numpy(tets.copy()).to(DEV)

    def get_point(self, with_coef=False):
        p = self.tfpoint_px3 + self.tfpointmov_px3
        return self.coef * p if with_coef else p

    def get_feat(self):
        return self.tfpointfeat_pxd


def processfunc(points, feat):
    return torch.sigmoid(feat[:, :1]), torch.sigmoid(feat[:, 1:4])


def test_module_routes_return_the_bits_of_the_raw_call():
    from deftet_amd import hip_ops, render
    from deftet_amd.layers.DefTet.deftet import DefTet, TetTopology
    R, B, C, Q = 4, 3, 4, 90                                           # (at most 2 queries per tet: every gradient has one order)
    want = run(R, B, C, Q)
    tet_bxfx4 = gpu(want["tets"])[None].expand(B, -1, -1).contiguous()
    for route in ("topology", "module"):
        f, p, x = gpu(want["field"], True), gpu(want["pos"], True), gpu(want["pts"], True)
        if route == "topology":
            out = TetTopology(tet_bxfx4, want["V"]).field_sample(f, p, x)
        else:
            out = DefTet(device=DEV).field_query(p, tet_bxfx4, x, f)
        out.backward(gpu(want["gout"]))
        for got, k in ((out, "out"), (f.grad, "gfield"), (p.grad, "gpos"), (x.grad, "gpts")):
            assert same_bits(got, want[k]), (route, k)
    out, cond, bary = TetTopology(tet_bxfx4, want["V"]).field_sample(gpu(want["field"]), gpu(want["pos"]), gpu(want["pts"]), fill=2.0,
                                                                    return_index=True)
    assert same_bits(cond, want["cond"]) and same_bits(bary, want["bary"]) and (out[cond[..., 0] < 0] == 2.0).all()
    # the render-side model: the features themselves, and what processfunc makes of them
    model = StubModel(want["pos"][0], want["tets"])
    pts = gpu(want["pts"][0])
    for fn in (None, processfunc):
        vals, hit = render.field_at_points(model, pts, fn)
        points, feat = model.get_point(True), model.get_feat()
        field = feat if fn is None else torch.cat(fn(points, feat), 1)
        raw, cond, _ = hip_ops.tet_field_sample(field[None], points[None], model.tftet_tx4, pts[None], return_index=True)
        assert vals.shape == (Q, 4) and hit.dtype == torch.bool and same_bits(vals, raw[0]) and torch.equal(hit, cond[0, :, 0] >= 0)
        assert 0.05 < 1 - hit.float().mean() < 0.6
    gm, gf = torch.autograd.grad(vals.square().sum(), (model.tfpointmov_px3, model.tfpointfeat_pxd))
    assert gm.shape == (want["V"], 3) and gf.shape == (want["V"], 4) and gm.abs().max() > 0 and gf.abs().max() > 0
    kept = model._deftet_tet_topology[1]
    render.field_at_points(model, pts)
    assert model._deftet_tet_topology[1] is kept                       # the same list object: kept
    model.tftet_tx4 = model.tftet_tx4[: want["T"] // 2].clone()        # a new list object (deletetet): rebuilt
    _, fewer = render.field_at_points(model, pts)
    assert model._deftet_tet_topology[1] is not kept and 0 < fewer.sum() < hit.sum()


def test_argument_errors_raise():
    from deftet_amd import hip_ops
    B, C, Q = 2, 3, 7
    pos, tets = ref.mesh(4, B)
    V = pos.shape[1]
    field, pos, tets, pts = gpu(ref.field_of(B, V, C)), gpu(pos), gpu(tets), gpu(grids.random_queries(B, Q))
    f = hip_ops.tet_field_sample
    other = hip_ops.tet_vertex_csr(tets[:10], V)
    per_shape = hip_ops.tet_vertex_csr(tets[None].expand(B, -1, -1).contiguous(), V)
    bad = [lambda: f(field.double(), pos, tets, pts), lambda: f(field, pos.half(), tets, pts), lambda: f(field, pos, tets, pts.double()),
           lambda: f(field, pos, tets.float(), pts),
           lambda: f(field[:, :, 0], pos, tets, pts), lambda: f(field[:, :, :0], pos, tets, pts), lambda: f(field, pos[0], tets, pts),
           lambda: f(field, pos[:, :, :2], tets, pts), lambda: f(field, pos, tets[:, :3], pts), lambda: f(field, pos, tets, pts[0]),
           lambda: f(field, pos, tets, pts[:, :, :2]),
           lambda: f(field[:1], pos, tets, pts), lambda: f(field, pos, tets, pts[:1]), lambda: f(field[:, :-1], pos, tets, pts),
           lambda: f(field, pos, tets[None].expand(B + 1, -1, -1), pts),
           lambda: f(field, pos, tets, pts, csr=other), lambda: f(field, pos, tets, pts, csr=per_shape), lambda: f(field, pos, tets, pts, csr=other[:2]),
           lambda: f(field.cpu(), pos, tets, pts), lambda: f(field, pos, tets.cpu(), pts), lambda: f(field, pos, tets, pts.cpu())]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError, match="tet_field_sample|GPU tensors"):
            fn()
            pytest.fail("case %d did not raise" % k)
    assert f(field, pos, tets, pts).shape == (B, Q, C)
