"""tests/tri_dist_ref.py kept honest, and the CPU half of the fp64 pin of the point-to-triangle backward (operator A9):

* closest_on_triangle reproduces the fp64 point-to-triangle distance the forward is pinned with;
* envelope_gradient is what torch fp64 autograd gives, with the weights held fixed (every class) and with the closest point
  recomputed under autograd as the plane projection (face class);
* oracle.tri_dist_bwd, the transcription the HIP kernels are compared with bit for bit, equals envelope_gradient on the pin
  input (tests/tri_dist_cases.py), where only face-class and vertex-class points carry an incoming gradient.
"""
import numpy as np
import pytest
import torch

from tests import tri_dist_cases as C
from tests import tri_dist_ref as R


@pytest.fixture(scope="module")
def soup():
    rng = np.random.default_rng(3)
    tri = rng.random((200, 1, 3)) * 0.8 + 0.1 + (rng.random((200, 3, 3)) - 0.5) * 0.3
    pts = rng.random((500, 3)) * 1.2 - 0.1
    return tri, pts


def test_closest_on_triangle_reproduces_the_forward_pin(soup):
    from tests.test_surface_ops_gpu import _true_point_triangle_d2
    tri, pts = soup
    P, F = pts.shape[0], tri.shape[0]
    want = _true_point_triangle_d2(pts, tri)                         # [P,F]
    pp = np.repeat(pts, F, axis=0)
    tt = np.tile(tri, (P, 1, 1))
    w, cls = R.closest_on_triangle(pp, tt[:, 0], tt[:, 1], tt[:, 2])
    cl = (w[:, :, None] * tt).sum(1)
    got = ((pp - cl) ** 2).sum(1).reshape(P, F)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.abs(w.sum(1) - 1).max() <= 1e-12 and w.min() >= -1e-12
    # every class occurs, the class says how many weights are non-zero
    assert all((cls == k).sum() > 1000 for k in (R.FACE, R.EDGE, R.VERTEX))
    assert np.array_equal((w != 0).sum(1)[cls == R.VERTEX], np.ones((cls == R.VERTEX).sum()))
    assert ((w != 0).sum(1)[cls == R.EDGE] <= 2).all() and (w[cls == R.FACE] > 0).all()


def test_envelope_gradient_is_the_autograd_gradient(soup):
    tri, pts = soup
    rng = np.random.default_rng(4)
    P, F = 4000, tri.shape[0]
    f = rng.integers(0, F, P)
    p = tri[f].mean(1) + (rng.random((P, 3)) - 0.5) * 0.3           # around the saved face: all three classes
    g = rng.standard_normal(P)
    got = R.envelope_gradient(p, tri, f, g)
    t = tri[f]
    w, cls = R.closest_on_triangle(p, t[:, 0], t[:, 1], t[:, 2])
    assert all((cls == k).sum() > 300 for k in (R.FACE, R.EDGE, R.VERTEX))
    # the weights held fixed
    x = torch.from_numpy(tri).requires_grad_(True)
    cl = (torch.from_numpy(w)[:, :, None] * x[torch.from_numpy(f)]).sum(1)
    (torch.from_numpy(g) * ((torch.from_numpy(p) - cl) ** 2).sum(1)).sum().backward()
    assert np.abs(got - x.grad.numpy()).max() <= 1e-9 * np.abs(got).max()
    # face class: the closest point is the plane projection, differentiated through
    m = cls == R.FACE
    got_face = R.envelope_gradient(p[m], tri, f[m], g[m])
    x = torch.from_numpy(tri).requires_grad_(True)
    tf = x[torch.from_numpy(f[m])]
    n = torch.linalg.cross(tf[:, 1] - tf[:, 0], tf[:, 2] - tf[:, 0])
    n = n / n.norm(dim=1, keepdim=True)
    (torch.from_numpy(g[m]) * ((torch.from_numpy(p[m]) - tf[:, 0]) * n).sum(1) ** 2).sum().backward()
    assert np.abs(got_face - x.grad.numpy()).max() <= 1e-9 * np.abs(got_face).max()
    # saved indices outside [0, F) contribute nothing
    f2 = f.copy()
    f2[::3], f2[1::3] = -1, F
    assert np.array_equal(R.envelope_gradient(p, tri, f2, g), R.envelope_gradient(p[2::3], tri, f[2::3], g[2::3]))


def test_oracle_backward_equals_the_envelope_gradient_on_the_pin(oracle):
    """The bound is the fp32 evaluation error of the terms, not a measured figure: a term is 2 g w (cl - p), and w (cl - p)
    comes out of differences of coordinates of magnitude R (cancellation makes its error absolute in R, not relative to the
    small offset), through at most 8 roundings of 2^-24 each; a face's entry sums its points' terms."""
    tri, pts, rng = C.pin_surface_and_points(oracle)
    F = tri.shape[0]
    nfb = np.array([F], np.float32)
    _, cf = oracle.tri_dist_fwd(pts[None], tri[None], nfb)
    g, cls, clear = C.pin_gradient(tri, pts, cf, rng)
    stats = C.check_pin_conditions(tri, cf, cls, clear)
    want = R.envelope_gradient(pts, tri, cf, g)
    got = oracle.tri_dist_bwd(pts[None], tri[None], cf, g.reshape(1, -1, 1))[0]
    per_face = np.bincount(cf.reshape(-1).astype(np.int64), weights=np.abs(g).astype(np.float64), minlength=F)
    coord = max(np.abs(tri).max(), np.abs(pts).max())
    bound = 2 * per_face.max() * 8 * 2.0 ** -24 * coord / np.abs(want).max()
    err = C.maxnorm(got, want)
    print("pin: %s, scale %.3g, oracle max-norm error %.3g, bound %.3g" % (stats, np.abs(want).max(), err, bound))
    assert err <= bound, (err, bound)
    # what the pin would notice: a wrong sign, a wrong corner slot, weights of another corner are errors of order 1
    assert bound < 1e-4
    for wrong in (-want, np.roll(want, 1, axis=1), R.envelope_gradient(pts, tri[:, [1, 2, 0]], cf, g)):
        assert C.maxnorm(wrong, want) > 0.1
