"""The fp64 winding-number reference of check_sign_ref.py, checked on its own, and the proof that the inputs of
test_check_sign_sizes_gpu.py are fair: on every mesh kind (about 8k faces, 600 uniform + 400 near-surface
points) the winding number is an integer, agrees with the analytic answer where there is one, the ray-parity
oracle agrees with it at every point that is not set aside, and at most 1 % of the points are set aside.  The
1 % cap is a condition on the inputs, not a measurement: if a case exceeds it, the inputs change, never the cap.

Set-aside shares measured here (600 uniform / 400 near-surface / all 1,000 points, in %): sphere_rot 0.17 / 0.00 / 0.10;
sphere, torus, torus_rot, shell_rot and mixed_rot 0.00 / 0.00 / 0.00.  Mismatches between the oracle and the winding parity:
0 in every case, set aside or not."""
import numpy as np
import pytest

from tests import check_sign_ref as R

N_UNIFORM, N_NEAR = 600, 400
MAX_SET_ASIDE = 0.01


def _mesh(kind):
    if kind == "sphere":                                            # the one unrotated case: rings in planes z = const
        return R.uv_sphere(45)
    if kind == "sphere_rot":
        v, f = R.uv_sphere(45)
        return R.rotate(v, 11), f
    if kind == "torus":
        return R.torus(80, 50)
    if kind == "torus_rot":
        v, f = R.torus(80, 50)
        return R.rotate(v, 12), f
    if kind == "shell_rot":
        v, f = R.shell(33)
        return R.rotate(v, 13), f
    v, f = R.mixed(45)
    return R.rotate(v, 14), f


KINDS = ["sphere", "sphere_rot", "torus", "torus_rot", "shell_rot", "mixed_rot"]
_cache = {}


def _case(kind):
    """computed once per kind and shared, never modified"""
    if kind not in _cache:
        v, f = _mesh(kind)
        p = R.points_for(v, f, N_UNIFORM, N_NEAR, seed=100 + KINDS.index(kind))
        w = R.winding_number(v, f, p)
        _cache[kind] = (v, f, p, w, R.set_aside(v, f, p))
    return _cache[kind]


def test_makers_are_closed_and_outward():
    for kind in KINDS:
        v, f = _mesh(kind)
        assert v.dtype == np.float32 and f.dtype == np.int64 and f.min() == 0 and f.max() == v.shape[0] - 1
        assert 7900 <= f.shape[0] <= 8500, (kind, f.shape)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = e[:, 0] * v.shape[0] + e[:, 1]
        assert np.unique(key).size == key.size                                            # every directed edge once ...
        assert np.array_equal(np.sort(key), np.sort(e[:, 1] * v.shape[0] + e[:, 0]))      # ... and its reverse once: closed, oriented
    ball = lambda r: 4 / 3 * np.pi * r ** 3                         # noqa: E731  (outward: positive; inscribed: a little less)
    assert 0.98 * ball(0.4) < R.signed_volume(*R.uv_sphere(45)) < ball(0.4)
    assert 0.98 < R.signed_volume(*R.torus(80, 50)) / (2 * np.pi ** 2 * 0.3 * 0.1 ** 2) < 1.0
    vs, fs = R.shell(33)
    assert 0.98 < R.signed_volume(vs, fs) / (ball(R.SHELL_R[0]) - ball(R.SHELL_R[1])) < 1.0
    vc, fc = R.cube()
    assert abs(R.signed_volume(vc, fc) - (2 * R.CUBE_H) ** 3) < 1e-6
    assert R.sphere_faces_of(513) == 1050624 and R.uv_sphere(20)[1].shape[0] == R.sphere_faces_of(20)
    q = R.rotation(3)
    assert np.abs(q @ q.T - np.eye(3)).max() < 1e-14


@pytest.mark.parametrize("kind", KINDS)
def test_winding_number_is_an_integer(kind):
    v, f, p, w, _ = _case(kind)
    assert np.abs(w - np.round(w)).max() <= 1e-9
    assert set(np.unique(np.round(w).astype(int))) <= {0, 1, 2}
    assert R.winding_inside(w).any() and not R.winding_inside(w).all()


@pytest.mark.parametrize("kind", ["sphere", "sphere_rot", "shell_rot"])
def test_winding_equals_the_radius_test(kind):
    v, f, p, w, _ = _case(kind)
    d = np.linalg.norm(p.astype(np.float64), axis=1)
    if kind == "shell_rot":
        want = (d < R.SHELL_R[0]) & (d > R.SHELL_R[1])
        clear = (np.abs(d - R.SHELL_R[0]) > 1e-3) & (np.abs(d - R.SHELL_R[1]) > 1e-3)
    else:
        want, clear = d < 0.4, np.abs(d - 0.4) > 1e-3
    assert clear.sum() > 0.9 * p.shape[0]
    assert np.array_equal(R.winding_inside(w)[clear], want[clear])


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_parity_equals_winding_parity(oracle, kind):
    v, f, p, w, aside = _case(kind)
    got, cnt = oracle.check_sign(v[None], f, p[None], return_count=True)
    want = R.winding_inside(w)
    diff = got[0] != want
    share = [aside[:N_UNIFORM].mean(), aside[N_UNIFORM:].mean(), aside.mean()]
    print("%s: %d faces, set aside %.2f %% of the uniform, %.2f %% of the near-surface, %.2f %% of all points; "
          "mismatches %d, of them not set aside %d; largest crossing count %d"
          % (kind, f.shape[0], 100 * share[0], 100 * share[1], 100 * share[2], diff.sum(), (diff & ~aside).sum(), cnt.max()))
    assert not (diff & ~aside).any()
    assert aside.mean() <= MAX_SET_ASIDE
    assert cnt.max() >= (4 if kind in ("torus", "torus_rot", "shell_rot") else 2)


def test_torch_float64_gives_the_numpy_answer():
    """the GPU tests run the same code on torch.float64 tensors"""
    import torch
    v, f, p, w, aside = _case("torus_rot")
    pt, ft = torch.from_numpy(p[:200]), torch.from_numpy(f)
    wt = R.winding_number(torch.from_numpy(v), ft, pt)
    assert wt.dtype == torch.float64 and np.abs(wt.numpy() - w[:200]).max() < 1e-12
    assert np.array_equal(R.winding_inside(wt).numpy(), R.winding_inside(w[:200]))
    assert np.array_equal(R.set_aside(torch.from_numpy(v), ft, pt).numpy(), aside[:200])


def test_set_aside_marks_what_it_should():
    """rays through a vertex, through an edge, from a point on the surface and through an edge-on face are set aside;
    a ray through the middle of a face is not; without the dead-zone rule the edge-on face goes unnoticed"""
    v = np.float32([[0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0], [1, 1e-8, 1]])
    f = np.int64([[0, 1, 2], [0, 3, 4]])                           # face 1 is edge-on to +x: |a| = 1e-8
    p = np.float32([[-1, 0.25, 0.25], [-1, 0, 0.5], [-1, 1, 0], [0, 0.3, 0.3], [1, 0.25, 0.25], [-1, 0.5, 0.5 + 1e-3],
                    [0.5, 0.2e-8, 0.2], [-1, 0.25, 0.251]])
    assert R.set_aside(v, f, p).tolist() == [False, True, True, True, False, False, True, False]
    assert R.set_aside(v, f, p, orientation_test=False).tolist() == [False, True, True, True, False, False, False, False]
    far = np.float32([[0.002, 0.3, 0.3]])                          # the face lies 2e-3 BEHIND the point: not looked at
    assert not R.set_aside(v, f[:1], far).any()


def test_a_twice_reversed_inner_sphere_is_noticed(oracle):
    """the pin can fail: with the inner sphere of the shell outward again the winding number inside it is 2, not 0 —
    so a mesh maker that got the orientation wrong would show in the integer values — while its parity stays that
    of the ray; and a winding number that ignored the inner sphere disagrees with the ray parity"""
    v, f, p, w, aside = _case("shell_rot")
    n = f.shape[0] // 2
    f2 = np.concatenate([f[:n], f[n:, ::-1]])
    inner = np.linalg.norm(p.astype(np.float64), axis=1) < R.SHELL_R[1] - 1e-3
    assert inner.sum() > 20
    assert np.all(np.round(w[inner]) == 0) and np.all(np.round(R.winding_number(v, f2, p[inner])) == 2)
    got = oracle.check_sign(v[None], f, p[None])[0]
    assert (got[inner] != R.winding_inside(R.winding_number(v, f[:n], p[inner]))).all()


def test_the_dead_zone_rule_is_needed(oracle):
    """a sphere small enough that its silhouette faces fall into the contract's dead zone |a| < 1e-7: there ray parity and
    winding parity do differ, every such point is set aside by the dead-zone rule, and without that rule some are not — so
    the parity tests fail if set_aside stops looking at the projected area"""
    v, f = R.uv_sphere(12, radius=0.004)
    v = R.rotate(v, 15)
    p = R.uniform_points(v, 3000, seed=16, grow=0.0)
    diff = oracle.check_sign(v[None], f, p[None])[0] != R.winding_inside(R.winding_number(v, f, p))
    assert diff.sum() >= 10
    assert not (diff & ~R.set_aside(v, f, p)).any()
    assert (diff & ~R.set_aside(v, f, p, orientation_test=False)).sum() >= 10
