"""The meshes and points the winding-number tests share (test_winding_ref_cpu.py checks them and the numpy tree on the CPU,
test_winding_gpu.py runs the kernels on them): the meshes of check_sign_ref.py under a seeded rotation, an open sphere and a flipped
one, with points uniform in the enlarged box and at NEAR_OFFSET from the surface.  Everything is made once per process."""
import functools

import numpy as np

from tests import check_sign_ref as R

OPEN_CUT = 0.5            # the open sphere: faces whose centroid lies above this share of the radius (the top quarter of the height) are removed
BAND = 0.1                # open meshes: points whose fp64 winding number is within this of 0.5 are set aside for classification
N_UNIFORM, N_NEAR = 3000, 1000


def open_sphere(n_lat, radius=0.4):
    v, f = R.uv_sphere(n_lat, radius)
    cz = v[f].astype(np.float64)[:, :, 2].mean(1)
    return v, np.ascontiguousarray(f[cz <= OPEN_CUT * radius])


def flipped_sphere(n_lat):
    return R.uv_sphere(n_lat, flip=True)


MAKERS = {
    "sphere8": lambda: R.uv_sphere(8), "sphere24": lambda: R.uv_sphere(24), "torus24x12": lambda: R.torus(24, 12),
    "shell8": lambda: R.shell(8), "mixed8": lambda: R.mixed(8), "open8": lambda: open_sphere(8), "open24": lambda: open_sphere(24),
    "flipped8": lambda: flipped_sphere(8),
    # one more sphere per depth of the tree the chooser can return: 8, 48, 528 and 4,224 faces -> L = 0, 1, 3, 5 (224 -> 2, 2,208 -> 4)
    "sphere2": lambda: R.uv_sphere(2), "sphere4": lambda: R.uv_sphere(4), "sphere12": lambda: R.uv_sphere(12), "sphere33": lambda: R.uv_sphere(33),
}
WATERTIGHT = ("sphere8", "torus24x12", "shell8", "mixed8")          # where parity and the winding number must agree
OPEN = ("open8", "open24")
FAST_CASES = ("sphere8", "sphere24", "torus24x12", "shell8", "mixed8", "open8", "flipped8", "sphere2", "sphere4", "sphere12", "sphere33")
# the meshes E0 is measured over (the same list on the CPU and, times two, as the GPU bound)
E0_CASES = FAST_CASES + ("open24",)


@functools.lru_cache(maxsize=None)
def case(name, n_uniform=N_UNIFORM, n_near=N_NEAR):
    """(verts f32 [V,3], faces int64 [F,3], points f32 [P,3]) of a named mesh, rotated by a seed of its own"""
    seed = 100 + sorted(MAKERS).index(name)
    v, f = MAKERS[name]()
    v = R.rotate(v, seed)
    return v, f, R.points_for(v, f, n_uniform, n_near, seed + 1000)


@functools.lru_cache(maxsize=None)
def exact64(name, n_uniform=N_UNIFORM, n_near=N_NEAR):
    """the fp64 winding numbers of case(name): computed once, shared, never modified"""
    v, f, p = case(name, n_uniform, n_near)
    w = R.winding_number(v, f, p)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------------------------------ the accuracy contract
BETA = 3.0                        # the default opening ratio the library ships
E0 = 0.016373185087338413         # measured: largest error of tests/winding_ref.py (fp64, BETA) against the exact fp64 value over E0_CASES
E_FAST = 2.0 * E0                 # the GPU fast path against exact fp64: the margin covers fp32 and far/near decisions that flip under rounding
E_FAST_CAP = 0.05                 # a condition, not a measurement
EXACT_MEASURED = 3.505e-6         # measured on an MI355X: largest |exact path - fp64| over the cases of test_exact_against_fp64_at_wave_edges
EXACT_TOL = min(4.0 * EXACT_MEASURED, 1e-3)     # four times the measurement, never above 1e-3 (integers stay unambiguous)


def cone(n=24):
    """an open fan of n long triangles from the origin to a small circle about (0.9, 0.9, 0.9): every centroid lies in the upper
    octant of the box, so all faces land in ONE leaf of a tree that has eight (24 faces: L = 1)"""
    t = 2.0 * np.pi * np.arange(n) / n
    u, w = np.float64([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.float64([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    ring = 0.9 + 0.08 * (np.cos(t)[:, None] * u[None] + np.sin(t)[:, None] * w[None])
    v = np.concatenate([[[0.0, 0.0, 0.0]], ring]).astype(np.float32)
    i = np.arange(n, dtype=np.int64)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1)
