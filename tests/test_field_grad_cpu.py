"""CPU tests of the field gradients on the tets: the restatements of tests/field_grad_ref.py against the fp64 chain
on the GPU tests' own inputs and on fields whose gradient is known, the seven symbols of the C ABI, the energies' workspace and
the argument checks (all refused by name before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import field_grad_ref as ref
from tests.tol import check_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5
EINVAL, ELIMIT = -1, -4
SYMBOLS = ["deftet_tet_field_gradient_fwd_f32", "deftet_tet_field_gradient_bwd_f32", "deftet_tet_field_energies_workspace_bytes",
           "deftet_tet_field_energies_fwd_f32", "deftet_tet_field_energies_bwd_f32", "deftet_tet_to_vertex_fwd_f32",
           "deftet_tet_to_vertex_bwd_f32"]

_raw = ctypes.create_string_buffer(1 << 16)
P = ctypes.c_void_p((ctypes.addressof(_raw) + 255) // 256 * 256)      # stands for a device pointer: checked, never followed


@pytest.fixture(scope="module")
def lib():
    from deftet_amd import _lib, build
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("R,B,C,per_shape", [(4, 1, 1, False), (6, 1, 4, False), (6, 3, 3, True), (8, 3, 8, False)])
def test_fp32_restatements_lie_within_the_bound_of_the_fp64_chain(R, B, C, per_shape):
    pos, tets = ref.mesh(R, B, per_shape)
    V = pos.shape[1]
    field = ref.normal_field((B, V, C))
    live = ref.live_mask(pos, tets)
    assert live.all()
    f64, p64 = torch.from_numpy(field).double(), torch.from_numpy(pos).double()
    g64, v64 = ref.chain64(f64, p64, tets, live)
    g32, v32 = ref.gradient(field, pos, tets)
    name = "tfg.cpu.R%d.B%d.C%d" % (R, B, C)
    check_close(name + ".grad", g32, g64, BOUND)
    check_close(name + ".vol", v32, v64, BOUND)
    check_close(name + ".grad.np64", ref.gradient(field, pos, tets, np.float64)[0], g64, 1e-12)
    check_close(name + ".energies", ref.energies(field, pos, tets, 1.0), ref.energies64(f64, p64, tets, live, 1.0), BOUND)
    assert float(np.sqrt((g64.numpy() ** 2).sum(-1)).min()) > 0.05      # the inputs stay away from the Eikonal kink


def test_a_linear_field_has_its_slope_in_every_tet():
    pos, tets = ref.mesh(6, 3)
    a = np.array([[0.6, -0.8, 0.0], [1.0, 2.0, -2.0]])                   # |a| = 1 and 3
    exact = pos.astype(np.float64) @ a.T + np.array([0.25, -0.5])        # [B,V,2]
    field = exact.astype(np.float32)
    g, vol = ref.gradient(exact, pos, tets, np.float64)
    assert np.abs(g - a[None, None]).max() < 1e-12
    g32, _ = ref.gradient(field, pos, tets)
    check_close("tfg.cpu.linear", g32, np.broadcast_to(a, g32.shape), 1e-5)
    assert vol.min() > 0 and abs(vol.sum(1) - 1.0).max() < 1e-6          # the jitter moves interior vertices only: the cube keeps volume 1
    for dtype, tol in ((np.float64, 1e-6), (np.float32, 1e-5)):
        e1 = ref.energies(field, pos, tets, 1.0, dtype)
        e3 = ref.energies(field, pos, tets, 3.0, dtype)
        assert np.abs(e1[:, :, 0] - [1.0, 9.0]).max() < 9 * tol          # Dirichlet: |a|^2
        assert np.abs(e1[:, 0, 1]).max() < tol and np.abs(e3[:, 1, 1]).max() < 9 * tol       # Eikonal: 0 where |a| = target
        assert np.abs(e1[:, 1, 1] - 4.0).max() < 9 * tol and np.abs(e3[:, 0, 1] - 4.0).max() < 9 * tol


def test_dead_tets_give_nothing():
    pos, tets, dead, lonely = ref.dead_tet_mesh()
    V = pos.shape[1]
    field = ref.normal_field((1, V, 2))
    g, vol = ref.gradient(field, pos, tets)
    assert np.all(g[0, list(dead)] == 0) and np.all(vol[0, list(dead)] == 0) and np.isfinite(g).all()
    keep = np.delete(np.arange(len(tets)), dead)
    check_close("tfg.cpu.dead.energies", ref.energies(field, pos, tets, 1.0, np.float64), ref.energies(field, pos, tets[keep], 1.0, np.float64), 1e-12)
    out, wsum = ref.tet_to_vertex(g.reshape(1, len(tets), 6), tets, V, weights=vol, fill=-3.0)
    assert np.all(out[0, lonely] == -3.0) and wsum[0, lonely] == 0 and np.all(out[0, V - 1] == -3.0)


def test_tet_to_vertex_of_a_constant_is_that_constant_and_fill_elsewhere():
    pos, tets = ref.mesh(6, 3, True)
    V = pos.shape[1]
    tets = tets[:, :65]                                                  # some vertices lose every incidence
    used = np.zeros((3, V), bool)
    for b in range(3):
        used[b, tets[b].reshape(-1)] = True
    assert used.any() and not used.all()
    val = np.full((3, 65, 2), 0.375, np.float32)
    out, wsum = ref.tet_to_vertex(val, tets, V, fill=-1.0)               # a dyadic constant: the plain mean is exact
    assert np.all(out[used] == 0.375) and np.all(out[~used] == -1.0) and np.all(wsum[~used] == 0)
    counts = np.stack([np.bincount(tets[b].reshape(-1), minlength=V) for b in range(3)])
    assert np.array_equal(wsum, counts.astype(np.float32))
    w = np.abs(ref.normal_field((3, 65))) + 0.5
    out, _ = ref.tet_to_vertex(val, tets, V, weights=w, fill=-1.0)
    assert np.abs(out[used] - 0.375).max() < 1e-6 and np.all(out[~used] == -1.0)
    # the backward is the transpose of the forward: <gout, fwd(val)> = <bwd(gout), val> on the referenced vertices
    val = ref.normal_field((3, 65, 2))
    out, wsum = ref.tet_to_vertex(val, tets, V, weights=w)
    gout = ref.normal_field((3, V, 2))[:, ::-1].copy()
    gval = ref.tet_to_vertex_bwd(gout, wsum, tets, weights=w)
    lhs = float((gout.astype(np.float64) * out * used[:, :, None]).sum())
    assert abs(lhs - float((gval.astype(np.float64) * val).sum())) < 1e-4 * max(1.0, abs(lhs))


# ---------------------------------------------------------------------------- the C ABI
def test_header_note_ctypes_table_and_library_agree(lib):
    from deftet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "deftet_hip.h")).read()
    note = re.search(r"^/\* 390:(.*?)\*/", txt, flags=re.S | re.M)
    assert note, "no 390: version note"
    for s in SYMBOLS:
        assert re.sub(r"_(fwd|bwd)_f32$", "", s) in note.group(1), s
    declared = set(re.findall(r"\b(deftet_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert lib.deftet_version() >= 390


@pytest.mark.parametrize("B", [1, 3, 8])
def test_energies_workspace_is_the_layout_and_one_byte_short_is_refused(lib, B):
    got = lib.deftet_tet_field_energies_workspace_bytes(B)
    assert got == (B * 64 * 17 * 8 + 255) // 256 * 256                    # 64 partials of 17 doubles per shape
    args = lambda ws, n: (P, P, P, None, P, 1.0, B, 27, 48, 1, 3, ws, n, None)
    for ws, n in ((None, got), (P, got - 1), (ctypes.c_void_p(P.value + 16), got)):
        assert lib.deftet_tet_field_energies_fwd_f32(*args(ws, n)) == EINVAL
        assert b"workspace null, misaligned or too small: need %d bytes" % got in lib.deftet_last_error()
    assert lib.deftet_tet_field_energies_fwd_f32(*args(P, got)) == EINVAL and b"null pointer" in lib.deftet_last_error()
    assert lib.deftet_tet_field_energies_workspace_bytes(-1) == 0


def test_bad_arguments_are_refused_by_name(lib):
    gf, gb = lib.deftet_tet_field_gradient_fwd_f32, lib.deftet_tet_field_gradient_bwd_f32
    ef, eb = lib.deftet_tet_field_energies_fwd_f32, lib.deftet_tet_field_energies_bwd_f32
    vf, vb = lib.deftet_tet_to_vertex_fwd_f32, lib.deftet_tet_to_vertex_bwd_f32
    err = lib.deftet_last_error
    for C, V, Bi, msg in ((0, 10, 1, b"at least one channel"), (4, -1, 1, b"negative size"), (4, 10, 2, b"batch must be 1 or")):
        assert gf(P, P, P, P, None, 3, V, 20, Bi, C, None) == EINVAL and msg in err() and b"tet_field_gradient:" in err()
        assert gb(P, None, P, P, P, P, P, P, P, 3, V, 20, Bi, C, None) == EINVAL and msg in err() and b"tet_field_gradient_bwd:" in err()
        assert vf(P, None, P, P, P, P, 0.0, 3, V, 20, Bi, C, None) == EINVAL and msg in err() and b"tet_to_vertex:" in err()
        assert vb(P, P, None, P, P, 3, V, 20, Bi, C, None) == EINVAL and msg in err() and b"tet_to_vertex_bwd:" in err()
    # the energies take 1..8 channels
    for C in (0, 9, 33):
        assert ef(P, P, P, P, P, 1.0, 1, 10, 20, 1, C, P, 1 << 20, None) == EINVAL and b"between 1 and 8 channels" in err()
        assert eb(P, P, 1.0, P, P, P, P, P, P, P, 1, 10, 20, 1, C, None) == EINVAL and b"between 1 and 8 channels" in err()
    # null and misaligned pointers
    off = ctypes.c_void_p(P.value + 4)
    assert gf(P, P, None, P, None, 1, 10, 20, 1, 4, None) == EINVAL and b"null pointer" in err()
    assert gf(P, P, P, None, None, 1, 10, 20, 1, 4, None) == EINVAL and b"null pointer" in err()      # neither out nor vol
    assert gf(P, P, off, P, None, 1, 10, 20, 1, 4, None) == EINVAL and b"16-byte aligned" in err()
    assert gb(None, None, P, P, P, P, P, P, P, 1, 10, 20, 1, 4, None) == EINVAL and b"null pointer" in err()
    assert gb(P, None, P, P, off, P, P, P, P, 1, 10, 20, 1, 4, None) == EINVAL and b"16-byte aligned" in err()
    assert vf(P, None, None, P, P, P, 0.0, 1, 10, 20, 1, 4, None) == EINVAL and b"null pointer" in err()
    assert vf(P, None, P, P, P, None, 0.0, 1, 10, 20, 1, 4, None) == EINVAL and b"null pointer" in err()  # the weight sums are required
    assert vb(P, P, None, off, P, 1, 10, 20, 1, 4, None) == EINVAL and b"16-byte aligned" in err()
    # sizes past what the grids and indices hold
    assert gf(P, P, P, P, None, 70000, 10, 20, 1, 4, None) == ELIMIT and b"65535" in err()
    assert gf(P, P, P, P, None, 8, 10, 1 << 27, 1, 4, None) == ELIMIT and b"31 bits" in err()
    # nothing to do is not an error
    assert gf(None, None, None, None, None, 0, 10, 20, 1, 4, None) == 0
    assert gf(None, None, None, None, None, 2, 10, 0, 1, 4, None) == 0
    assert vb(None, None, None, None, None, 2, 10, 0, 1, 4, None) == 0
    assert vf(None, None, None, None, None, None, 0.0, 2, 0, 20, 1, 4, None) == 0


def test_front_end_refuses_cpu_tensors_and_bad_shapes():
    from deftet_amd import _lib, hip_ops
    field, pos, tets = torch.zeros(1, 5, 2), torch.zeros(1, 5, 3), torch.zeros(3, 4, dtype=torch.int64)
    for call in (lambda: hip_ops.tet_field_gradient(field, pos, tets), lambda: hip_ops.tet_field_energies(field, pos, tets),
                 lambda: hip_ops.tet_to_vertex(torch.zeros(1, 3, 2), tets, 5), lambda: hip_ops.vertex_field_gradient(field, pos, tets)):
        with pytest.raises(_lib.DefTetHipError):
            call()
    with pytest.raises(RuntimeError):
        hip_ops.tet_to_vertex(torch.zeros(3, 2), tets, 5)                 # values without a batch dimension
    for name in ("tet_field_gradient_fwd", "tet_field_gradient_bwd", "tet_to_vertex_fwd", "tet_to_vertex_bwd", "tet_volumes"):
        assert callable(getattr(hip_ops, name))
