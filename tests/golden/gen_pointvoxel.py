#!/usr/bin/env python
"""Generates tests/golden/pointvoxel_*.npz: inputs and outputs of the reference's average-voxelization and trilinear
devoxelization kernels (layers/pv_module/functional/src/voxelization/vox.cu, src/interpolate/trilinear_devox.cu), run on the
host: the kernel bodies are compiled as host C++ through the shim below, which includes them by path from
the reference tree, with -ffp-contract=off and ONE thread per block, so every loop runs in ascending point order.
Everything is built in a scratch directory; only inputs and outputs are stored here — no reference text, no binary.

    REF=<reference tree> python tests/golden/gen_pointvoxel.py

Cases: B = 2, C = 3, N = 257 at R = 2 and R = 8; N = 300 points in one voxel / one cell at R = 8.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REF") or ""
SRC = os.path.join(REF, "layers", "pv_module", "functional", "src")

SHIM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#define __global__
struct Idx3 { int x, y, z; };
static Idx3 blockIdx, blockDim, threadIdx;
static inline void atomicAdd(int *p, int v) { *p += v; }
static inline void atomicAdd(float *p, float v) { *p += v; }
#include "k/vox_kernels.inc"          /* their `#include "../cuda_utils.cuh"` finds the empty stub beside this file */
#include "k/devox_kernels.inc"
static void one_thread() { blockDim = {1, 1, 1}; threadIdx = {0, 0, 0}; }
extern "C" void run_vox(int b, int c, int n, int r, const int *coords, const float *feat, int *ind, int *cnt, float *out) {
    one_thread();
    for (int i = 0; i < b; ++i) { blockIdx = {i, 0, 0}; grid_stats_kernel(b, n, r, r * r, r * r * r, coords, ind, cnt); }
    for (int i = 0; i < b; ++i) { blockIdx = {i, 0, 0}; avg_voxelize_kernel(b, c, n, r * r * r, ind, cnt, feat, out); }
}
extern "C" void run_vox_grad(int b, int c, int n, int s, const int *ind, const int *cnt, const float *gy, float *gx) {
    one_thread();
    for (int i = 0; i < b; ++i) { blockIdx = {i, 0, 0}; avg_voxelize_grad_kernel(b, c, n, s, ind, cnt, gy, gx); }
}
extern "C" void run_devox(int b, int c, int n, int r, const float *coords, const float *feat, int *inds, float *wgts, float *outs) {
    one_thread();
    for (int i = 0; i < b; ++i) { blockIdx = {i, 0, 0}; trilinear_devoxelize_kernel(b, c, n, r, r * r, r * r * r, true, coords, feat, inds, wgts, outs); }
}
extern "C" void run_devox_grad(int b, int c, int n, int r3, const int *inds, const float *wgts, const float *gy, float *gx) {
    one_thread();
    for (int i = 0; i < b; ++i) { blockIdx = {i, 0, 0}; trilinear_devoxelize_grad_kernel(b, c, n, r3, inds, wgts, gy, gx); }
}
"""


def kernels_only(path, out):
    """the file up to its first host launcher (they use the <<< >>> launch syntax), written into the scratch directory"""
    lines = open(path).read().split("\n")
    cut = next(i for i, l in enumerate(lines) if l.startswith("void "))
    open(out, "w").write("\n".join(lines[:cut]) + "\n")


def build(tmp):
    os.mkdir(os.path.join(tmp, "k"))
    kernels_only(os.path.join(SRC, "voxelization", "vox.cu"), os.path.join(tmp, "k", "vox_kernels.inc"))
    kernels_only(os.path.join(SRC, "interpolate", "trilinear_devox.cu"), os.path.join(tmp, "k", "devox_kernels.inc"))
    open(os.path.join(tmp, "cuda_utils.cuh"), "w").write("/* stub: the kernel bodies need nothing of ATen / CUDA */\n")
    open(os.path.join(tmp, "shim.cpp"), "w").write(SHIM)
    lib = os.path.join(tmp, "libpvref.so")
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", tmp, os.path.join(tmp, "shim.cpp"), "-o", lib])
    return ctypes.CDLL(lib)


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def case(lib, rng, B, C, N, R, one_voxel):
    R3 = R ** 3
    if one_voxel:
        coords = np.tile(np.array([3, 5, 2], np.int32)[None, :, None], (B, 1, N))
        dv = (np.array([3, 5, 2], np.float32)[None, :, None] + rng.uniform(0.0, 0.999, (B, 3, N))).astype(np.float32)
    else:
        coords = rng.integers(0, R, (B, 3, N)).astype(np.int32)
        dv = rng.uniform(0, R - 1, (B, 3, N)).astype(np.float32)
        dv[:, :, :16] = np.round(dv[:, :, :16])                       # lattice points: d == 0, hi == lo
        dv[:, 0, 16:24] = R - 1
        dv[:, 1, 20:28] = 0
    feat = rng.standard_normal((B, C, N)).astype(np.float32)
    ind, cnt, out = np.zeros((B, N), np.int32), np.zeros((B, R3), np.int32), np.zeros((B, C, R3), np.float32)
    lib.run_vox(B, C, N, R, P(coords), P(feat), P(ind), P(cnt), P(out))
    gy = rng.standard_normal((B, C, R3)).astype(np.float32)
    gx = np.zeros((B, C, N), np.float32)
    lib.run_vox_grad(B, C, N, R3, P(ind), P(cnt), P(gy), P(gx))
    dv_feat = rng.standard_normal((B, C, R3)).astype(np.float32)
    inds, wgts, outs = np.zeros((B, 8, N), np.int32), np.zeros((B, 8, N), np.float32), np.zeros((B, C, N), np.float32)
    lib.run_devox(B, C, N, R, P(dv), P(dv_feat), P(inds), P(wgts), P(outs))
    dv_gy = rng.standard_normal((B, C, N)).astype(np.float32)
    dv_gx = np.zeros((B, C, R3), np.float32)
    lib.run_devox_grad(B, C, N, R3, P(inds), P(wgts), P(dv_gy), P(dv_gx))
    return dict(R=np.int64(R), feat=feat, coords=coords, out=out, ind=ind, cnt=cnt, gy=gy, gx=gx, dv_coords=dv, dv_feat=dv_feat,
                dv_outs=outs, dv_inds=inds, dv_wgts=wgts, dv_gy=dv_gy, dv_gx=dv_gx)


def main():
    if not os.path.isdir(SRC):
        raise SystemExit("set REF=<reference tree> (found no %s)" % SRC)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        rng = np.random.default_rng(20261017)
        for name, (N, R, one) in {"r2": (257, 2, False), "r8": (257, 8, False), "onevoxel": (300, 8, True)}.items():
            out = os.path.join(HERE, "pointvoxel_%s.npz" % name)
            np.savez_compressed(out, **case(lib, rng, 2, 3, N, R, one))
            print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    sys.exit(main())
