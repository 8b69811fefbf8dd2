// pointvoxel.hpp — the one statement of the trilinear arithmetic: the voxel coordinate of a point, the eight
// corners of its cell and the slope of one volume along the three axes.  pointvoxel.hip and tet_centroid_sample.hip both include
// it, so a value sampled at a tet centroid and its gradients are the SAME expressions as the point sampler's, not a restatement
// of them.  Anonymous namespace: each translation unit gets its own copy.  (The sort plumbing lives in cell_gather.hpp.)
#pragma once
#include "common.hpp"

namespace deftet {
namespace {

// u of one point per axis: `raw` before the clamp (the border rule of the position gradient reads it), `u` after it.
// pos_mode 0: pos f32 [B,N,3], normalised: u = clamp((pos + 0.5) r, 0, r - 1)   (sample_f's arithmetic, in that order)
// pos_mode 1: coords f32 [B,3,N] in voxel units: u = clamp(coords, 0, r - 1)    (trilinear_devoxelize's argument)
// fmaxf / fminf return the other operand for a NaN, so a NaN lands on 0 and every index below stays inside the volume.
__device__ __forceinline__ void load_u(const float *__restrict__ pos, int mode, int b, int p, int N, int r, float raw[3], float u[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        raw[j] = mode == 0 ? (pos[((size_t)b * N + p) * 3 + j] + 0.5f) * (float)r : pos[((size_t)b * 3 + j) * N + p];
        u[j] = fminf(fmaxf(raw[j], 0.0f), (float)(r - 1));
    }
}

// the cell of u: lo corner, the eight linear indices and weights (corner k = 4 kx + 2 ky + kz, z fastest).
// legacy: hi = lo where d == 0 (trilinear_devox.cu:64-75), else hi = min(lo + 1, r - 1); both stay below r as u <= r - 1.
struct Corners {
    int idx[8];
    float w[8];
};
__device__ __forceinline__ void corners_of(const float u[3], int r, bool legacy, Corners &c)
{
    int lo[3], hi[3];
    float d1[3], d0[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float f = floorf(u[j]);
        d1[j] = u[j] - f;
        d0[j] = 1.0f - d1[j];
        lo[j] = (int)f;
        hi[j] = legacy ? lo[j] + (d1[j] > 0.0f ? 1 : 0) : min(lo[j] + 1, r - 1);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int kx = k >> 2, ky = (k >> 1) & 1, kz = k & 1;
        c.idx[k] = ((kx ? hi[0] : lo[0]) * r + (ky ? hi[1] : lo[1])) * r + (kz ? hi[2] : lo[2]);
        c.w[k] = ((kx ? d1[0] : d0[0]) * (ky ? d1[1] : d0[1])) * (kz ? d1[2] : d0[2]);
    }
}

// the sampled value of one channel: the eight rounded products added in corner order 000 .. 111
__device__ __forceinline__ float sample_corners(const float *__restrict__ f, const Corners &cn)
{
    float acc = __fmul_rn(cn.w[0], f[cn.idx[0]]);
#pragma unroll
    for (int k = 1; k < 8; ++k) acc = __fadd_rn(acc, __fmul_rn(cn.w[k], f[cn.idx[k]]));
    return acc;
}

// The gradient of one volume's channels [0, C) with respect to the position of point p, res[3]: the channel sum from 0 in
// ascending order, times the scale of the position mode, and grid_sample's border rule: no gradient for a coordinate the clamp
// holds (u <= 0 or u >= r - 1, a NaN included).  vol f32 [B,C,R,R,R]; gout f32 [B,C_total,N], this volume's rows from c_off.
__device__ __forceinline__ void pos_grad_of_volume(const float *__restrict__ vol, const float *__restrict__ gout, const float raw[3],
                                                   const float u[3], int b, int p, int C, int R, int N, int c_off, int C_total, int mode,
                                                   float res[3])
{
    Corners cn;
    corners_of(u, R, false, cn);
    float d1[3], d0[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d1[j] = u[j] - floorf(u[j]);
        d0[j] = 1.0f - d1[j];
    }
    const float wyz[4] = {d0[1] * d0[2], d0[1] * d1[2], d1[1] * d0[2], d1[1] * d1[2]};
    const float wxz[4] = {d0[0] * d0[2], d0[0] * d1[2], d1[0] * d0[2], d1[0] * d1[2]};
    const float wxy[4] = {d0[0] * d0[1], d0[0] * d1[1], d1[0] * d0[1], d1[0] * d1[1]};
    const size_t R3 = (size_t)R * R * R;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float *f = vol + ((size_t)b * C + c) * R3;
        const float go = gout[((size_t)b * C_total + c_off + c) * N + p];
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = f[cn.idx[k]];
        const float ddx = (v[4] - v[0]) * wyz[0] + (v[5] - v[1]) * wyz[1] + (v[6] - v[2]) * wyz[2] + (v[7] - v[3]) * wyz[3];
        const float ddy = (v[2] - v[0]) * wxz[0] + (v[3] - v[1]) * wxz[1] + (v[6] - v[4]) * wxz[2] + (v[7] - v[5]) * wxz[3];
        const float ddz = (v[1] - v[0]) * wxy[0] + (v[3] - v[2]) * wxy[1] + (v[5] - v[4]) * wxy[2] + (v[7] - v[6]) * wxy[3];
        gx += go * ddx;
        gy += go * ddy;
        gz += go * ddz;
    }
    const float scale = mode == 0 ? (float)R : 1.0f, top = (float)(R - 1);
    res[0] = raw[0] > 0.0f && raw[0] < top ? scale * gx : 0.0f;
    res[1] = raw[1] > 0.0f && raw[1] < top ? scale * gy : 0.0f;
    res[2] = raw[2] > 0.0f && raw[2] < top ? scale * gz : 0.0f;
}

}  // namespace
}  // namespace deftet
