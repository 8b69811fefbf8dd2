// image_sample.hpp — the one statement of the bilinear arithmetic of image_sample.hip: the pixel coordinate of a
// uv pair, the four corners of its cell with their weights and in-map masks, the cell key the map backward sorts by and the slope
// of one channel along x and y.  The forward, the sorted weights and both backward kernels call these, so a value and its
// gradients are the same expressions.  Anonymous namespace, as cell_gather.hpp.
#pragma once
#include "cell_gather.hpp"                      // kPvBlock, the sort by cell, the corner partials and their workspace

namespace deftet {
namespace {

// grid_sample's unnormalisation: -1 .. 1 spans the image
__device__ __forceinline__ float pixel_of(float x, int size, int align)
{
    return align ? (x + 1.0f) * 0.5f * (float)(size - 1) : ((x + 1.0f) * (float)size - 1.0f) * 0.5f;
}

// The cell of one point.  Corner k = 2 ky + kx: (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1); w[k] = (x factor) * (y factor);
// m[k]: the corner lies in the map (idx[k] is its texel, 0 otherwise and then never read).
// out: the point is fully outside (decided in float before any conversion: +-1e30, +-inf and NaN land here under `zeros`);
// every mask is off, x0 = y0 = 0.  hx / hy (border only): the clamp holds the coordinate, so it has no gradient; fmaxf / fminf
// return the other operand for a NaN, which therefore reads pixel 0.
struct Tap {
    int idx[4], x0, y0;
    float w[4], tx, ty;
    bool m[4], out, hx, hy;
};
__device__ __forceinline__ void tap_of(float u, float v, int H, int W, int border, int align, Tap &t)
{
    float ix = pixel_of(u, W, align), iy = pixel_of(v, H, align);
    t.hx = t.hy = false;
    if (border) {
        t.hx = !(ix > 0.0f && ix < (float)(W - 1));
        t.hy = !(iy > 0.0f && iy < (float)(H - 1));
        ix = fminf(fmaxf(ix, 0.0f), (float)(W - 1));
        iy = fminf(fmaxf(iy, 0.0f), (float)(H - 1));
    }
    t.out = !(ix > -1.0f && ix < (float)W) || !(iy > -1.0f && iy < (float)H);
    if (t.out) ix = iy = 0.0f;
    const float fx = floorf(ix), fy = floorf(iy);
    t.tx = ix - fx;
    t.ty = iy - fy;
    t.x0 = (int)fx;                             // in [-1, W-1] x [-1, H-1] by the test above
    t.y0 = (int)fy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kx = k & 1, ky = k >> 1, cx = t.x0 + kx, cy = t.y0 + ky;
        t.m[k] = !t.out && cx >= 0 && cx < W && cy >= 0 && cy < H;
        t.idx[k] = t.m[k] ? cy * W + cx : 0;
        t.w[k] = (kx ? t.tx : 1.0f - t.tx) * (ky ? t.ty : 1.0f - t.ty);
    }
}

// the cells of one map: lo corners [-1, W-1] x [-1, H-1], so that a partially-outside cell has a key of its own
__device__ __host__ __forceinline__ int cells_of(int H, int W) { return (H + 1) * (W + 1); }
__device__ __forceinline__ int cell_of(const Tap &t, int W) { return (t.y0 + 1) * (W + 1) + (t.x0 + 1); }

// the value of one channel plane: the four rounded products in corner order; a corner outside the map adds 0 and is not read
__device__ __forceinline__ float sample_tap(const float *__restrict__ f, const Tap &t)
{
    float acc = t.m[0] ? __fmul_rn(t.w[0], f[t.idx[0]]) : 0.0f;
#pragma unroll
    for (int k = 1; k < 4; ++k) acc = __fadd_rn(acc, t.m[k] ? __fmul_rn(t.w[k], f[t.idx[k]]) : 0.0f);
    return acc;
}

// d value / d (ix, iy) of one channel plane, texels outside the map counting as 0 (what grid_sample does under `zeros`)
__device__ __forceinline__ void slope_tap(const float *__restrict__ f, const Tap &t, float &ddx, float &ddy)
{
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = t.m[k] ? f[t.idx[k]] : 0.0f;
    ddx = (v[1] - v[0]) * (1.0f - t.ty) + (v[3] - v[2]) * t.ty;
    ddy = (v[2] - v[0]) * (1.0f - t.tx) + (v[3] - v[1]) * t.tx;
}

}  // namespace
}  // namespace deftet
