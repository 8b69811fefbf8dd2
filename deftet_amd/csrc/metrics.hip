// metrics.hip — the evaluation metrics of eval.py:237-260 (Engine.validate_iou) and utils/point_cloud_utils.py, forward only:
//   point-to-mesh distance   the true Euclidean distance from a point to a triangle soup (Ericson, Real-Time Collision Detection
//                            §5.1.5), an exact uniform-grid search and a streaming scan with the same evaluation;
//   surface sampling         area-weighted face choice through an exact integer CDF, then the square-root warp of k_face_samples;
//   sided distance           A10's nn_index (unchanged) plus the distance at the index, with A10's own formula;
//   metric reduction         chamfer, chamfer-L1, F-score and Hausdorff per shape, a fixed-order two-stage reduction.
// Contracts and the exactness argument of the grid search: DESIGN.md §6f.
#include <math.h>

#include "common.hpp"
#include "grid_setup.hpp"

namespace deftet {
namespace met {

// ---------------------------------------------------------------------------- closest point on a triangle
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ bool face_finite(const float *fc)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(fc[k]);
    return ok;
}

// |p - q|^2 for the closest point q of segment [a, a + ab] (t = ap·ab / ab·ab clamped to [0, 1]; ab = 0: t = 0); *end = 0 / 1 when
// t was clamped to that end, -1 inside
__device__ __forceinline__ float seg_dist(const float *a, const float *b, const float *p, int *end)
{
    const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
    const float apx = p[0] - a[0], apy = p[1] - a[1], apz = p[2] - a[2];
    const float l2 = dot3(abx, aby, abz, abx, aby, abz);
    float t = l2 > 0.f ? dot3(apx, apy, apz, abx, aby, abz) / l2 : 0.f;
    *end = -1;
    if (!(t > 0.f)) { t = 0.f; *end = 0; }
    else if (t >= 1.f) { t = 1.f; *end = 1; }
    const float dx = p[0] - (a[0] + t * abx), dy = p[1] - (a[1] + t * aby), dz = p[2] - (a[2] + t * abz);
    return (dx * dx + dy * dy) + dz * dz;
}

// Ericson's ClosestPtPointTriangle in its branch order, fp32, no contraction (the build's -ffp-contract=off).  Returns
// |p - q|^2 = ((dx*dx + dy*dy) + dz*dz), d = p - q; *type: 0 inside, 1/2/3 vertex a/b/c, 4/5/6 edge ab/bc/ca.  When the interior
// branch is reached with a denominator sum = va + vb + vc that is not > 0, or with a non-finite v or w (a zero-area face, or one
// whose area is lost to rounding), or when a branch's distance is not finite (0/0 of a degenerate face), the face takes the
// minimum over the segments ab, bc, ca, in that order.
__device__ __forceinline__ float tri_dist(const float *a, const float *b, const float *c, const float *p, int *type)
{
    const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
    const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
    const float apx = p[0] - a[0], apy = p[1] - a[1], apz = p[2] - a[2];
    float qx, qy, qz;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.f && d2 <= 0.f) { qx = a[0]; qy = a[1]; qz = a[2]; *type = 1; goto done; }
    {
        const float bpx = p[0] - b[0], bpy = p[1] - b[1], bpz = p[2] - b[2];
        const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
        if (d3 >= 0.f && d4 <= d3) { qx = b[0]; qy = b[1]; qz = b[2]; *type = 2; goto done; }
        const float vc = d1 * d4 - d3 * d2;
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
            const float v = d1 / (d1 - d3);
            qx = a[0] + v * abx; qy = a[1] + v * aby; qz = a[2] + v * abz; *type = 4; goto done;
        }
        const float cpx = p[0] - c[0], cpy = p[1] - c[1], cpz = p[2] - c[2];
        const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
        if (d6 >= 0.f && d5 <= d6) { qx = c[0]; qy = c[1]; qz = c[2]; *type = 3; goto done; }
        const float vb = d5 * d2 - d1 * d6;
        if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
            const float w = d2 / (d2 - d6);
            qx = a[0] + w * acx; qy = a[1] + w * acy; qz = a[2] + w * acz; *type = 6; goto done;
        }
        const float va = d3 * d6 - d5 * d4;
        const float e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {
            const float w = e43 / (e43 + e56);
            qx = b[0] + w * (c[0] - b[0]); qy = b[1] + w * (c[1] - b[1]); qz = b[2] + w * (c[2] - b[2]); *type = 5; goto done;
        }
        const float sum = (va + vb) + vc;
        const float denom = 1.0f / sum;
        const float v = vb * denom, w = vc * denom;
        if (!(sum > 0.f) || !isfinite(v) || !isfinite(w)) goto segments;   // zero (or rounding-level) area
        qx = (a[0] + abx * v) + acx * w; qy = (a[1] + aby * v) + acy * w; qz = (a[2] + abz * v) + acz * w;
        *type = 0;
    }
done:
    {
        const float dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (isfinite(d)) return d;                                    // else a 0/0 of a degenerate face (e.g. two equal corners)
    }
segments:
    int e0, e1, e2;
    const float s0 = seg_dist(a, b, p, &e0), s1 = seg_dist(b, c, p, &e1), s2 = seg_dist(c, a, p, &e2);
    float m = s0;
    int t = e0 < 0 ? 4 : (e0 == 0 ? 1 : 2);
    if (s1 < m) { m = s1; t = e1 < 0 ? 5 : (e1 == 0 ? 2 : 3); }
    if (s2 < m) { m = s2; t = e2 < 0 ? 6 : (e2 == 0 ? 3 : 1); }
    *type = t;
    return m;
}

__device__ __forceinline__ void take(float d, int f, int t, float &best, int &bf, int &bt)
{   // lexicographic (distance, face) minimum == first strict minimum of the ascending scan; NaN never wins
    if (d < best || (d == best && f < bf)) { best = d; bf = f; bt = t; }
}

__device__ __forceinline__ int shape_faces(const int *n_face, int b, int F)
{
    if (!n_face) return F;
    const int n = n_face[b];
    return n < 0 ? 0 : (n > F ? F : n);
}

__device__ __forceinline__ void write_result(int b, int q, int P, const float *p, float best, int bf, int bt, float *dist, long long *fidx,
                                             int *dtype)
{
    const size_t o = (size_t)b * P + q;
    const bool pf = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    dist[o] = pf ? best : NAN;
    fidx[o] = pf ? (long long)bf : -1;
    dtype[o] = pf ? bt : -1;
}

// streaming scan: every lane one point, the faces of its shape in ascending order (wave-uniform loads)
__global__ __launch_bounds__(256) void k_pm_scan(const float *__restrict__ pts, const float *__restrict__ face, const int *__restrict__ n_face,
                                                 int P, int F, float *dist, long long *fidx, int *dtype)
{
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < P;
    const float *pp = pts + ((size_t)b * P + (live ? q : 0)) * 3;
    const float p[3] = {pp[0], pp[1], pp[2]};
    const int nf = shape_faces(n_face, b, F);
    const float *__restrict__ fb = face + (size_t)b * F * 9;
    float best = INFINITY;
    int bf = -1, bt = -1;
    for (int f = 0; f < nf; ++f) {
        float fc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) fc[k] = fb[(size_t)f * 9 + k];
        if (!face_finite(fc)) continue;
        int t;
        const float d = tri_dist(fc, fc + 3, fc + 6, p, &t);
        if (d < best) { best = d; bf = f; bt = t; }
    }
    if (live) write_result(b, q, P, p, best, bf, bt, dist, fidx, dtype);
}

// ---------------------------------------------------------------------------- the grid search
// Faces are binned by bounding box into a uniform grid of at most 64 cells per axis whose cells are about one mean face extent
// wide.  A point walks shells of cells (Chebyshev rings) around its own cell and stops once the distance from it to the part of
// the grid outside the walked box, less a margin, exceeds its best distance.  "Wide" faces — outside
// |x| <= 2^20, slivers (|n|^2 < 1e-4 L^4, L the longest edge) and faces over more than kPMaxCells cells — are evaluated by
// every point; faces with a non-finite corner are skipped by both paths.
constexpr int kPGMax = 64;
constexpr int kPCells = kPGMax * kPGMax * kPGMax;
constexpr int kPMaxCells = 32;
constexpr int kPParts = 64;
constexpr float kPLimit = 1048576.0f;
constexpr float kPMargin = 1.0f / 4096.0f;   // margin = kPMargin * (grid scale + |p|_inf)

struct PGrid { float o[3], cs[3], inv[3], scale; int g[3], any; };   // any: some face is binned

__device__ __forceinline__ bool face_binned(const float *fc)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && (fabsf(fc[k]) <= kPLimit);
    if (!ok) return false;
    const float abx = fc[3] - fc[0], aby = fc[4] - fc[1], abz = fc[5] - fc[2];
    const float acx = fc[6] - fc[0], acy = fc[7] - fc[1], acz = fc[8] - fc[2];
    const float bcx = fc[6] - fc[3], bcy = fc[7] - fc[4], bcz = fc[8] - fc[5];
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float n2 = dot3(nx, ny, nz, nx, ny, nz);
    const float l2 = fmaxf(dot3(abx, aby, abz, abx, aby, abz), fmaxf(dot3(acx, acy, acz, acx, acy, acz), dot3(bcx, bcy, bcz, bcx, bcy, bcz)));
    return l2 > 0.f && n2 >= 1e-4f * l2 * l2;
}

__global__ __launch_bounds__(256) void k_pm_stats(const float *__restrict__ face, const int *__restrict__ n_face, int F, float *part)
{
    __shared__ float sh[4][8];
    const int b = blockIdx.y;
    const int nf = shape_faces(n_face, b, F);
    const float *fb = face + (size_t)b * F * 9;
    BoxStats<3, 2> bs;                                              // sums: largest box extent of the binned faces, their number
    for (int f = blockIdx.x * 256 + threadIdx.x; f < nf; f += gridDim.x * 256) {
        float fc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) fc[k] = fb[(size_t)f * 9 + k];
        if (!face_finite(fc) || !face_binned(fc)) continue;
        float l[3], h[3], w = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            l[k] = fminf(fc[k], fminf(fc[3 + k], fc[6 + k])); h[k] = fmaxf(fc[k], fmaxf(fc[3 + k], fc[6 + k]));
            w = fmaxf(w, h[k] - l[k]);
        }
        bs.add_box(l, h);
        bs.add_sum(0, w);
        bs.add_sum(1, 1.f);
    }
    bs.block_store(sh, part + ((size_t)b * kPParts + blockIdx.x) * 8);
}

__global__ __launch_bounds__(64) void k_pm_grid(const float *__restrict__ part, PGrid *grids)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    BoxStats<3, 2> bs;
    bs.load(part + ((size_t)b * kPParts + lane) * 8);
    bs.wave_reduce();
    if (lane == 0) {
        PGrid g;
        const float sw = bs.sum[0], cnt = bs.sum[1];
        const float meanw = cnt > 0.f ? sw / cnt : 0.f;
        float scale = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool ok = bs.hi[k] >= bs.lo[k];
            const float l = ok ? bs.lo[k] : 0.f, h = ok ? bs.hi[k] : 0.f, ext = h - l;
            float n = (meanw > 0.f && ext > 0.f) ? ceilf(ext / meanw) : 1.f;
            n = fminf(fmaxf(n, 1.f), (float)kPGMax);
            g.g[k] = (int)n;
            g.o[k] = l;
            g.cs[k] = ext > 0.f ? ext / n : 1.f;
            g.inv[k] = ext > 0.f ? n / ext : 0.f;
            scale = fmaxf(scale, fmaxf(fabsf(l), fabsf(h)));
        }
        g.scale = scale;
        g.any = cnt > 0.f;
        grids[b] = g;
    }
}

// mode 0: count the cells of every binned face, append the wide faces; mode 1: fill the cell lists
__global__ __launch_bounds__(256) void k_pm_bin(const float *__restrict__ face, const int *__restrict__ n_face, int F,
                                                const PGrid *__restrict__ grids, int mode, int *count, const int *__restrict__ start,
                                                int *fill, int *list, int *wide, int *nWide)
{
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= shape_faces(n_face, b, F)) return;
    float fc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fc[k] = face[((size_t)b * F + f) * 9 + k];
    if (!face_finite(fc)) return;
    const PGrid g = grids[b];
    int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    bool binned = face_binned(fc);
    if (binned) {
        const float pad = 1e-5f * g.scale;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float l = fminf(fc[k], fminf(fc[3 + k], fc[6 + k])), h = fmaxf(fc[k], fmaxf(fc[3 + k], fc[6 + k]));
            c0[k] = grid_cell(l - pad, g.o[k], g.inv[k], g.g[k]);
            c1[k] = grid_cell(h + pad, g.o[k], g.inv[k], g.g[k]);
        }
        binned = (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1) <= kPMaxCells;
    }
    if (!binned) {
        if (mode == 0) wide[(size_t)b * F + atomicAdd(&nWide[b], 1)] = f;
        return;
    }
    const size_t cb = (size_t)b * kPCells;
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const size_t c = cb + ((size_t)z * kPGMax + y) * kPGMax + x;
                if (mode == 0) atomicAdd(&count[c], 1);
                else list[start[c] + atomicAdd(&fill[c], 1)] = f;
            }
}

__device__ __forceinline__ void visit_cell(const float *__restrict__ fb, const int *__restrict__ list, int s, int n, const float *p, float &best,
                                           int &bf, int &bt)
{
    for (int i = s; i < s + n; ++i) {
        const int f = list[i];
        float fc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) fc[k] = fb[(size_t)f * 9 + k];
        int t;
        const float d = tri_dist(fc, fc + 3, fc + 6, p, &t);
        take(d, f, t, best, bf, bt);
    }
}

__global__ __launch_bounds__(256) void k_pm_query(const float *__restrict__ pts, const float *__restrict__ face, int P, int F,
                                                  const PGrid *__restrict__ grids, const int *__restrict__ count,
                                                  const int *__restrict__ start, const int *__restrict__ list, const int *__restrict__ wide,
                                                  const int *__restrict__ nWide, float *dist, long long *fidx, int *dtype)
{
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    const float *pp = pts + ((size_t)b * P + q) * 3;
    const float p[3] = {pp[0], pp[1], pp[2]};
    const float *__restrict__ fb = face + (size_t)b * F * 9;
    float best = INFINITY;
    int bf = -1, bt = -1;
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
        const int nw = nWide[b];
        for (int i = 0; i < nw; ++i) {
            const int f = wide[(size_t)b * F + i];
            float fc[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) fc[k] = fb[(size_t)f * 9 + k];
            int t;
            const float d = tri_dist(fc, fc + 3, fc + 6, p, &t);
            take(d, f, t, best, bf, bt);
        }
        const PGrid g = grids[b];
        if (g.any) {
            int c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = grid_cell(p[k], g.o[k], g.inv[k], g.g[k]);
            const float margin = kPMargin * (g.scale + fmaxf(fabsf(p[0]), fmaxf(fabsf(p[1]), fabsf(p[2]))));
            const int *cnt = count + (size_t)b * kPCells, *st = start + (size_t)b * kPCells;
            for (int r = 0;; ++r) {
                const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.g[2] - 1);
                const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.g[1] - 1);
                for (int z = z0; z <= z1; ++z)
                    for (int y = y0; y <= y1; ++y) {
                        const bool ring = z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r;
                        const int row = (z * kPGMax + y) * kPGMax;
                        if (ring) {
                            for (int x = max(c[0] - r, 0); x <= min(c[0] + r, g.g[0] - 1); ++x) visit_cell(fb, list, st[row + x], cnt[row + x], p, best, bf, bt);
                        } else {
                            if (c[0] - r >= 0) visit_cell(fb, list, st[row + c[0] - r], cnt[row + c[0] - r], p, best, bf, bt);
                            if (r > 0 && c[0] + r < g.g[0]) visit_cell(fb, list, st[row + c[0] + r], cnt[row + c[0] + r], p, best, bf, bt);
                        }
                    }
                // every face not yet seen lies in cells outside the box [c - r, c + r]: at least `gap` away from p
                float gap = INFINITY;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (c[k] - r > 0) gap = fminf(gap, p[k] - (g.o[k] + (float)(c[k] - r) * g.cs[k]));
                    if (c[k] + r < g.g[k] - 1) gap = fminf(gap, (g.o[k] + (float)(c[k] + r + 1) * g.cs[k]) - p[k]);
                }
                if (gap == INFINITY) break;                              // the box covers the grid
                const float lb = gap - margin;
                if (lb > 0.f && lb * lb > best) break;
            }
        }
    }
    write_result(b, q, P, p, best, bf, bt, dist, fidx, dtype);
}

// ---------------------------------------------------------------------------- area-weighted sampling
constexpr float kQuantScale = 16777216.0f;   // 2^24: the largest face of a shape gets 2^24 tickets

__device__ __forceinline__ float face_area(const float *fc)
{
    const float e1x = fc[3] - fc[0], e1y = fc[4] - fc[1], e1z = fc[5] - fc[2];
    const float e2x = fc[6] - fc[0], e2y = fc[7] - fc[1], e2z = fc[8] - fc[2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    return 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
}

// a[b,f] = the face's area (or the caller's), 0 beyond n_face and for non-finite or non-positive areas; amax[b] = its maximum
__global__ __launch_bounds__(256) void k_samp_area(const float *__restrict__ face, const float *__restrict__ areas, const int *__restrict__ n_face,
                                                   int F, float *a, unsigned *amax)
{
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float v = 0.f;
    if (f < shape_faces(n_face, b, F)) {
        if (areas) v = areas[(size_t)b * F + f];
        else {
            float fc[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) fc[k] = face[((size_t)b * F + f) * 9 + k];
            v = face_area(fc);
        }
        if (!(isfinite(v) && v > 0.f)) v = 0.f;
    }
    a[(size_t)b * F + f] = v;
    if (v > 0.f) atomicMax(&amax[b], __float_as_uint(v));         // non-negative floats order as their bits
}

__global__ __launch_bounds__(256) void k_samp_quant(const float *__restrict__ a, const unsigned *__restrict__ amax, int F, long long *tickets)
{
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float m = __uint_as_float(amax[b]);
    const float v = a[(size_t)b * F + f];
    long long t = 0;
    if (v > 0.f) {
        const float s = kQuantScale / m;
        t = (long long)(v * s);
        if (t < 1) t = 1;
    }
    tickets[(size_t)b * F + f] = t;
}

// cum: inclusive scan of the tickets over the flat [B,F] array; shape b's CDF is cum[b,f] - cum[b-1,F-1]
__global__ __launch_bounds__(256) void k_samp_points(const float *__restrict__ face, const long long *__restrict__ cum, const float *__restrict__ u,
                                                     int F, int N, float *out, long long *choice, int *empty)
{
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const size_t o = (size_t)b * N + j;
    const long long base = (b > 0 && F > 0) ? cum[(size_t)b * F - 1] : 0;
    const long long T = F > 0 ? cum[(size_t)b * F + F - 1] - base : 0;
    if (T <= 0) {
        out[o * 3] = NAN; out[o * 3 + 1] = NAN; out[o * 3 + 2] = NAN;
        choice[o] = -1;
        empty[b] = 1;
        return;
    }
    const float u0 = u[o * 3], u1 = u[o * 3 + 1], u2 = u[o * 3 + 2];
    long long t;
    if (!(u0 > 0.f)) t = 0;
    else if (u0 >= 1.f) t = T - 1;
    else {
        t = (long long)floor((double)u0 * (double)T);
        if (t > T - 1) t = T - 1;
    }
    const long long *cb = cum + (size_t)b * F;
    int lo = 0, hi = F - 1;                                           // first f with cb[f] - base > t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cb[mid] - base > t) hi = mid; else lo = mid + 1;
    }
    const float *fc = face + ((size_t)b * F + lo) * 9;
    const float s = sqrtf(u1);
    const float wa = 1.0f - s, wb = s * (1.0f - u2), wc = s * u2;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[o * 3 + k] = (wa * fc[k] + wb * fc[3 + k]) + wc * fc[6 + k];
    choice[o] = lo;
}

// ---------------------------------------------------------------------------- sided distance at an index
__device__ __forceinline__ float nn_dist(const float *q, const float *pts, int M, int i)
{   // A10's k_nn: d = 0; d += dx*dx; d += dy*dy; d += dz*dz, dx = point - query
    if (i < 0 || i >= M) return NAN;
    const float dx = pts[(size_t)i * 3] - q[0], dy = pts[(size_t)i * 3 + 1] - q[1], dz = pts[(size_t)i * 3 + 2] - q[2];
    float d = 0.f;
    d += dx * dx;
    d += dy * dy;
    d += dz * dz;
    return d;
}

__global__ __launch_bounds__(256) void k_nn_dist(const float *__restrict__ queries, const float *__restrict__ points, const int *__restrict__ idx,
                                                 int N, int M, float *dist, long long *idx64)
{
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    if (q >= N) return;
    const size_t o = (size_t)b * N + q;
    const int i = idx[o];
    dist[o] = nn_dist(queries + o * 3, points + (size_t)b * M * 3, M, i);
    if (idx64) idx64[o] = i;
}

// ---------------------------------------------------------------------------- fused metric reduction
constexpr int kMParts = 64;
constexpr int kMVals = 11;      // s1 s2 l1a l1b le1 gt1 le2 gt2 hsum hmaxa hmaxb
constexpr float kEsp = 1e-15f;  // utils/point_cloud_utils.py `esp`, added in fp32

__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }   // NaN sticks, as torch.max

__device__ __forceinline__ void side(const float *__restrict__ p, const float *__restrict__ o, const int *__restrict__ idx, int N, int M,
                                     int i, float r, float &s, float &l1, float &le, float &gt)
{
    const float *q = p + (size_t)i * 3;
    const int j = idx[i];
    const float d = nn_dist(q, o, M, j);
    const float sd = sqrtf(d + kEsp);
    s += sd;
    if (sd <= r) le += 1.f;
    if (sd > r) gt += 1.f;
    if (j >= 0 && j < M) {
        const float *w = o + (size_t)j * 3;
        l1 += (fabsf(q[0] - w[0]) + fabsf(q[1] - w[1])) + fabsf(q[2] - w[2]);
    } else l1 += NAN;
}

// block k of shape b reduces the k-th contiguous chunk of each array: per thread in index order, then the wave tree, then the
// four waves in fixed order
__global__ __launch_bounds__(256) void k_met_partial(const float *__restrict__ p1, const float *__restrict__ p2, const int *__restrict__ idx12,
                                                     const int *__restrict__ idx21, const float *__restrict__ da, const float *__restrict__ db,
                                                     int N1, int N2, int Nh, float radius, float *part)
{
    __shared__ float sh[4][kMVals];
    const int b = blockIdx.y, k = blockIdx.x;
    p1 += (size_t)b * N1 * 3; p2 += (size_t)b * N2 * 3; idx12 += (size_t)b * N1; idx21 += (size_t)b * N2;
    float v[kMVals];
#pragma unroll
    for (int i = 0; i < kMVals; ++i) v[i] = 0.f;
    v[9] = v[10] = -INFINITY;
    const int c1 = (N1 + kMParts - 1) / kMParts, c2 = (N2 + kMParts - 1) / kMParts, ch = (Nh + kMParts - 1) / kMParts;
    for (int i = k * c1 + threadIdx.x; i < min(N1, (k + 1) * c1); i += 256) side(p1, p2, idx12, N1, N2, i, radius, v[0], v[2], v[4], v[5]);
    for (int i = k * c2 + threadIdx.x; i < min(N2, (k + 1) * c2); i += 256) side(p2, p1, idx21, N2, N1, i, radius, v[1], v[3], v[6], v[7]);
    if (da && db)
        for (int i = k * ch + threadIdx.x; i < min(Nh, (k + 1) * ch); i += 256) {
            const float sa = sqrtf(da[(size_t)b * Nh + i] + kEsp), sb = sqrtf(db[(size_t)b * Nh + i] + kEsp);
            v[8] += (sa + sb) / 2.0f;
            v[9] = nanmax(v[9], sa);
            v[10] = nanmax(v[10], sb);
        }
#pragma unroll  // wave_sum's order (wave.hpp) with nanmax beside it; written out, a call changes this kernel's instruction stream
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 9; ++i) v[i] += __shfl_xor(v[i], off);
        v[9] = nanmax(v[9], __shfl_xor(v[9], off));
        v[10] = nanmax(v[10], __shfl_xor(v[10], off));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < kMVals; ++i) sh[w][i] = v[i];
    __syncthreads();
    if (threadIdx.x < kMVals) {
        const int i = threadIdx.x;
        const float r = i < 9 ? (sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]) : nanmax(nanmax(sh[0][i], sh[1][i]), nanmax(sh[2][i], sh[3][i]));
        part[((size_t)b * kMParts + k) * kMVals + i] = r;
    }
}

// out [B,5]: chamfer, chamfer_l1, f_score, mean_hausdorff, max_hausdorff (the last two NaN without point-to-mesh distances)
__global__ __launch_bounds__(64) void k_met_final(const float *__restrict__ part, int N1, int N2, int Nh, int have_h, float *out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    float v[kMVals];
#pragma unroll
    for (int i = 0; i < kMVals; ++i) v[i] = part[((size_t)b * kMParts + lane) * kMVals + i];
#pragma unroll  // wave_sum's order (wave.hpp) with nanmax beside it; written out, a call changes this kernel's instruction stream
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 9; ++i) v[i] += __shfl_xor(v[i], off);
        v[9] = nanmax(v[9], __shfl_xor(v[9], off));
        v[10] = nanmax(v[10], __shfl_xor(v[10], off));
    }
    if (lane == 0) {
        const float m1 = v[0] / (float)N1, m2 = v[1] / (float)N2;
        const float precision = v[6] / (v[6] + v[7]), recall = v[4] / (v[4] + v[5]);
        out[b * 5 + 0] = (m1 + m2) / 2.0f;
        out[b * 5 + 1] = v[2] / (float)N1 + v[3] / (float)N2;
        out[b * 5 + 2] = 2.0f * (precision * recall) / ((precision + recall) + 1e-8f);
        out[b * 5 + 3] = have_h ? v[8] / (float)Nh : NAN;
        out[b * 5 + 4] = have_h ? (v[9] + v[10]) / 2.0f : NAN;
    }
}

struct PMSlices {
    PGrid *grids; float *part; int *count, *start, *fill, *nWide, *wide, *list; void *scan_ws; size_t scan_bytes;
};
static size_t pm_layout(int B, int F, void *base, PMSlices *s)
{
    Arena ar(base);
    const size_t nc = (size_t)B * kPCells;
    PMSlices t;
    t.grids = ar.take<PGrid>(B);
    t.part = ar.take<float>((size_t)B * kPParts * 8);
    t.count = ar.take<int>(nc);
    t.start = ar.take<int>(nc);
    t.fill = ar.take<int>(nc);
    t.nWide = ar.take<int>(B);
    t.wide = ar.take<int>((size_t)B * F);
    t.list = ar.take<int>((size_t)B * F * kPMaxCells);
    t.scan_bytes = deftet_scan_workspace_bytes((long long)nc, 4);
    t.scan_ws = ar.take<char>(t.scan_bytes);
    if (s) *s = t;
    return ar.off + 256;
}

// areas, their quantised tickets (scanned in place), the largest area per shape
struct SampLayout {
    float *a; long long *cum; unsigned *amax; void *scan_ws; size_t scan_bytes, bytes;
};
static SampLayout samp_layout(int B, int F, void *base)
{
    SampLayout L{};
    Arena ar(base);
    const size_t n = (size_t)B * F;
    L.a = ar.take<float>(n);
    L.cum = ar.take<long long>(n);
    L.amax = ar.take<unsigned>(B);
    L.scan_bytes = deftet_scan_workspace_bytes((long long)n, 8);
    L.scan_ws = ar.take<char>(L.scan_bytes);
    L.bytes = ar.end();
    return L;
}

}  // namespace met
}  // namespace deftet

using namespace deftet;

static int pm_check(const float *pts, const float *face, const int32_t *n_face, int B, int P, int F, float *dist, int64_t *face_idx,
                    int32_t *dist_type)
{
    DEFTET_CHECK_ARG(B >= 0 && P >= 0 && F >= 0 && B <= 65535, "bad size (B=%d, P=%d, F=%d)", B, P, F);
    DEFTET_CHECK_ARG(F <= (1 << 24) && (long long)B * F <= (1LL << 26) && P <= (1 << 28), "too many faces or points (B=%d, P=%d, F=%d)", B, P, F);
    if (B == 0 || P == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(pts && dist && face_idx && dist_type && (F == 0 || face), "null pointer");
    DEFTET_CHECK_ARG(aligned(pts, 4) && aligned(face, 4) && aligned(n_face, 4) && aligned(dist, 4) &&
                         aligned(face_idx, 8) && aligned(dist_type, 4),
                     "misaligned pointer");
    return DEFTET_OK;
}

extern "C" size_t deftet_point_mesh_distance_workspace_bytes(int n_batch, int n_point, int n_face)
{
    if (n_batch < 0 || n_point < 0 || n_face < 0) return 0;
    return met::pm_layout(n_batch, n_face, nullptr, nullptr);
}

extern "C" int deftet_point_mesh_distance_f32(const float *pts, const float *face, const int32_t *n_face, int B, int P, int F, float *dist,
                                              int64_t *face_idx, int32_t *dist_type, void *workspace, size_t workspace_bytes, void *stream_)
{
    const int rc = pm_check(pts, face, n_face, B, P, F, dist, face_idx, dist_type);
    if (rc != DEFTET_OK || B == 0 || P == 0) return rc;
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, deftet_point_mesh_distance_workspace_bytes(B, P, F)));
    hipStream_t st = as_stream(stream_);
    met::PMSlices s;
    met::pm_layout(B, F, workspace, &s);
    const size_t nc = (size_t)B * met::kPCells;
    DEFTET_HIP(hipMemsetAsync(s.count, 0, nc * 4, st));
    DEFTET_HIP(hipMemsetAsync(s.fill, 0, nc * 4, st));
    DEFTET_HIP(hipMemsetAsync(s.nWide, 0, (size_t)B * 4, st));
    const float *fc = F > 0 ? face : pts;                          // never read without faces
    const int *nf = (const int *)n_face;
    DEFTET_LAUNCH(met::k_pm_stats, dim3(met::kPParts, B), dim3(256), st, fc, nf, F, s.part);
    DEFTET_LAUNCH(met::k_pm_grid, dim3(B), dim3(64), st, s.part, s.grids);
    if (F > 0) {
        const dim3 fg(blocks_for(F, 256), B);
        DEFTET_LAUNCH(met::k_pm_bin, fg, dim3(256), st, fc, nf, F, s.grids, 0, s.count, s.start, s.fill, s.list, s.wide, s.nWide);
        const int src = deftet_scan(s.count, s.start, (long long)nc, 4, 0, s.scan_ws, s.scan_bytes, stream_);
        if (src != DEFTET_OK) return src;
        DEFTET_LAUNCH(met::k_pm_bin, fg, dim3(256), st, fc, nf, F, s.grids, 1, s.count, s.start, s.fill, s.list, s.wide, s.nWide);
    }
    DEFTET_LAUNCH(met::k_pm_query, dim3(blocks_for(P, 256), B), dim3(256), st, pts, fc, P, F, s.grids, s.count, s.start, s.list, s.wide,
                  s.nWide, dist, (long long *)face_idx, (int *)dist_type);
    return DEFTET_OK;
}

extern "C" int deftet_point_mesh_distance_scan_f32(const float *pts, const float *face, const int32_t *n_face, int B, int P, int F,
                                                   float *dist, int64_t *face_idx, int32_t *dist_type, void *stream_)
{
    const int rc = pm_check(pts, face, n_face, B, P, F, dist, face_idx, dist_type);
    if (rc != DEFTET_OK || B == 0 || P == 0) return rc;
    DEFTET_LAUNCH(met::k_pm_scan, dim3(blocks_for(P, 256), B), dim3(256), as_stream(stream_), pts, F > 0 ? face : pts, (const int *)n_face, P,
                  F, dist, (long long *)face_idx, (int *)dist_type);
    return DEFTET_OK;
}

extern "C" size_t deftet_sample_points_workspace_bytes(int n_batch, int n_face)
{
    return n_batch < 0 || n_face < 0 ? 0 : met::samp_layout(n_batch, n_face, nullptr).bytes;
}

extern "C" int deftet_sample_points_f32(const float *face, const float *areas, const int32_t *n_face, const float *uniforms, int B, int F,
                                        int N, float *points, int64_t *face_choice, int32_t *empty_flag, void *workspace,
                                        size_t workspace_bytes, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && F >= 0 && N >= 0 && B <= 65535 && (long long)B * F <= (1LL << 30), "bad size (B=%d, F=%d, N=%d)", B, F, N);
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(empty_flag && (N == 0 || (uniforms && points && face_choice)) && (F == 0 || face), "null pointer");
    DEFTET_CHECK_ARG(aligned(face, 4) && aligned(areas, 4) && aligned(n_face, 4) && aligned(uniforms, 4) &&
                         aligned(points, 4) && aligned(face_choice, 8) && aligned(empty_flag, 4),
                     "misaligned pointer");
    const met::SampLayout L = met::samp_layout(B, F, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    hipStream_t st = as_stream(stream_);
    const size_t n = (size_t)B * F;
    DEFTET_HIP(hipMemsetAsync(empty_flag, 0, (size_t)B * 4, st));
    DEFTET_HIP(hipMemsetAsync(L.amax, 0, (size_t)B * 4, st));
    if (F > 0) {
        const dim3 fg(blocks_for(F, 256), B);
        DEFTET_LAUNCH(met::k_samp_area, fg, dim3(256), st, face, areas, (const int *)n_face, F, L.a, L.amax);
        DEFTET_LAUNCH(met::k_samp_quant, fg, dim3(256), st, L.a, L.amax, F, L.cum);
        const int src = deftet_scan(L.cum, L.cum, (long long)n, 8, 1, L.scan_ws, L.scan_bytes, stream_);
        if (src != DEFTET_OK) return src;
    }
    if (N > 0)
        DEFTET_LAUNCH(met::k_samp_points, dim3(blocks_for(N, 256), B), dim3(256), st, F > 0 ? face : uniforms, L.cum, uniforms, F, N, points,
                      (long long *)face_choice, (int *)empty_flag);
    return DEFTET_OK;
}

extern "C" int deftet_nn_distance_f32(const float *queries, const float *points, const int32_t *idx, int B, int N, int M, float *dist,
                                      int64_t *idx64, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && N >= 0 && M >= 0 && B <= 65535, "bad size (B=%d, N=%d, M=%d)", B, N, M);
    if (B == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(queries && idx && dist && (M == 0 || points), "null pointer");
    DEFTET_CHECK_ARG(aligned(queries, 4) && aligned(points, 4) && aligned(idx, 4) && aligned(dist, 4) &&
                         aligned(idx64, 8),
                     "misaligned pointer");
    DEFTET_LAUNCH(met::k_nn_dist, dim3(blocks_for(N, 256), B), dim3(256), as_stream(stream_), queries, M > 0 ? points : queries,
                  (const int *)idx, N, M, dist, (long long *)idx64);
    return DEFTET_OK;
}

extern "C" size_t deftet_surface_metrics_workspace_bytes(int n_batch)
{
    if (n_batch < 0) return 0;
    return align_up((size_t)n_batch * met::kMParts * met::kMVals * 4, 256);
}

extern "C" int deftet_surface_metrics_f32(const float *p1, const float *p2, const int32_t *idx12, const int32_t *idx21, const float *dist_a,
                                          const float *dist_b, int B, int N1, int N2, int Nh, float radius, float *out, void *workspace,
                                          size_t workspace_bytes, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && N1 > 0 && N2 > 0 && Nh >= 0 && B <= 65535 && N1 <= (1 << 24) && N2 <= (1 << 24) && Nh <= (1 << 24),
                     "bad size (B=%d, N1=%d, N2=%d, Nh=%d)", B, N1, N2, Nh);
    DEFTET_CHECK_ARG((dist_a == nullptr) == (dist_b == nullptr), "dist_a and dist_b: both or neither");
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(p1 && p2 && idx12 && idx21 && out, "null pointer");
    DEFTET_CHECK_ARG(aligned(p1, 4) && aligned(p2, 4) && aligned(idx12, 4) && aligned(idx21, 4) &&
                         aligned(dist_a, 4) && aligned(dist_b, 4) && aligned(out, 4),
                     "misaligned pointer");
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, deftet_surface_metrics_workspace_bytes(B)));
    hipStream_t st = as_stream(stream_);
    float *part = static_cast<float *>(workspace);
    const int have_h = dist_a != nullptr && Nh > 0;
    DEFTET_LAUNCH(met::k_met_partial, dim3(met::kMParts, B), dim3(256), st, p1, p2, (const int *)idx12, (const int *)idx21,
                  have_h ? dist_a : nullptr, have_h ? dist_b : nullptr, N1, N2, Nh, radius, part);
    DEFTET_LAUNCH(met::k_met_final, dim3(B), dim3(64), st, part, N1, N2, Nh, have_h, out);
    return DEFTET_OK;
}
