// winding_number.hip — generalised winding number of a triangle mesh about query points (Jacobson et al. 2013): the sum over the
// faces of the signed solid angle, over 4 pi.  An integer on a closed, consistently oriented mesh (the number of times the surface
// wraps the point), smooth across holes, additive over nested and intersecting parts — the inside test for meshes on which the ray
// parity of check_sign.hip is noise.  DESIGN.md §6q.
//
// The term (Van Oosterom-Strackee; a, b, c the corners minus the point):
//     2 atan2(det(a,b,c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
//
// Two paths behind one entry point, both without a float atomic and with a per-point summation order that depends on nothing but
// the point and the mesh:
//  * DEFTET_WN_EXACT — every point against every face in face order; one point per lane, the 48-byte face records are
//    wave-uniform and come through the scalar cache (as k_brute of check_sign.hip).
//  * DEFTET_WN_FAST — a dense octree of depth L(F) <= 5 over the box of the mesh.  Faces are sorted by the Morton code of the leaf
//    their centroid falls in (prims.hpp, stable: face order inside a leaf); a leaf's node is a segmented reduction over its run of
//    faces, every level above is made from its eight children in child order.  A node holds the summed area vector, the summed area,
//    an area-weighted centre and a radius that covers every corner of every face below it.  A query walks the tree top-down, the
//    WAVE at once: a node is opened when any lane needs it (ballot); a lane whose point is farther than beta radii from the centre
//    takes the dipole N.d / (4 pi |d|^3) there and sits out the subtree (one bit per level in a lane-private mask); an opened leaf
//    evaluates its faces exactly.  Level and node index are wave-uniform, so node records and leaf faces are scalar loads.  Which
//    nodes the wave VISITS depends on its 64 points, which terms a lane ADDS depends on its own point only, and it adds them in the
//    depth-first order, so a point's value does not depend on its wave.  To make waves coherent the points are first sorted by the
//    leaf they fall in (DEFTET_WN_FAST_UNSORTED leaves that out: for the
//    measurement of what the sort is worth, and the tests' second assignment of points to waves).
//
// Per-lane sums are compensated (Kahan) in fp32 on both paths: the term count goes from a few hundred (fast) to the face count
// (exact, 10^5 and more), and a plain fp32 sum of F terms of either sign drifts by up to F u times the largest partial sum — at
// 10^5 faces that alone is of the order of the 1e-3 the integer reading of the result can bear.  The compensation costs four adds
// beside an atan2 and makes the sum's own error O(u) at any F; what is left is the rounding of the single terms.
//
// Bad input is counted, never read: a face with an index outside its mesh or with a non-finite corner gets a zero record, is
// counted in bad[0] / bad[1] and turns every value of its SHAPE into NaN; a non-finite point is counted in bad[2] and gets NaN.
#include <math.h>

#include "cell_gather.hpp"
#include "grid_setup.hpp"
#include "prims.hpp"

#include "common.hpp"

namespace deftet {
namespace wn {

constexpr int kMaxL = 5;                    // 8^5 leaves, 37,449 nodes of 32 bytes: 1.2 MB per shape, inside one XCD's 4 MB L2
constexpr int kParts = 64;                  // box partials per shape
constexpr float kInv2Pi = 0.15915494309189535f;
constexpr float kInv4Pi = 0.07957747154594767f;
constexpr float kBetaDefault = 3.0f;        // measured, E0 of tests/winding_ref.py
constexpr float kFltMax = 3.402823466e+38f;
// AUTO takes the tree from kAutoFastFaces faces on, and from kAutoFastFacesMany on when there are kAutoManyPoints points or more
// (measured, DESIGN.md §6q: at 48 faces the exact path wins at 4,096 and at 2 M points, at 120 faces it wins at 4,096 points only, at
// 224 faces and above the tree wins at both)
constexpr int kAutoFastFaces = 200, kAutoFastFacesMany = 100;
constexpr long long kAutoManyPoints = 1 << 20;

// depth of the tree of a mesh of F faces: floor((floor(log2 F) - 2) / 2) in [0, kMaxL] — a leaf holds a handful of faces of a
// surface (a surface meets ~4^L of the 8^L leaves).  The same function sizes the workspace on the host and picks the per-shape
// depth of a ragged batch on the device.
__host__ __device__ inline int pick_L(int F)
{
    int lg = 0;
    while (lg < 30 && (F >> (lg + 1)) > 0) ++lg;
    int L = (lg - 2) / 2;
    return L < 0 ? 0 : (L > kMaxL ? kMaxL : L);
}
__host__ __device__ inline unsigned lvl_off(int l) { return ((1u << (3 * l)) - 1u) / 7u; }     // nodes above level l

struct Mesh {
    long long vBase, fBase;
    int V, F;
};
// uniform batches: V and F per shape, one face list shared by all shapes; ragged ones: offsets into concatenated arrays.  Records
// are per shape in both (the vertices differ), shape b's at fBase for ragged and at b F for uniform batches.
__device__ __forceinline__ Mesh mesh_of(int b, int V, int F, const int *__restrict__ vOff, const int *__restrict__ fOff, long long &rBase)
{
    Mesh m;
    if (fOff) {
        m.vBase = vOff ? vOff[b] : 0; m.V = vOff ? vOff[b + 1] - vOff[b] : 0;
        m.fBase = fOff[b]; m.F = fOff[b + 1] - fOff[b];
        rBase = m.fBase;
    } else {
        m.vBase = (long long)b * V; m.V = V;
        m.fBase = 0; m.F = F;
        rBase = (long long)b * F;
    }
    return m;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) <= kFltMax && fabsf(y) <= kFltMax && fabsf(z) <= kFltMax; }

// sum += t, compensated
__device__ __forceinline__ void kahan(float &sum, float &comp, float t)
{
    const float y = t - comp;
    const float s = sum + y;
    comp = (s - sum) - y;
    sum = s;
}

// the solid angle of the face (r0.xyz | r0.w r1.xy | r1.zw r2.x) seen from p, over 4 pi
__device__ __forceinline__ float face_term(const float4 r0, const float4 r1, const float4 r2, float px, float py, float pz)
{
    const float ax = r0.x - px, ay = r0.y - py, az = r0.z - pz;
    const float bx = r0.w - px, by = r1.x - py, bz = r1.y - pz;
    const float cx = r1.z - px, cy = r1.w - py, cz = r2.x - pz;
    const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
    const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
    const float den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb;
    return atan2f(det, den) * kInv2Pi;
}

// face records (three corners, 48 bytes; zeros for a bad face) and, for the tree, the box of the corners per block
__global__ __launch_bounds__(256) void k_wn_prep(const float *__restrict__ verts, const long long *__restrict__ faces, int V, int F,
                                                 float4 *rec, float *part, int *bad, int *shapeBad, const int *__restrict__ vOff,
                                                 const int *__restrict__ fOff)
{
    __shared__ float sh[4][6];
    const int b = blockIdx.y;
    long long rBase;
    const Mesh M = mesh_of(b, V, F, vOff, fOff, rBase);
    const float *vb = verts + (size_t)M.vBase * 3;
    const long long *fb = faces + (size_t)M.fBase * 3;
    BoxStats<3, 0> bs;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < M.F; k += gridDim.x * blockDim.x) {
        const long long i0 = fb[(size_t)k * 3], i1 = fb[(size_t)k * 3 + 1], i2 = fb[(size_t)k * 3 + 2];
        float a[3] = {0.f, 0.f, 0.f}, c1[3] = {0.f, 0.f, 0.f}, c2[3] = {0.f, 0.f, 0.f};
        if (i0 < 0 || i0 >= M.V || i1 < 0 || i1 >= M.V || i2 < 0 || i2 >= M.V) {      // no vertex is read
            atomicAdd(&bad[0], 1);
            shapeBad[b] = 1;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) { a[c] = vb[i0 * 3 + c]; c1[c] = vb[i1 * 3 + c]; c2[c] = vb[i2 * 3 + c]; }
            if (!(finite3(a[0], a[1], a[2]) && finite3(c1[0], c1[1], c1[2]) && finite3(c2[0], c2[1], c2[2]))) {
                atomicAdd(&bad[1], 1);
                shapeBad[b] = 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = c1[c] = c2[c] = 0.f;
            } else {
                bs.add_point(a);
                bs.add_point(c1);
                bs.add_point(c2);
            }
        }
        float4 *r = rec + ((size_t)rBase + k) * 3;
        r[0] = make_float4(a[0], a[1], a[2], c1[0]);
        r[1] = make_float4(c1[1], c1[2], c2[0], c2[1]);
        r[2] = make_float4(c2[2], 0.f, 0.f, 0.f);
    }
    if (!part) return;                                               // (uniform: the exact path keeps no box)
    bs.block_store(sh, part + ((size_t)b * kParts + blockIdx.x) * 6);
}

// one wave per shape: the box -> origin and inverse cell size per axis for the shape's own 2^L grid; dom[b] = ox oy oz ix iy iz, lvl[b] = L
__global__ __launch_bounds__(64) void k_wn_dom(const float *__restrict__ part, int nPart, int F, int Lmax, const int *__restrict__ fOff,
                                               float *dom, int *lvl)
{
    const int b = blockIdx.x;
    const int Fb = fOff ? fOff[b + 1] - fOff[b] : F;
    const int L = min(pick_L(Fb), Lmax);                             // (Lmax is what the node arrays are sized for)
    BoxStats<3, 0> bs;
    bs.load_reduce(part + (size_t)b * kParts * 6, nPart);
    if (threadIdx.x == 0) {
        const float G = (float)(1 << L);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool ok = bs.hi[k] >= bs.lo[k];
            const float w = ok ? bs.hi[k] - bs.lo[k] : 0.f;
            dom[b * 6 + k] = ok ? bs.lo[k] : 0.f;
            dom[b * 6 + 3 + k] = w > 1e-30f ? G / w : 0.f;
        }
        lvl[b] = L;
    }
}

__device__ __forceinline__ unsigned spread3(unsigned x)              // 5 bits -> every third bit
{
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
// Morton code of the leaf of (x, y, z) in shape b's grid (x in the lowest bit of every triple); points outside the box are clamped in
__device__ __forceinline__ unsigned leaf_of(float x, float y, float z, const float *__restrict__ dom, int L)
{
    const int G = 1 << L;
    const unsigned cx = (unsigned)grid_cell(x, dom[0], dom[3], G), cy = (unsigned)grid_cell(y, dom[1], dom[4], G),
                   cz = (unsigned)grid_cell(z, dom[2], dom[5], G);
    return spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2);
}

// key of a face: shape-major, then the leaf of its centroid
__global__ __launch_bounds__(256) void k_wn_face_keys(const float4 *__restrict__ rec, int F, const int *__restrict__ fOff,
                                                      const float *__restrict__ dom, const int *__restrict__ lvl, unsigned nLeafMax, unsigned *keys)
{
    const int b = blockIdx.y;
    long long rBase;
    const Mesh M = mesh_of(b, 0, F, nullptr, fOff, rBase);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M.F) return;
    const float4 *r = rec + ((size_t)rBase + k) * 3;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
    const float third = 1.0f / 3.0f;
    const float gx = ((r0.x + r0.w) + r1.z) * third, gy = ((r0.y + r1.x) + r1.w) * third, gz = ((r0.z + r1.y) + r2.x) * third;
    keys[(size_t)rBase + k] = (unsigned)b * nLeafMax + leaf_of(gx, gy, gz, dom + b * 6, lvl[b]);
}

// records in sorted order: a leaf's faces are one run
__global__ __launch_bounds__(256) void k_wn_gather(const float4 *__restrict__ rec, const int32_t *__restrict__ perm, long long nRec, float4 *srec)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nRec) return;
    const float4 *r = rec + (size_t)perm[j] * 3;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
    srec[(size_t)j * 3] = r0;
    srec[(size_t)j * 3 + 1] = r1;
    srec[(size_t)j * 3 + 2] = r2;
}

// A node is two float4: (N.xyz, radius) (centre.xyz, area).  radius < 0: nothing below the node.
// Leaves: one thread per leaf over its run of faces, in run order (= face order: the sort is stable).
__global__ __launch_bounds__(256) void k_wn_leaves(const float4 *__restrict__ srec, const int32_t *__restrict__ seg, const int *__restrict__ lvl,
                                                   unsigned nLeafMax, unsigned nNodeMax, float4 *nodes)
{
    const int b = blockIdx.y;
    const int L = lvl[b];
    const unsigned m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (1u << (3 * L))) return;
    const int s = seg[(size_t)b * nLeafMax + m], e = seg[(size_t)b * nLeafMax + m + 1];
    float4 *out = nodes + ((size_t)b * nNodeMax + lvl_off(L) + m) * 2;
    if (e <= s) {
        out[0] = make_float4(0.f, 0.f, 0.f, -1.f);
        out[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float nx = 0.f, ny = 0.f, nz = 0.f, A = 0.f, wx = 0.f, wy = 0.f, wz = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    const float third = 1.0f / 3.0f;
    for (int j = s; j < e; ++j) {
        const float4 r0 = srec[(size_t)j * 3], r1 = srec[(size_t)j * 3 + 1], r2 = srec[(size_t)j * 3 + 2];
        const float ux = r0.w - r0.x, uy = r1.x - r0.y, uz = r1.y - r0.z;
        const float vx = r1.z - r0.x, vy = r1.w - r0.y, vz = r2.x - r0.z;
        const float fx = 0.5f * (uy * vz - uz * vy), fy = 0.5f * (uz * vx - ux * vz), fz = 0.5f * (ux * vy - uy * vx);
        const float a = sqrtf(fx * fx + fy * fy + fz * fz);
        const float cx = ((r0.x + r0.w) + r1.z) * third, cy = ((r0.y + r1.x) + r1.w) * third, cz = ((r0.z + r1.y) + r2.x) * third;
        nx += fx; ny += fy; nz += fz;
        A += a;
        wx += a * cx; wy += a * cy; wz += a * cz;
        gx += cx; gy += cy; gz += cz;
    }
    float cx, cy, cz;
    if (A > 0.f) { cx = wx / A; cy = wy / A; cz = wz / A; }
    else { const float inv = 1.0f / (float)(e - s); cx = gx * inv; cy = gy * inv; cz = gz * inv; }
    float r2max = 0.f;
    for (int j = s; j < e; ++j) {
        const float4 r0 = srec[(size_t)j * 3], r1 = srec[(size_t)j * 3 + 1], r2 = srec[(size_t)j * 3 + 2];
        const float ax = r0.x - cx, ay = r0.y - cy, az = r0.z - cz;
        const float bx = r0.w - cx, by = r1.x - cy, bz = r1.y - cz;
        const float dx = r1.z - cx, dy = r1.w - cy, dz = r2.x - cz;
        r2max = fmaxf(r2max, fmaxf(ax * ax + ay * ay + az * az, fmaxf(bx * bx + by * by + bz * bz, dx * dx + dy * dy + dz * dz)));
    }
    out[0] = make_float4(nx, ny, nz, sqrtf(r2max));
    out[1] = make_float4(cx, cy, cz, A);
}

// level l from its eight children of level l + 1, in child order; shapes whose tree is not deeper than l do nothing
__global__ __launch_bounds__(256) void k_wn_up(int l, const int *__restrict__ lvl, unsigned nNodeMax, float4 *nodes)
{
    const int b = blockIdx.y;
    if (l >= lvl[b]) return;
    const unsigned m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (1u << (3 * l))) return;
    float4 *nb = nodes + (size_t)b * nNodeMax * 2;
    const float4 *ch = nb + ((size_t)lvl_off(l + 1) + 8u * m) * 2;
    float4 c0[8], c1[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { c0[c] = ch[c * 2]; c1[c] = ch[c * 2 + 1]; }
    float nx = 0.f, ny = 0.f, nz = 0.f, A = 0.f, wx = 0.f, wy = 0.f, wz = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c0[c].w < 0.f) continue;
        ++cnt;
        nx += c0[c].x; ny += c0[c].y; nz += c0[c].z;
        A += c1[c].w;
        wx += c1[c].w * c1[c].x; wy += c1[c].w * c1[c].y; wz += c1[c].w * c1[c].z;
        gx += c1[c].x; gy += c1[c].y; gz += c1[c].z;
    }
    float4 *out = nb + ((size_t)lvl_off(l) + m) * 2;
    if (cnt == 0) {
        out[0] = make_float4(0.f, 0.f, 0.f, -1.f);
        out[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float cx, cy, cz;
    if (A > 0.f) { cx = wx / A; cy = wy / A; cz = wz / A; }
    else { const float inv = 1.0f / (float)cnt; cx = gx * inv; cy = gy * inv; cz = gz * inv; }
    float rad = 0.f;                                                 // a child's ball lies inside |c_child - c| + r_child
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c0[c].w < 0.f) continue;
        const float dx = c1[c].x - cx, dy = c1[c].y - cy, dz = c1[c].z - cz;
        rad = fmaxf(rad, sqrtf(dx * dx + dy * dy + dz * dz) + c0[c].w);
    }
    out[0] = make_float4(nx, ny, nz, rad);
    out[1] = make_float4(cx, cy, cz, A);
}

// key of a point: its leaf in its shape's grid (clamped into the box), shape-major — every shape's N points stay one run of N
__global__ __launch_bounds__(256) void k_wn_point_keys(const float *__restrict__ points, int N, const float *__restrict__ dom,
                                                       const int *__restrict__ lvl, unsigned nLeafMax, unsigned *keys)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float *p = points + ((size_t)b * N + i) * 3;
    keys[(size_t)b * N + i] = (unsigned)b * nLeafMax + leaf_of(p[0], p[1], p[2], dom + b * 6, lvl[b]);
}

template <bool SORTED>
__global__ __launch_bounds__(256) void k_wn_query(const float *__restrict__ points, const float4 *__restrict__ srec,
                                                  const float4 *__restrict__ nodes, const int32_t *__restrict__ seg,
                                                  const int *__restrict__ lvl, const int *__restrict__ shapeBad,
                                                  const unsigned *__restrict__ pperm, int N, unsigned nLeafMax, unsigned nNodeMax, float beta2,
                                                  float *out, int *bad)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < N;
    size_t pid = (size_t)b * N + (live ? i : 0);
    if (SORTED) pid = pperm[pid];                                    // (a point of shape b: the keys are shape-major)
    const float px = points[pid * 3], py = points[pid * 3 + 1], pz = points[pid * 3 + 2];
    const bool fin = finite3(px, py, pz);
    const int L = lvl[b];
    const float4 *nb = nodes + (size_t)b * nNodeMax * 2;
    const int32_t *sg = seg + (size_t)b * nLeafMax;
    unsigned alive = live && fin ? 1u : 0u;                          // bit l: this lane walks the current subtree of level l
    float sum = 0.f, comp = 0.f;
    int l = 0;                                                       // l, m: wave-uniform (they move on ballots and on node records only)
    unsigned m = 0u;
    if (shapeBad[b] == 0 && __ballot(alive != 0u) != 0ull) {
        for (;;) {
            const float4 n0 = nb[((size_t)lvl_off(l) + m) * 2], n1 = nb[((size_t)lvl_off(l) + m) * 2 + 1];
            if (n0.w >= 0.f) {
                const bool mine = ((alive >> l) & 1u) != 0u;
                const float dx = n1.x - px, dy = n1.y - py, dz = n1.z - pz;
                const float d2 = dx * dx + dy * dy + dz * dz;
                const bool far = d2 > beta2 * (n0.w * n0.w);
                if (mine && far) kahan(sum, comp, (n0.x * dx + n0.y * dy + n0.z * dz) / (d2 * sqrtf(d2)) * kInv4Pi);
                const bool open = mine && !far;
                if (__ballot(open) != 0ull) {
                    if (l == L) {
                        const int s = sg[m], e = sg[m + 1];
                        for (int j = s; j < e; ++j) {
                            const float t = face_term(srec[(size_t)j * 3], srec[(size_t)j * 3 + 1], srec[(size_t)j * 3 + 2], px, py, pz);
                            if (open) kahan(sum, comp, t);
                        }
                    } else {
                        const unsigned bit = 2u << l;
                        alive = open ? (alive | bit) : (alive & ~bit);
                        ++l;
                        m <<= 3;
                        continue;
                    }
                }
            }
            while (l > 0 && (m & 7u) == 7u) { --l; m >>= 3; }
            if (l == 0) break;
            ++m;
        }
    }
    if (!live) return;
    if (!fin) atomicAdd(&bad[2], 1);
    out[pid] = (fin && shapeBad[b] == 0) ? sum : __int_as_float(0x7FC00000);
}

// every face, in face order; the records are wave-uniform
__global__ __launch_bounds__(256) void k_wn_exact(const float *__restrict__ points, const float4 *__restrict__ rec, int N, int F,
                                                  const int *__restrict__ fOff, const int *__restrict__ shapeBad, float *out, int *bad)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < N;
    long long rBase;
    const Mesh M = mesh_of(b, 0, F, nullptr, fOff, rBase);
    const size_t pid = (size_t)b * N + (live ? i : 0);
    const float px = points[pid * 3], py = points[pid * 3 + 1], pz = points[pid * 3 + 2];
    const bool fin = finite3(px, py, pz);
    const float4 *rb = rec + (size_t)rBase * 3;
    float sum = 0.f, comp = 0.f;
    if (shapeBad[b] == 0)
        for (int k = 0; k < M.F; ++k) kahan(sum, comp, face_term(rb[(size_t)k * 3], rb[(size_t)k * 3 + 1], rb[(size_t)k * 3 + 2], px, py, pz));
    if (!live) return;
    if (!fin) atomicAdd(&bad[2], 1);
    out[pid] = (fin && shapeBad[b] == 0) ? sum : __int_as_float(0x7FC00000);
}

// no face at all: 0, NaN for a non-finite point
__global__ __launch_bounds__(256) void k_wn_empty(const float *__restrict__ points, long long n, float *out, int *bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool fin = finite3(points[i * 3], points[i * 3 + 1], points[i * 3 + 2]);
    if (!fin) atomicAdd(&bad[2], 1);
    out[i] = fin ? 0.f : __int_as_float(0x7FC00000);
}

static int resolve(int algo, int Fmax, long long nPoint)
{
    if (algo != 0) return algo;
    return Fmax >= kAutoFastFaces || (Fmax >= kAutoFastFacesMany && nPoint >= kAutoManyPoints) ? 2 : 1;
}

struct Layout {
    int Lmax;
    unsigned nLeafMax, nNodeMax;
    size_t bytes;
    float4 *rec, *srec, *nodes;
    int *shapeBad, *lvl;
    float *part, *dom;
    SortBufs fs, ps;
    int32_t *fperm, *seg;
    unsigned *pperm;
};

// F: largest mesh, nRec: all faces of the batch, algo: resolved (1 exact, 2 fast, 3 fast without the point sort)
static Layout make_layout(int B, int F, long long nRec, int N, int algo, void *ws, size_t wsBytes)
{
    Layout L{};
    Arena A(ws, wsBytes);
    L.rec = A.take<float4>((size_t)nRec * 3);
    L.shapeBad = A.take<int>((size_t)B);
    if (algo != 1) {
        L.Lmax = pick_L(F);
        L.nLeafMax = 1u << (3 * L.Lmax);
        L.nNodeMax = lvl_off(L.Lmax + 1);
        L.srec = A.take<float4>((size_t)nRec * 3);
        L.part = A.take<float>((size_t)B * kParts * 6);
        L.dom = A.take<float>((size_t)B * 6);
        L.lvl = A.take<int>((size_t)B);
        L.nodes = A.take<float4>((size_t)B * L.nNodeMax * 2);
        L.fperm = A.take<int32_t>((size_t)nRec);
        L.seg = A.take<int32_t>((size_t)B * L.nLeafMax + 1);
        take_sort(A, (size_t)nRec, L.fs);
        if (algo == 2) {
            L.pperm = A.take<unsigned>((size_t)B * N);
            take_sort(A, (size_t)B * N, L.ps);
        }
    }
    L.bytes = A.end();
    return L;
}

}  // namespace wn
}  // namespace deftet

using namespace deftet;
using namespace deftet::wn;

extern "C" int deftet_winding_number_levels(int n_face) { return pick_L(n_face > 0 ? n_face : 0); }

extern "C" int deftet_winding_number_resolve_algo(int algo, int n_face_max, long long n_point_total)
{
    if (algo < 0 || algo > 3) return DEFTET_EINVAL;
    return resolve(algo, n_face_max, n_point_total);
}

extern "C" size_t deftet_winding_number_workspace_bytes(int B, long long n_face_total, int n_face_max, int N, int algo)
{
    if (B <= 0 || n_face_total < 0 || n_face_max < 0 || N < 0 || algo < 0 || algo > 3) return 0;
    return make_layout(B, n_face_max, n_face_total, N, resolve(algo, n_face_max, (long long)B * N), nullptr, 0).bytes;
}

extern "C" int deftet_winding_number_f32(const float *verts, const int32_t *vert_offsets, const int64_t *faces, const int32_t *face_offsets,
                                         const float *points, float *winding, int32_t *bad_counts, int B, int V, long long nRec, int F,
                                         int N, int algo, float beta, void *workspace, size_t workspace_bytes, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && V >= 0 && F >= 0 && N >= 0 && nRec >= 0, "negative size");
    DEFTET_CHECK_ARG(algo >= 0 && algo <= 3, "unknown algo %d", algo);
    DEFTET_CHECK_ARG(B <= 65535, "n_batch=%d exceeds 65535", B);
    DEFTET_CHECK_ARG((vert_offsets == nullptr) == (face_offsets == nullptr), "vertex and face offsets come together");
    DEFTET_CHECK_ARG(face_offsets || nRec == (long long)B * F, "uniform batch: n_face_total must be n_batch * n_face");
    DEFTET_CHECK_ARG(nRec < 0x7FFFFFFFLL && (long long)B * N < 0x7FFFFFFFLL, "too many faces or points");
    DEFTET_CHECK_ARG(!(beta != 0.f) || (beta >= 1.f && beta <= 1e6f), "beta=%g: 0 (the default) or a value in [1, 1e6] expected", (double)beta);
    if (B == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(points && winding && bad_counts, "null pointer");
    hipStream_t st = as_stream(stream_);
    const dim3 blk(256), gn(blocks_for(N, 256), B);
    if (F == 0 || nRec == 0) {
        DEFTET_HIP(hipMemsetAsync(bad_counts, 0, 16, st));
        DEFTET_LAUNCH(k_wn_empty, dim3(blocks_for((long long)B * N, 256)), blk, st, points, (long long)B * N, winding, bad_counts);
        return DEFTET_OK;
    }
    DEFTET_CHECK_ARG(verts && faces, "null mesh");
    algo = resolve(algo, F, (long long)B * N);
    Layout L = make_layout(B, F, nRec, N, algo, workspace, workspace_bytes);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    DEFTET_CHECK_ARG(algo == 1 || (unsigned long long)B * L.nLeafMax < 0x7FFFFFFFull, "too many leaves in the batch");
    DEFTET_HIP(hipMemsetAsync(bad_counts, 0, 16, st));
    DEFTET_HIP(hipMemsetAsync(L.shapeBad, 0, (size_t)B * 4, st));
    int pb = (F + 255) / 256;
    if (pb > kParts) pb = kParts;
    DEFTET_LAUNCH(k_wn_prep, dim3(pb, B), blk, st, verts, (const long long *)faces, V, F, L.rec, algo == 1 ? (float *)nullptr : L.part, bad_counts,
                  L.shapeBad, vert_offsets, face_offsets);
    if (algo == 1) {
        DEFTET_LAUNCH(k_wn_exact, gn, blk, st, points, (const float4 *)L.rec, N, F, face_offsets, (const int *)L.shapeBad, winding, bad_counts);
        return DEFTET_OK;
    }
    const float b = beta != 0.f ? beta : kBetaDefault;
    DEFTET_LAUNCH(k_wn_dom, dim3(B), dim3(64), st, (const float *)L.part, pb, F, L.Lmax, face_offsets, L.dom, L.lvl);
    DEFTET_LAUNCH(k_wn_face_keys, dim3(blocks_for(F, 256), B), blk, st, (const float4 *)L.rec, F, face_offsets, (const float *)L.dom,
                  (const int *)L.lvl, L.nLeafMax, L.fs.keys);
    DEFTET_TRY(sort_and_segment(L.fs, L.fperm, L.seg, (size_t)nRec, (unsigned)B * L.nLeafMax, st));
    DEFTET_LAUNCH(k_wn_gather, dim3(blocks_for(nRec, 256)), blk, st, (const float4 *)L.rec, (const int32_t *)L.fperm, nRec, L.srec);
    DEFTET_LAUNCH(k_wn_leaves, dim3(blocks_for(L.nLeafMax, 256), B), blk, st, (const float4 *)L.srec, (const int32_t *)L.seg, (const int *)L.lvl,
                  L.nLeafMax, L.nNodeMax, L.nodes);
    for (int l = L.Lmax - 1; l >= 0; --l)
        DEFTET_LAUNCH(k_wn_up, dim3(blocks_for((1u << (3 * l)), 256), B), blk, st, l, (const int *)L.lvl, L.nNodeMax, L.nodes);
    if (algo == 2) {
        DEFTET_LAUNCH(k_wn_point_keys, gn, blk, st, points, N, (const float *)L.dom, (const int *)L.lvl, L.nLeafMax, L.ps.keys);
        DEFTET_TRY(prims::radix_sort_from<unsigned, unsigned>(prims::PtrLoad<unsigned>{L.ps.keys}, L.ps.sorted, prims::IotaLoad{}, L.pperm,
                                                              (size_t)B * N, key_bits((unsigned)B * L.nLeafMax), L.ps.tmp, L.ps.tmp_bytes, st));
        DEFTET_LAUNCH(k_wn_query<true>, gn, blk, st, points, (const float4 *)L.srec, (const float4 *)L.nodes, (const int32_t *)L.seg,
                      (const int *)L.lvl, (const int *)L.shapeBad, (const unsigned *)L.pperm, N, L.nLeafMax, L.nNodeMax, b * b, winding, bad_counts);
    } else {
        DEFTET_LAUNCH(k_wn_query<false>, gn, blk, st, points, (const float4 *)L.srec, (const float4 *)L.nodes, (const int32_t *)L.seg,
                      (const int *)L.lvl, (const int *)L.shapeBad, (const unsigned *)nullptr, N, L.nLeafMax, L.nNodeMax, b * b, winding, bad_counts);
    }
    return DEFTET_OK;
}
