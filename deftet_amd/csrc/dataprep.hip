// dataprep.hip — ground-truth preparation on the GPU (gfx950): conservative surface voxelization, orthographic depth maps and
// their projection, the fused fill, the cuberille surface of a voxel grid and the unique edges of a triangle list.
//
//   dataloader.py:24-61 (MakeSurfaceMesh.__call__) makes a shape watertight with six Kaolin calls: trianglemeshes_to_voxelgrids,
//   extract_odms, project_odms, voxelgrids_to_trianglemeshes, adjacency_matrix (+ torch.sparse.mm).  PARITY UNPINNED: Kaolin is
//   neither in the reference tree nor readable here; the semantics below are this library's own and are
//   restated in numpy in tests/dataprep_ref.py.
//
// The hand-off format between the stages is the bit grid: uint32 [B,R,R,W], W = ceil(R / 32), bit k % 32 of word k / 32 of row
// (i, j) is voxel (i, j, k); the pad bits of the last word are zero.
//
// Voxelization.  q = ((v - origin) / scale) * R in fp32.  A count pass (one lane per triangle) gives every triangle its
// candidate box and the number of wave tasks it needs: the unit of work is one word column (i, j, word of k) of the box, a
// task is kUnitBudget units, so a triangle across the whole grid is cut into many tasks that run on as many waves instead of
// serialising one (the rasterizer's sliver finding; the launch never has fewer than kMinRasterBlocks workgroups, so this
// holds for a mesh of a few large triangles too).  An exclusive scan of the task counts gives every triangle's first task;
// a wave finds its triangle by a binary search of that table (uniform over the wave), sets the triangle up once and its lanes
// take the units: up to 32 separating-axis tests along k build one mask, ONE atomicOr per word publishes it.  The OR does not
// depend on the order of its operands: the grid is bit-reproducible.
//
// Fill (project_odms(extract_odms(v)) at votes = 1): a voxel stays iff on every axis it lies between the first and the last
// occupied voxel of its ray.  Along k that is first-set-bit / last-set-bit of the row's words; along i and j it is
// (prefix OR) & (suffix OR) of the words of a column, 32 rays per thread.  No depth map is stored.
//
// Surface.  Count (popcounts of occ & ~neighbour per word and direction; used lattice corners per corner word), two
// exclusive scans (prims.hpp), fill — the pattern of surface_extract.hip.  Rows are ordered by (voxel, direction, triangle),
// vertices by corner key, so the mesh is welded by construction.
#include "common.hpp"
#include "prims.hpp"

namespace deftet {
namespace dp {

constexpr int kThreads = 256;
constexpr int kUnitBudget = 256;          // word columns per wave task (DEFTET_VOXELIZE_UNIT_BUDGET)
constexpr int kMaxRes = 1024;
constexpr unsigned kMinRasterBlocks = 1024;   // four workgroups (16 waves) on each of 256 compute units

static inline int words_of(int R) { return (R + 31) >> 5; }
// ---------------------------------------------------------------------------- voxelization
// os[b] = (origin x, y, z, scale): the given ones, or the minimum of the vertices / their largest extent
__global__ __launch_bounds__(kThreads) void k_vx_frame(const float *__restrict__ verts, int V, const float *__restrict__ origin,
                                                        const float *__restrict__ scale, float4 *os)
{
    __shared__ float s_mn[3][kThreads / 64], s_mx[3][kThreads / 64];
    const int b = blockIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (!origin || !scale) {
        const float *v = verts + (size_t)b * V * 3;
        for (int i = threadIdx.x; i < V; i += kThreads)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = v[(size_t)i * 3 + k];
                mn[k] = fminf(mn[k], x);                              // (min and max do not depend on the order)
                mx[k] = fmaxf(mx[k], x);
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll  // wave_min's and wave_max's order (wave.hpp); written out, a call changes this kernel's instruction stream
            for (int off = 32; off > 0; off >>= 1) {
                mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
                mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
            }
            if ((threadIdx.x & 63) == 0) { s_mn[k][threadIdx.x >> 6] = mn[k]; s_mx[k][threadIdx.x >> 6] = mx[k]; }
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (!origin || !scale)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int w = 0; w < kThreads / 64; ++w) { mn[k] = fminf(mn[k], s_mn[k][w]); mx[k] = fmaxf(mx[k], s_mx[k][w]); }
    float4 r;
    r.x = origin ? origin[b * 3 + 0] : mn[0];
    r.y = origin ? origin[b * 3 + 1] : mn[1];
    r.z = origin ? origin[b * 3 + 2] : mn[2];
    r.w = scale ? scale[b] : fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    os[b] = r;
}

struct Tri {
    float q[3][3];            // corner m, coordinate c, in voxel units
    int lo[3], hi[3];         // candidate box, inclusive; empty when lo > hi on an axis
    bool ok;
};

__device__ __forceinline__ Tri load_tri(const float *__restrict__ verts, const long long *__restrict__ faces, const float4 *__restrict__ os,
                                        int b, int f, int V, int R, int *bad)
{
    Tri t;
    t.ok = false;
    const float4 o = os[b];
    const float oc[3] = {o.x, o.y, o.z}, Rf = (float)R;
    bool fin = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const long long vi = faces[(size_t)f * 3 + m];
        if (vi < 0 || vi >= V) { if (bad) *bad = 1; return t; }
        const float *p = verts + ((size_t)b * V + (size_t)vi) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float q = ((p[c] - oc[c]) / o.w) * Rf;
            t.q[m][c] = q;
            fin = fin && (fabsf(q) <= 3.0e38f);                      // false for NaN and +-inf
        }
    }
    if (!fin) return t;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mn = fminf(fminf(t.q[0][c], t.q[1][c]), t.q[2][c]), mx = fmaxf(fmaxf(t.q[0][c], t.q[1][c]), t.q[2][c]);
        // i + 1 >= mn and i <= mx, clipped to the grid (the clamp first: the conversion must not overflow)
        const int lo = (int)ceilf(fminf(fmaxf(mn, -1.0f), Rf + 1.0f)) - 1, hi = (int)floorf(fminf(fmaxf(mx, -1.0f), Rf + 1.0f));
        t.lo[c] = max(lo, 0);
        t.hi[c] = min(hi, R - 1);
    }
    t.ok = t.lo[0] <= t.hi[0] && t.lo[1] <= t.hi[1] && t.lo[2] <= t.hi[2];
    return t;
}

__device__ __forceinline__ int tri_units(const Tri &t)
{
    return (t.hi[0] - t.lo[0] + 1) * (t.hi[1] - t.lo[1] + 1) * ((t.hi[2] >> 5) - (t.lo[2] >> 5) + 1);
}

// ntask[b F + f] = wave tasks of the triangle; ntask[B F] = 0 (its exclusive scan value is the total)
__global__ __launch_bounds__(kThreads) void k_vx_count(const float *__restrict__ verts, const long long *__restrict__ faces,
                                                        const float4 *__restrict__ os, int B, int V, int F, int R, int *ntask, int *stats)
{
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x, n = (long long)B * F;
    if (g > n) return;
    if (g == n) { ntask[g] = 0; return; }
    const Tri t = load_tri(verts, faces, os, (int)(g / F), (int)(g % F), V, R, stats + 2);
    const int nt = t.ok ? (tri_units(t) + kUnitBudget - 1) / kUnitBudget : 0;
    ntask[g] = nt;
    if (nt > 1) atomicAdd(stats + 1, 1);                              // (an integer count: order-free)
}

// the 13-axis separating-axis test of a triangle against the closed box of half size 0.5 about the origin, in fp32, every
// product and sum rounded on its own (the build contracts nothing).  a[m] = corner m relative to the voxel centre.
__device__ __forceinline__ bool tri_box_overlap(const float a[3][3], const float e[3][3])
{
    const float h = 0.5f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mn = fminf(fminf(a[0][c], a[1][c]), a[2][c]), mx = fmaxf(fmaxf(a[0][c], a[1][c]), a[2][c]);
        if (mn > h || mx < -h) return false;
    }
    const float nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2],
                nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    const float d = (nx * a[0][0] + ny * a[0][1]) + nz * a[0][2];
    if (fabsf(d) > h * ((fabsf(nx) + fabsf(ny)) + fabsf(nz))) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // e_i x unit axis j has two non-zero components, on the axes u = j + 1 and v = j + 2 (mod 3): (e_v, -e_u)
            const int u = (j + 1) % 3, v = (j + 2) % 3;
            const float p0 = e[i][v] * a[0][u] - e[i][u] * a[0][v], p1 = e[i][v] * a[1][u] - e[i][u] * a[1][v],
                        p2 = e[i][v] * a[2][u] - e[i][u] * a[2][v];
            const float r = h * (fabsf(e[i][v]) + fabsf(e[i][u]));
            if (fminf(fminf(p0, p1), p2) > r || fmaxf(fmaxf(p0, p1), p2) < -r) return false;
        }
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void k_vx_raster(const float *__restrict__ verts, const long long *__restrict__ faces,
                                                         const float4 *__restrict__ os, int B, int V, int F, int R, int W,
                                                         const int *__restrict__ tpos, unsigned *bits, int *stats)
{
    const int lane = threadIdx.x & 63;
    const long long nwave = (long long)gridDim.x * (kThreads / 64), n = (long long)B * F;
    const int total = tpos[n];
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = total;
    for (long long task = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); task < total; task += nwave) {
        // the last triangle whose first task is <= task (triangles without tasks repeat their successor's value: skipped)
        long long lo = 0, hi = n - 1;
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if (tpos[mid] <= (int)task) lo = mid; else hi = mid - 1;
        }
        const int b = (int)(lo / F), f = (int)(lo % F), chunk = (int)task - tpos[lo];
        const Tri t = load_tri(verts, faces, os, b, f, V, R, nullptr);
        if (!t.ok) continue;                                          // (never: the count pass gave it tasks)
        float e[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            e[0][c] = t.q[1][c] - t.q[0][c];
            e[1][c] = t.q[2][c] - t.q[1][c];
            e[2][c] = t.q[0][c] - t.q[2][c];
        }
        const int ny = t.hi[1] - t.lo[1] + 1, w0 = t.lo[2] >> 5, nw = (t.hi[2] >> 5) - w0 + 1;
        const int units = tri_units(t), end = min(units, (chunk + 1) * kUnitBudget);
        for (int u = chunk * kUnitBudget + lane; u < end; u += 64) {
            const int wz = u % nw, r = u / nw, i = t.lo[0] + r / ny, j = t.lo[1] + r % ny, w = w0 + wz;
            const int ka = max(t.lo[2], w * 32), kb = min(t.hi[2], w * 32 + 31);
            const float cx = (float)i + 0.5f, cy = (float)j + 0.5f;
            float a[3][3];
#pragma unroll
            for (int m = 0; m < 3; ++m) { a[m][0] = t.q[m][0] - cx; a[m][1] = t.q[m][1] - cy; }
            unsigned mask = 0u;
            for (int k = ka; k <= kb; ++k) {
                const float cz = (float)k + 0.5f;
#pragma unroll
                for (int m = 0; m < 3; ++m) a[m][2] = t.q[m][2] - cz;
                if (tri_box_overlap(a, e)) mask |= 1u << (k & 31);
            }
            if (mask) atomicOr(bits + (((size_t)b * R + i) * R + j) * W + w, mask);      // i, j < R and w < W by the clipped box
        }
    }
}

// ---------------------------------------------------------------------------- bit grid <-> byte grid
__global__ __launch_bounds__(kThreads) void k_unpack(const unsigned *__restrict__ bits, size_t n, int R, int W, unsigned char *vox)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    const size_t row = g / R;
    const int k = (int)(g - row * R);
    vox[g] = (unsigned char)((bits[row * W + (k >> 5)] >> (k & 31)) & 1u);
}

__global__ __launch_bounds__(kThreads) void k_pack(const unsigned char *__restrict__ vox, size_t nword, int R, int W, unsigned *bits)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= nword) return;
    const size_t row = g / W;
    const int w = (int)(g - row * W), k1 = min(R, w * 32 + 32);
    unsigned m = 0u;
    for (int k = w * 32; k < k1; ++k) m |= (vox[row * R + k] ? 1u : 0u) << (k & 31);
    bits[g] = m;
}

// ---------------------------------------------------------------------------- depth maps and their projection
// direction d scans axis d / 2, ascending (d even) or descending (d odd); a map is indexed by the two other axes, ascending
__global__ __launch_bounds__(kThreads) void k_odm_extract(const unsigned char *__restrict__ vox, int B, int R, int *odms)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)B * 6 * R * R;
    if (g >= n) return;
    const int q = (int)(g % R), p = (int)((g / R) % R), d = (int)((g / ((size_t)R * R)) % 6), b = (int)(g / ((size_t)6 * R * R));
    const int axis = d >> 1;
    const size_t sp = axis == 0 ? (size_t)R : (size_t)R * R, sq = axis == 2 ? (size_t)R : 1, ss = axis == 0 ? (size_t)R * R : (axis == 1 ? R : 1);
    const unsigned char *base = vox + (size_t)b * R * R * R + p * sp + q * sq;
    int depth = R;
    for (int s = 0; s < R; ++s) {
        const int x = (d & 1) ? R - 1 - s : s;
        if (base[x * ss]) { depth = s; break; }
    }
    odms[g] = depth;
}

__global__ __launch_bounds__(kThreads) void k_odm_project(const int *__restrict__ odms, const unsigned char *__restrict__ vin, int B, int R,
                                                           int votes, unsigned char *out)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)B * R * R * R;
    if (g >= n) return;
    const int k = (int)(g % R), j = (int)((g / R) % R), i = (int)((g / ((size_t)R * R)) % R);
    const size_t b = g / ((size_t)R * R * R);
    const int *m = odms + b * 6 * R * R;
    const size_t RR = (size_t)R * R;
    const int x[3] = {i, j, k};
    const size_t at[3] = {(size_t)j * R + k, (size_t)i * R + k, (size_t)i * R + j};
    int carved = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        carved += x[a] < m[(2 * a) * RR + at[a]] ? 1 : 0;                       // in front of the first voxel seen from below
        carved += R - 1 - x[a] < m[(2 * a + 1) * RR + at[a]] ? 1 : 0;           // ... from above
    }
    const bool start = vin ? vin[g] != 0 : true;
    out[g] = (unsigned char)((start && carved < votes) ? 1 : 0);
}

// ---------------------------------------------------------------------------- fused fill on the bit grid
// out = the span between the first and the last set bit of every (i, j) row, over its W words
__global__ __launch_bounds__(kThreads) void k_fill_span_k(const unsigned *__restrict__ bits, size_t nrow, int W, unsigned *out)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= nrow) return;
    const unsigned *row = bits + g * W;
    int first = -1, last = -1;
    for (int w = 0; w < W; ++w) {
        const unsigned x = row[w];
        if (x) {
            if (first < 0) first = w * 32 + __ffs(x) - 1;
            last = w * 32 + 31 - __clz(x);
        }
    }
    for (int w = 0; w < W; ++w) {
        unsigned m = 0u;
        if (first >= 0 && last >= w * 32 && first <= w * 32 + 31) {
            const int a = max(first - w * 32, 0), z = min(last - w * 32, 31);
            m = (z == 31 ? 0xFFFFFFFFu : ((1u << (z + 1)) - 1u)) & ~((1u << a) - 1u);
        }
        out[g * W + w] = m;
    }
}

// out &= (prefix OR) & (suffix OR) of the input words along one of the two unpacked axes: a thread owns 32 rays.
// column c of shape b: words at base(c) + s * stride, s = 0 .. R-1
__global__ __launch_bounds__(kThreads) void k_fill_span_axis(const unsigned *__restrict__ bits, int B, int R, int W, int axis, unsigned *tmp,
                                                              unsigned *out)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)B * R * W;
    if (g >= n) return;
    const int w = (int)(g % W), o = (int)((g / W) % R);
    const size_t b = g / ((size_t)W * R);
    const size_t stride = axis == 0 ? (size_t)R * W : (size_t)W;
    const size_t base = b * R * R * W + (axis == 0 ? (size_t)o * W : (size_t)o * R * W) + w;
    unsigned run = 0u;
    for (int s = 0; s < R; ++s) {
        run |= bits[base + s * stride];
        tmp[base + s * stride] = run;                                 // (own words: nobody else reads or writes them)
    }
    run = 0u;
    for (int s = R - 1; s >= 0; --s) {
        run |= bits[base + s * stride];
        out[base + s * stride] &= tmp[base + s * stride] & run;
    }
}

// ---------------------------------------------------------------------------- cuberille surface
struct Grid {
    const unsigned *bits;
    int B, R, W, Wc;          // Wc = words of a corner row (R + 1 corners)
};

__device__ __forceinline__ unsigned word_at(const Grid &G, int b, int i, int j, int w)
{
    if (i < 0 || j < 0 || w < 0 || i >= G.R || j >= G.R || w >= G.W) return 0u;
    return G.bits[(((size_t)b * G.R + i) * G.R + j) * G.W + w];
}

// m[d] = voxels of the word whose neighbour in direction d is empty or outside: d = 0 / 1 towards -i / +i, 2 / 3 -j / +j, 4 / 5 -k / +k
__device__ __forceinline__ unsigned face_masks(const Grid &G, int b, int i, int j, int w, unsigned m[6])
{
    const unsigned occ = word_at(G, b, i, j, w);
    if (!occ) { m[0] = m[1] = m[2] = m[3] = m[4] = m[5] = 0u; return 0u; }
    m[0] = occ & ~word_at(G, b, i - 1, j, w);
    m[1] = occ & ~word_at(G, b, i + 1, j, w);
    m[2] = occ & ~word_at(G, b, i, j - 1, w);
    m[3] = occ & ~word_at(G, b, i, j + 1, w);
    m[4] = occ & ~((occ << 1) | (word_at(G, b, i, j, w - 1) >> 31));
    m[5] = occ & ~((occ >> 1) | (word_at(G, b, i, j, w + 1) << 31));
    return occ;
}

__global__ __launch_bounds__(kThreads) void k_sf_count_faces(Grid G, int *fcnt)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)G.B * G.R * G.R * G.W;
    if (g > n) return;
    if (g == n) { fcnt[g] = 0; return; }
    const int w = (int)(g % G.W), j = (int)((g / G.W) % G.R), i = (int)((g / ((size_t)G.W * G.R)) % G.R), b = (int)(g / ((size_t)G.W * G.R * G.R));
    unsigned m[6];
    face_masks(G, b, i, j, w, m);
    int c = 0;
#pragma unroll
    for (int d = 0; d < 6; ++d) c += __popc(m[d]);
    fcnt[g] = 2 * c;
}

// a lattice corner is in use iff the (up to) eight voxels around it are not all equal, outside counting as empty
__global__ __launch_bounds__(kThreads) void k_sf_count_verts(Grid G, unsigned *used, int *vcnt)
{
    const int R1 = G.R + 1;
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)G.B * R1 * R1 * G.Wc;
    if (g > n) return;
    if (g == n) { vcnt[g] = 0; return; }
    const int w = (int)(g % G.Wc), j = (int)((g / G.Wc) % R1), i = (int)((g / ((size_t)G.Wc * R1)) % R1), b = (int)(g / ((size_t)G.Wc * R1 * R1));
    unsigned any = 0u, all = 0xFFFFFFFFu, anyp = 0u, allp = 0xFFFFFFFFu;
#pragma unroll
    for (int di = -1; di <= 0; ++di)
#pragma unroll
        for (int dj = -1; dj <= 0; ++dj) {
            const unsigned x = word_at(G, b, i + di, j + dj, w), xp = word_at(G, b, i + di, j + dj, w - 1);
            any |= x; all &= x; anyp |= xp; allp &= xp;
        }
    // corner k looks at the voxels k - 1 and k of the four rows
    const unsigned any_lo = (any << 1) | (anyp >> 31), all_lo = (all << 1) | (allp >> 31);
    unsigned u = (any | any_lo) & ~(all & all_lo);
    const int left = R1 - w * 32;                                     // corners of this word: k <= R
    if (left < 32) u &= (1u << left) - 1u;
    used[g] = u;
    vcnt[g] = __popc(u);
}

__global__ void k_sf_offsets(const int *__restrict__ fpos, const int *__restrict__ vpos, Grid G, int *offsets)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > G.B) return;
    const int R1 = G.R + 1;
    offsets[b] = fpos[(size_t)b * G.R * G.R * G.W];
    offsets[G.B + 1 + b] = vpos[(size_t)b * R1 * R1 * G.Wc];
}

__device__ __forceinline__ long long corner_id(const Grid &G, const unsigned *__restrict__ used, const int *__restrict__ vpos, int b,
                                               const int c[3], int vbase)
{
    const int R1 = G.R + 1;
    const size_t cw = (((size_t)b * R1 + c[0]) * R1 + c[1]) * G.Wc + (c[2] >> 5);
    return (long long)(vpos[cw] - vbase + __popc(used[cw] & ((1u << (c[2] & 31)) - 1u)));
}

__global__ __launch_bounds__(kThreads) void k_sf_fill_faces(Grid G, const int *__restrict__ fpos, const unsigned *__restrict__ used,
                                                             const int *__restrict__ vpos, long long capacity, long long *faces)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)G.B * G.R * G.R * G.W;
    if (g >= n) return;
    long long row = fpos[g];
    if (fpos[g + 1] == (int)row || row < 0) return;
    const int w = (int)(g % G.W), j = (int)((g / G.W) % G.R), i = (int)((g / ((size_t)G.W * G.R)) % G.R), b = (int)(g / ((size_t)G.W * G.R * G.R));
    unsigned m[6];
    face_masks(G, b, i, j, w, m);
    const int R1 = G.R + 1, vbase = vpos[(size_t)b * R1 * R1 * G.Wc];
    unsigned todo = m[0] | m[1] | m[2] | m[3] | m[4] | m[5];
    while (todo) {
        const int t = __ffs(todo) - 1;
        todo &= todo - 1u;
        const int x[3] = {i, j, w * 32 + t};
        for (int d = 0; d < 6; ++d) {
            if (!((m[d] >> t) & 1u)) continue;
            const int a = d >> 1, u = (a + 1) % 3, v = (a + 2) % 3;
            int p00[3] = {x[0], x[1], x[2]}, p10[3], p11[3], p01[3];
            p00[a] += d & 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) { p10[c] = p00[c] + (c == u); p01[c] = p00[c] + (c == v); p11[c] = p00[c] + (c == u) + (c == v); }
            const long long i00 = corner_id(G, used, vpos, b, p00, vbase), i10 = corner_id(G, used, vpos, b, p10, vbase),
                            i11 = corner_id(G, used, vpos, b, p11, vbase), i01 = corner_id(G, used, vpos, b, p01, vbase);
            // e_u x e_v = e_a: (p00, p10, p11) looks along +a; the face towards -a is wound the other way
            const long long q[6] = {i00, (d & 1) ? i10 : i01, i11, i00, i11, (d & 1) ? i01 : i10};
            if (row + 2 <= capacity)
#pragma unroll
                for (int c = 0; c < 6; ++c) faces[row * 3 + c] = q[c];
            row += 2;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_sf_fill_verts(Grid G, const unsigned *__restrict__ used, const int *__restrict__ vpos,
                                                             long long capacity, float *verts)
{
    const int R1 = G.R + 1;
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, n = (size_t)G.B * R1 * R1 * G.Wc;
    if (g >= n) return;
    unsigned u = used[g];
    long long row = vpos[g];
    if (!u || row < 0) return;
    const int w = (int)(g % G.Wc), j = (int)((g / G.Wc) % R1), i = (int)((g / ((size_t)G.Wc * R1)) % R1);
    while (u) {
        const int t = __ffs(u) - 1;
        u &= u - 1u;
        if (row < capacity) {
            verts[row * 3 + 0] = (float)i;
            verts[row * 3 + 1] = (float)j;
            verts[row * 3 + 2] = (float)(w * 32 + t);
        }
        ++row;
    }
}

// ---------------------------------------------------------------------------- unique directed edges of a triangle list
__global__ __launch_bounds__(kThreads) void k_edge_keys(const long long *__restrict__ faces, long long n, int V, unsigned long long *keys,
                                                         int *n_out)
{
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const long long f = e / 6;
    const int s = (int)(e - f * 6), ca = s >> 1, cb = (ca + 1) % 3;
    const long long a = faces[f * 3 + ((s & 1) ? cb : ca)], b = faces[f * 3 + ((s & 1) ? ca : cb)];
    const unsigned long long none = (unsigned long long)V * (unsigned long long)V;
    if (a < 0 || b < 0 || a >= V || b >= V) { n_out[1] = 1; keys[e] = none; return; }
    keys[e] = a == b ? none : (unsigned long long)a * (unsigned long long)V + (unsigned long long)b;      // (no self edge)
}

__device__ __forceinline__ bool edge_head(const unsigned long long *__restrict__ keys, long long i, unsigned long long none)
{
    return keys[i] < none && (i == 0 || keys[i] != keys[i - 1]);
}

__global__ __launch_bounds__(kThreads) void k_edge_flag(const unsigned long long *__restrict__ keys, long long n, int V, int *flag)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && edge_head(keys, i, (unsigned long long)V * (unsigned long long)V)) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_edge_compact(const unsigned long long *__restrict__ keys, long long n, int V,
                                                            const int *__restrict__ pos, int *pairs, int *n_out)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    if (i == n) { n_out[0] = pos[n]; return; }
    if (!edge_head(keys, i, (unsigned long long)V * (unsigned long long)V)) return;
    const int p = pos[i];                                             // p <= i < n: inside the 6 F rows the caller gave
    pairs[(size_t)p * 2 + 0] = (int)(keys[i] / (unsigned long long)V);
    pairs[(size_t)p * 2 + 1] = (int)(keys[i] % (unsigned long long)V);
}

static int check_grid(int B, int R)
{
    DEFTET_CHECK_ARG(R >= 1 && R <= kMaxRes, "resolution=%d outside 1..%d", R, kMaxRes);
    DEFTET_CHECK_ARG(B >= 1, "n_batch=%d must be positive", B);
    DEFTET_CHECK_ARG((long long)B * (R + 1) * (R + 1) * (R + 1) < 2147483647LL, "n_batch * (resolution + 1)^3 does not fit 31 bits");
    return DEFTET_OK;
}

// the face table is int32: a shape has at most 3 R R (R + 1) lattice faces, two triangles each
static int check_surface(int B, int R)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG((long long)B * 6 * R * R * (R + 1) < 2147483647LL, "n_batch * 6 * resolution^2 * (resolution + 1) triangles at most do not fit 31 bits");
    return DEFTET_OK;
}

struct SurfWs {
    int *fpos, *vpos;
    unsigned *used;
    void *tmp;
    size_t tmp_bytes, total;
};
static SurfWs surf_carve(void *ws, int B, int R)
{
    const size_t nf = (size_t)B * R * R * words_of(R) + 1, nv = (size_t)B * (R + 1) * (R + 1) * words_of(R + 1) + 1;
    Arena A(ws);
    SurfWs s;
    s.fpos = A.take<int>(nf);
    s.vpos = A.take<int>(nv);
    s.used = A.take<unsigned>(nv);
    s.tmp_bytes = prims::scan_temp_bytes<int>(nf > nv ? nf : nv);
    s.tmp = A.take<char>(s.tmp_bytes);
    s.total = A.end();
    return s;
}

// the frame of every shape, the wave tasks of every triangle (scanned in place; the last entry becomes the total)
struct VoxWs {
    float4 *os;
    int *tpos;
    void *tmp;
    size_t n, tmp_bytes, total;
};
static VoxWs vox_carve(void *ws, int B, int F)
{
    Arena A(ws);
    VoxWs s;
    s.n = (size_t)B * F + 1;
    s.os = A.take<float4>(B);
    s.tpos = A.take<int>(s.n);
    s.tmp_bytes = prims::scan_temp_bytes<int>(s.n);
    s.tmp = A.take<char>(s.tmp_bytes);
    s.total = A.end();
    return s;
}

// the six directed edge keys of every face before and after the sort, the heads' flags (scanned in place; entry n is the count)
struct EdgeWs {
    unsigned long long *k0, *k1;
    int *pos;
    void *scan_tmp, *sort_tmp;
    size_t n, scan_bytes, sort_bytes, total;
};
static EdgeWs edge_carve(void *ws, int F)
{
    Arena A(ws);
    EdgeWs s;
    s.n = (size_t)F * 6;
    s.k0 = A.take<unsigned long long>(s.n);
    s.k1 = A.take<unsigned long long>(s.n);
    s.pos = A.take<int>(s.n + 1);
    s.scan_bytes = prims::scan_temp_bytes<int>(s.n + 1);
    s.scan_tmp = A.take<char>(s.scan_bytes);
    s.sort_bytes = prims::radix_sort_temp_bytes<unsigned long long, unsigned>(s.n, false);
    s.sort_tmp = A.take<char>(s.sort_bytes);
    s.total = A.end();
    return s;
}

}  // namespace dp
}  // namespace deftet

using namespace deftet;
using namespace deftet::dp;

extern "C" size_t deftet_mesh_voxelize_workspace_bytes(int B, int F)
{
    return B <= 0 || F < 0 ? 256 : vox_carve(nullptr, B, F).total;
}

extern "C" int deftet_mesh_voxelize_f32(const float *verts, const int64_t *faces, const float *origin, const float *scale, int B, int V,
                                        int F, int R, uint32_t *bits, uint8_t *vox, int32_t *stats, void *workspace, size_t wsb,
                                        void *stream_)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG(V >= 0 && F >= 0, "n_vertex=%d, n_face=%d: neither may be negative", V, F);
    DEFTET_CHECK_ARG((long long)B * F < 2147483647LL, "n_batch * n_face does not fit 31 bits");
    {
        // the task table is int32: a triangle has at most ceil(R R W / budget) tasks (its box is the whole grid)
        const long long per_tri = ((long long)R * R * words_of(R) + kUnitBudget - 1) / kUnitBudget;
        DEFTET_CHECK_ARG((long long)B * F * per_tri < 2147483647LL,
                         "n_batch * n_face * ceil(R * R * ceil(R / 32) / %d) = %lld wave tasks at most do not fit 31 bits", kUnitBudget,
                         (long long)B * F * per_tri);
    }
    DEFTET_CHECK_ARG(bits && stats, "null pointer: bits / stats");
    DEFTET_CHECK_ARG(F == 0 || (verts && faces && V > 0), "null pointer: verts / faces");
    DEFTET_CHECK_ARG(V > 0 || (origin && scale), "no vertices: origin and scale cannot be derived");
    const VoxWs S = vox_carve(workspace, B, F);
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, S.total));
    hipStream_t st = as_stream(stream_);
    const int W = words_of(R);
    const size_t nword = (size_t)B * R * R * W, n = S.n;
    DEFTET_HIP(hipMemsetAsync(bits, 0, nword * 4, st));
    DEFTET_HIP(hipMemsetAsync(stats, 0, 16, st));
    if (F > 0) {
        DEFTET_LAUNCH(k_vx_frame, dim3(B), dim3(kThreads), st, verts, V, origin, scale, S.os);
        DEFTET_LAUNCH(k_vx_count, dim3(blocks_for(n, kThreads)), dim3(kThreads), st, verts, (const long long *)faces, (const float4 *)S.os, B, V, F, R, S.tpos,
                      (int *)stats);
        DEFTET_TRY(prims::scan<int, prims::Plus, true>(S.tpos, S.tpos, n, 0, prims::Plus(), S.tmp, S.tmp_bytes, st));
        // the number of tasks stays on the device, so the grid cannot follow it: one wave per triangle, but never fewer than
        // kMinRasterBlocks workgroups (a few large triangles are many tasks; a wave without a task reads the total and leaves)
        // and never more than a full machine of waves; the waves stride over the tasks
        const size_t want = (n - 1 + 3) / 4;
        const unsigned nblk = (unsigned)(want < kMinRasterBlocks ? kMinRasterBlocks : (want < 8192 ? want : 8192));
        DEFTET_LAUNCH(k_vx_raster, dim3(nblk), dim3(kThreads), st, verts, (const long long *)faces, (const float4 *)S.os, B, V, F, R, W,
                      (const int *)S.tpos, (unsigned *)bits, (int *)stats);
    }
    if (vox) DEFTET_LAUNCH(k_unpack, dim3(blocks_for((size_t)B * R * R * R, kThreads)), dim3(kThreads), st, (const unsigned *)bits, (size_t)B * R * R * R, R, W, vox);
    return DEFTET_OK;
}

extern "C" int deftet_voxel_pack_u8(const uint8_t *vox, int B, int R, uint32_t *bits, void *stream_)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG(vox && bits, "null pointer: vox / bits");
    const int W = words_of(R);
    const size_t nword = (size_t)B * R * R * W;
    DEFTET_LAUNCH(k_pack, dim3(blocks_for(nword, kThreads)), dim3(kThreads), as_stream(stream_), vox, nword, R, W, (unsigned *)bits);
    return DEFTET_OK;
}

extern "C" int deftet_voxel_unpack_u8(const uint32_t *bits, int B, int R, uint8_t *vox, void *stream_)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG(vox && bits, "null pointer: vox / bits");
    const size_t n = (size_t)B * R * R * R;
    DEFTET_LAUNCH(k_unpack, dim3(blocks_for(n, kThreads)), dim3(kThreads), as_stream(stream_), (const unsigned *)bits, n, R, words_of(R), vox);
    return DEFTET_OK;
}

extern "C" int deftet_extract_odms_u8(const uint8_t *vox, int B, int R, int32_t *odms, void *stream_)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG(vox && odms, "null pointer: vox / odms");
    DEFTET_LAUNCH(k_odm_extract, dim3(blocks_for((size_t)B * 6 * R * R, kThreads)), dim3(kThreads), as_stream(stream_), vox, B, R, (int *)odms);
    return DEFTET_OK;
}

extern "C" int deftet_project_odms_i32(const int32_t *odms, const uint8_t *vox_in, int B, int R, int votes, uint8_t *out, void *stream_)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG(odms && out, "null pointer: odms / out");
    DEFTET_CHECK_ARG(votes >= 1 && votes <= 6, "votes=%d outside 1..6", votes);
    DEFTET_LAUNCH(k_odm_project, dim3(blocks_for((size_t)B * R * R * R, kThreads)), dim3(kThreads), as_stream(stream_), (const int *)odms, vox_in, B, R, votes,
                  out);
    return DEFTET_OK;
}

extern "C" size_t deftet_voxel_fill_workspace_bytes(int B, int R)
{
    if (B <= 0 || R <= 0) return 256;
    return align_up((size_t)B * R * R * words_of(R) * 4, 256);
}

extern "C" int deftet_voxel_fill_b32(const uint32_t *bits, int B, int R, uint32_t *out, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_grid(B, R));
    DEFTET_CHECK_ARG(bits && out && bits != out, "null pointer: bits / out, or out aliases bits");
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, deftet_voxel_fill_workspace_bytes(B, R)));
    hipStream_t st = as_stream(stream_);
    const int W = words_of(R);
    DEFTET_LAUNCH(k_fill_span_k, dim3(blocks_for((size_t)B * R * R, kThreads)), dim3(kThreads), st, (const unsigned *)bits, (size_t)B * R * R, W, (unsigned *)out);
    for (int axis = 0; axis < 2; ++axis)
        DEFTET_LAUNCH(k_fill_span_axis, dim3(blocks_for((size_t)B * R * W, kThreads)), dim3(kThreads), st, (const unsigned *)bits, B, R, W, axis,
                      (unsigned *)workspace, (unsigned *)out);
    return DEFTET_OK;
}

extern "C" size_t deftet_voxel_surface_workspace_bytes(int B, int R)
{
    if (B <= 0 || R <= 0 || R > kMaxRes) return 256;
    return surf_carve(nullptr, B, R).total;
}

extern "C" int deftet_voxel_surface_count_b32(const uint32_t *bits, int B, int R, int32_t *offsets, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_surface(B, R));
    DEFTET_CHECK_ARG(bits && offsets, "null pointer: bits / offsets");
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, deftet_voxel_surface_workspace_bytes(B, R)));
    hipStream_t st = as_stream(stream_);
    const SurfWs S = surf_carve(workspace, B, R);
    const Grid G{(const unsigned *)bits, B, R, words_of(R), words_of(R + 1)};
    const size_t nf = (size_t)B * R * R * G.W + 1, nv = (size_t)B * (R + 1) * (R + 1) * G.Wc + 1;
    DEFTET_LAUNCH(k_sf_count_faces, dim3(blocks_for(nf, kThreads)), dim3(kThreads), st, G, S.fpos);
    DEFTET_LAUNCH(k_sf_count_verts, dim3(blocks_for(nv, kThreads)), dim3(kThreads), st, G, S.used, S.vpos);
    DEFTET_TRY(prims::scan<int, prims::Plus, true>(S.fpos, S.fpos, nf, 0, prims::Plus(), S.tmp, S.tmp_bytes, st));
    DEFTET_TRY(prims::scan<int, prims::Plus, true>(S.vpos, S.vpos, nv, 0, prims::Plus(), S.tmp, S.tmp_bytes, st));
    DEFTET_LAUNCH(k_sf_offsets, dim3((B + 256) / 256), dim3(256), st, (const int *)S.fpos, (const int *)S.vpos, G, (int *)offsets);
    return DEFTET_OK;
}

extern "C" int deftet_voxel_surface_fill_b32(const uint32_t *bits, int B, int R, long long cap_faces, long long cap_verts, float *verts,
                                             int64_t *faces, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_surface(B, R));
    DEFTET_CHECK_ARG(bits, "null pointer: bits");
    DEFTET_CHECK_ARG(cap_faces >= 0 && cap_verts >= 0, "negative capacity");
    DEFTET_CHECK_ARG((cap_faces == 0 || faces) && (cap_verts == 0 || verts), "null pointer: verts / faces");
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, deftet_voxel_surface_workspace_bytes(B, R)));
    hipStream_t st = as_stream(stream_);
    const SurfWs S = surf_carve(workspace, B, R);
    const Grid G{(const unsigned *)bits, B, R, words_of(R), words_of(R + 1)};
    const size_t nf = (size_t)B * R * R * G.W, nv = (size_t)B * (R + 1) * (R + 1) * G.Wc;
    if (cap_faces > 0)
        DEFTET_LAUNCH(k_sf_fill_faces, dim3(blocks_for(nf, kThreads)), dim3(kThreads), st, G, (const int *)S.fpos, (const unsigned *)S.used, (const int *)S.vpos,
                      cap_faces, (long long *)faces);
    if (cap_verts > 0)
        DEFTET_LAUNCH(k_sf_fill_verts, dim3(blocks_for(nv, kThreads)), dim3(kThreads), st, G, (const unsigned *)S.used, (const int *)S.vpos, cap_verts, verts);
    return DEFTET_OK;
}

extern "C" size_t deftet_face_edges_workspace_bytes(int F)
{
    return F <= 0 ? 256 : edge_carve(nullptr, F).total;
}

extern "C" int deftet_face_edges_i32(const int64_t *faces, int F, int V, int32_t *pairs, int32_t *n_out, void *workspace, size_t wsb,
                                     void *stream_)
{
    DEFTET_CHECK_ARG(F >= 0 && F <= 300000000, "n_face=%d outside 0..3e8", F);
    DEFTET_CHECK_ARG(V > 0, "n_vertex=%d must be positive", V);
    DEFTET_CHECK_ARG(n_out, "null pointer: n_out");
    hipStream_t st = as_stream(stream_);
    const EdgeWs S = edge_carve(workspace, F);
    DEFTET_CHECK_ARG(F == 0 || (faces && pairs), "null pointer: faces / pairs");
    if (F > 0) DEFTET_TRY(workspace_ok(__func__, workspace, wsb, S.total));
    DEFTET_HIP(hipMemsetAsync(n_out, 0, 8, st));
    if (F == 0) return DEFTET_OK;
    const size_t n = S.n;
    int bits = 1;
    while (bits < 64 && ((unsigned long long)V * (unsigned long long)V) >> bits) ++bits;       // the sentinel V^2 must sort last
    DEFTET_LAUNCH(k_edge_keys, dim3(blocks_for(n, kThreads)), dim3(kThreads), st, (const long long *)faces, (long long)n, V, S.k0, (int *)n_out);
    DEFTET_TRY(prims::radix_sort_keys<unsigned long long>(S.k0, S.k1, n, bits, S.sort_tmp, S.sort_bytes, st));
    DEFTET_LAUNCH(k_edge_flag, dim3(blocks_for(n + 1, kThreads)), dim3(kThreads), st, (const unsigned long long *)S.k1, (long long)n, V, S.pos);
    DEFTET_TRY(prims::scan<int, prims::Plus, true>(S.pos, S.pos, n + 1, 0, prims::Plus(), S.scan_tmp, S.scan_bytes, st));
    DEFTET_LAUNCH(k_edge_compact, dim3(blocks_for(n + 1, kThreads)), dim3(kThreads), st, (const unsigned long long *)S.k1, (long long)n, V, (const int *)S.pos,
                  (int *)pairs, (int *)n_out);
    return DEFTET_OK;
}
