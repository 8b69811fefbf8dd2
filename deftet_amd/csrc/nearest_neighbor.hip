// nearest_neighbor.hip — the nearest-neighbour index layers.DefTet.forward calls per shape
// for CDNA4 / gfx950; what it shares with the other surface operators is in surface_batch.hpp.
//   A10 deftet_nn_index_f32        layers/nearest_neighbor/nearest_neighbor_cuda.cu:15-80
#pragma clang fp contract(off)
#include "common.hpp"
#include "grid_setup.hpp"
#include "prims.hpp"
#include "surface_batch.hpp"

namespace deftet {
namespace surf {

// ---------------------------------------------------------------------------- A10 nearest neighbour
// the squared distance as the reference accumulates it
__device__ __forceinline__ float nn_dist(float px, float py, float pz, float qx, float qy, float qz)
{
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    float d = 0.f;
    d += dx * dx;                                                   // nearest_neighbor_cuda.cu:42
    d += dy * dy;                                                   // :44
    d += dz * dz;                                                   // :46
    return d;
}

// result = index of the first point with the strictly smallest ((dx*dx + dy*dy) + dz*dz)
__global__ __launch_bounds__(256) void k_nn(const float *__restrict__ queries, const float *__restrict__ points, int N,
                                            int M, int *result)
{
    const int b = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = q < N;
    const float *qq = queries + ((size_t)b * N + (live ? q : 0)) * 3;
    const float qx = qq[0], qy = qq[1], qz = qq[2];
    const float *__restrict__ pp = points + (size_t)b * M * 3;      // wave-uniform stream -> s_load
    float best = 1e20f;                                             // nearest_neighbor_cuda.cu:28
    int besti = 0;
    int i = 0;
    for (; i + 4 <= M; i += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = nn_dist(pp[(i + k) * 3], pp[(i + k) * 3 + 1], pp[(i + k) * 3 + 2], qx, qy, qz);
            if (d < best) { best = d; besti = i + k; }              // :48-51
        }
    }
    for (; i < M; ++i) {
        const float d = nn_dist(pp[i * 3], pp[i * 3 + 1], pp[i * 3 + 2], qx, qy, qz);
        if (d < best) { best = d; besti = i; }
    }
    if (live) result[(size_t)b * N + q] = besti;
}

// --- A10, grid-accelerated (exact) -------------------------------------------------------------------
// Points are counting-sorted into a uniform G^3 grid over their bounding box; a query walks the
// cell shells around its own (virtual) cell in increasing Chebyshev radius r and stops as soon as
// the best distance found is smaller than a certified lower bound for everything outside the
// shell box.  Distances are evaluated exactly as the reference does, and candidates are combined
// lexicographically (distance, index), which equals "first strict minimum of an ascending scan".
constexpr int kNNBlocks = 64;

constexpr int kNNCoarse = 4;           // coarse cells are 4x4x4 fine cells
struct NNGrid { float o[3], inv[3], cs[3], slack[3]; int G, Gc; };

// (the same launch clears what the later kernels accumulate into: cell counters, coarse-cell representatives, nRep)
__global__ __launch_bounds__(256) void k_nn_bbox(const float *__restrict__ pts, int M, float *part, size_t slice, int *cells, int *rep,
                                                 int *nRep, int nc)
{
    __shared__ float sh[4][6];
    const int sb = blockIdx.y;
    pts += (size_t)sb * M * 3;
    SHAPE(part); SHAPE(cells); SHAPE(rep); SHAPE(nRep);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc; i += gridDim.x * blockDim.x) { cells[i] = 0; rep[i] = -1; }
    if (blockIdx.x == 0 && threadIdx.x < 4) nRep[threadIdx.x] = 0;
    BoxStats<3, 0> bs;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const float p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
        if (fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY) bs.add_point(p);     // finite (NaN fails)
    }
    bs.block_store(sh, part + blockIdx.x * 6);
}

__global__ __launch_bounds__(64) void k_nn_grid(const float *__restrict__ part, int G, NNGrid *g, size_t slice)
{
    const int sb = blockIdx.x;
    SHAPE(part); SHAPE(g);
    const int lane = threadIdx.x;
    BoxStats<3, 0> bs;
    bs.load(part + lane * 6);
    bs.wave_reduce();
    if (lane == 0) {
        NNGrid r;
        r.G = G;
        r.Gc = (G + kNNCoarse - 1) / kNNCoarse;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool ok = bs.hi[k] >= bs.lo[k];
            const float l = ok ? bs.lo[k] : 0.f, h = ok ? bs.hi[k] : 0.f;
            const float ext = h - l;
            r.o[k] = l;
            const bool flat = !(ext > 1e-30f) || !(ext < 1e30f);
            r.inv[k] = flat ? 0.f : (float)G / ext;
            r.cs[k] = flat ? INFINITY : ext / (float)G;          // cell size (inf: one slab, no bound on this axis)
            // absolute uncertainty of a cell boundary position as seen through the fp32 cell assignment
            r.slack[k] = 8e-6f * (fabsf(l) + fabsf(h)) + 1e-30f;
        }
        *g = r;
    }
}

__global__ __launch_bounds__(256) void k_nn_bin(const float *__restrict__ pts, int M, const NNGrid *__restrict__ gp, int *cells,
                                                int2 *pcell, int *rep, size_t slice)
{
    const int sb = blockIdx.y;
    pts += (size_t)sb * M * 3;
    SHAPE(gp); SHAPE(cells); SHAPE(pcell); SHAPE(rep);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < M;                                       // (no early return: run_atomic_rank is a wave operation)
    const NNGrid g = *gp;
    const int ii = live ? i : 0;
    const float x = pts[ii * 3], y = pts[ii * 3 + 1], z = pts[ii * 3 + 2];
    int2 r = make_int2(-1, 0);
    int cx = 0, cy = 0, cz = 0;
    if (live && fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY) {
        cx = grid_cell(x, g.o[0], g.inv[0], g.G); cy = grid_cell(y, g.o[1], g.inv[1], g.G); cz = grid_cell(z, g.o[2], g.inv[2], g.G);
        r.x = (cz * g.G + cy) * g.G + cx;
    }
    r.y = run_atomic_rank(cells, r.x);
    // any point of the coarse cell will do as its representative: the first arrival of every fine cell offers itself
    // (one atomic per occupied fine cell — one per POINT put hundreds of them on the same address: 0.33 ms per 8 shapes)
    if (r.x >= 0 && r.y == 0) atomicMax(&rep[((cz / kNNCoarse) * g.Gc + cy / kNNCoarse) * g.Gc + cx / kNNCoarse], i);
    if (live) pcell[i] = r;                                        // non-finite points can never be nearest (d is inf/NaN)
}

__global__ __launch_bounds__(256) void k_nn_scatter(const float *__restrict__ pts, int M, const int2 *__restrict__ pcell,
                                                    const int *__restrict__ start, float4 *sorted, size_t slice)
{
    const int sb = blockIdx.y;
    pts += (size_t)sb * M * 3;
    SHAPE(pcell); SHAPE(start); SHAPE(sorted);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int2 r = pcell[i];
    if (r.x < 0) return;
    sorted[start[r.x] + r.y] = make_float4(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], __int_as_float(i));
}

// Sort key of the queries k_nn_query answered itself: the first power of two above every Morton key of the grid (three
// interleaved coordinates 0..G+1), so that the far queries sort to the front on 3*bits + 1 key bits (16 for G <= 30).
static int nn_far_key_bits(int G)
{
    int bits = 1;
    while ((1 << bits) < G + 2) ++bits;
    return 3 * bits;
}
constexpr int kFarRows = 25;

__device__ __forceinline__ unsigned spread3(unsigned v)            // bit i of an 8-bit value -> bit 3i
{
    v = (v | (v << 8)) & 0x0000F00Fu;
    v = (v | (v << 4)) & 0x000C30C3u;
    v = (v | (v << 2)) & 0x00249249u;
    return v;
}

// Two phases per query (one lane each):
//  1. an UPPER bound U on the nearest distance from the coarse grid: shells of coarse cells are
//     searched until one holds a representative point; U = smallest exact distance to those;
//  2. every fine-grid row (cz,cy) whose slab can intersect the ball of radius sqrt(U) is visited
//     once: the x-interval of the ball in that row is one contiguous slice of the sorted points.
// All points with fp32 distance <= U lie in the enumerated slices (margins below), so the
// lexicographic (distance, index) minimum over them equals the reference's ascending scan.
__global__ __launch_bounds__(256) void k_nn_query(const float *__restrict__ queries, int N, const NNGrid *__restrict__ gp,
                                                  const int *__restrict__ start, const float4 *__restrict__ sorted,
                                                  const int *__restrict__ rep, const float *__restrict__ pts, int M, int *result,
                                                  unsigned *farKey, unsigned notFar, size_t slice, ShapeCounts cnt, int Nst,
                                                  unsigned shapeShift)
{
    // N = the query stride; shape sb has cnt.n[sb] <= N queries.  farKey is ONE array of Nst keys per shape (not in the
    // slices: the far keys of all shapes are sorted by one call, with the shape index above the key bits).
    const int sb = blockIdx.y;
    queries += (size_t)sb * N * 3; pts += (size_t)sb * M * 3; result += (size_t)sb * N; farKey += (size_t)sb * Nst;
    SHAPE(gp); SHAPE(start); SHAPE(sorted); SHAPE(rep);
    const unsigned shapeBits = (unsigned)sb << shapeShift;
    notFar |= shapeBits;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnt.n[sb]) {
        if (q < Nst) farKey[q] = notFar;                            // padding keys sort behind the shape's far queries
        return;
    }
    const NNGrid g = *gp;
    const int G = g.G, Gc = g.Gc;
    const float qx = queries[q * 3], qy = queries[q * 3 + 1], qz = queries[q * 3 + 2];
    const float qq[3] = {qx, qy, qz};
    farKey[q] = notFar;
    if (!(fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY)) { result[q] = 0; return; }   // every d is inf/NaN
    // a far query is keyed by the Morton code of its (clamped) fine cell: sorted by it, the lanes of k_nn_far are neighbours
    auto far_key = [&]() {
        unsigned key = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float f = floorf((qq[k] - g.o[k]) * g.inv[k]);
            f = fminf(fmaxf(f, -1.f), (float)G) + 1.f;              // 0 .. G+1 <= 161: eight bits
            key |= spread3((unsigned)f) << k;
        }
        return key;
    };
    auto dist = [&](float px, float py, float pz) { return nn_dist(px, py, pz, qx, qy, qz); };
    // ---- phase 0: tight upper bound from the 3x3x3 fine cells around the query (near queries)
    float U = INFINITY;
    {
        int c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float f = floorf((qq[k] - g.o[k]) * g.inv[k]);
            f = fminf(fmaxf(f, -2.f), (float)(G + 1));
            c[k] = (int)f;
        }
        const int x0 = max(c[0] - 1, 0), x1 = min(c[0] + 1, G - 1);
        if (x0 <= x1)
            for (int cz = max(c[2] - 1, 0); cz <= min(c[2] + 1, G - 1); ++cz)
                for (int cy = max(c[1] - 1, 0); cy <= min(c[1] + 1, G - 1); ++cy) {
                    const int row = (cz * G + cy) * G;
                    const int s = start[row + x0], e = start[row + x1 + 1];
                    for (int j = s; j < e; j += 4) {
                        float4 p[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) p[k] = sorted[min(j + k, e - 1)];
#pragma unroll
                        for (int k = 0; k < 4; ++k) U = fminf(U, dist(p[k].x, p[k].y, p[k].z));
                    }
                }
    }
    // ---- phase 1: otherwise a loose bound from the coarse grid (one representative point per 4^3 cells)
    int cc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float f = floorf((qq[k] - g.o[k]) * g.inv[k] * (1.0f / kNNCoarse));
        f = fminf(fmaxf(f, -1.f), (float)Gc);
        cc[k] = (int)f;
    }
    constexpr int kCoarseRings = 1;                                  // beyond that the query is "far": streaming scan
    for (int r = 0; r <= kCoarseRings && !(U < INFINITY); ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cc[2] + dz;
            if (z < 0 || z >= Gc) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cc[1] + dy;
                if (y < 0 || y >= Gc) continue;
                const bool face = max(abs(dz), abs(dy)) == r;
                for (int dx = -r; dx <= r; dx += (face ? 1 : (r > 0 ? 2 * r : 1))) {
                    const int x = cc[0] + dx;
                    if (x < 0 || x >= Gc) continue;
                    const int i = rep[(z * Gc + y) * Gc + x];
                    if (i >= 0) U = fminf(U, dist(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]));
                }
            }
        }
    }
    float best = 1e20f;                                             // :28
    int besti = 0;
    if (!(U < INFINITY)) {                                           // nothing within one coarse ring: far (or no finite point)
        farKey[q] = far_key() | shapeBits;
        return;
    }
    U = fminf(U, 1e20f);                                            // nothing farther than the initial best can win
    // ---- phase 2: rows intersecting the ball of radius R (inflated for fp32 rounding of d and of the cell map)
    const float R = sqrtf(U) * 1.00001f;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = grid_cell(qq[k] - R - g.slack[k], g.o[k], g.inv[k], G);
        hi[k] = grid_cell(qq[k] + R + g.slack[k], g.o[k], g.inv[k], G);
    }
    const float R2 = R * R;
    // A query whose ball spans many cell rows pays a dependent lookup per row and gathers points at
    // ~4x the per-point cost of a wave-uniform stream: hand it to the k_nn_far_* kernels.  (Threshold measured on 80k
    // queries against 100k points on a sphere: uniform queries 1.03 / 1.39 / 2.66 ms for 9 / 25 / 100 rows; queries sampled
    // on a nearby surface 0.59 / 0.47 / 0.47 ms — the far path has ~0.15 ms of dependent-load latency of its own.)
    if ((long long)(hi[2] - lo[2] + 1) * (hi[1] - lo[1] + 1) > kFarRows) {
        farKey[q] = far_key() | shapeBits;
        return;
    }
    for (int cz = lo[2]; cz <= hi[2]; ++cz) {
        const float dz = slab_dist(g, 2, cz, qz);
        for (int cy = lo[1]; cy <= hi[1]; ++cy) {
            const float dy = slab_dist(g, 1, cy, qy);
            const float rem = R2 - dy * dy - dz * dz;
            if (rem < 0.f) continue;                                 // the whole row is farther than R
            const float rx = sqrtf(rem) * 1.00001f;
            const int x0 = grid_cell(qx - rx - g.slack[0], g.o[0], g.inv[0], G), x1 = grid_cell(qx + rx + g.slack[0], g.o[0], g.inv[0], G);
            const int row = (cz * G + cy) * G;
            const int s = start[row + x0], e = start[row + x1 + 1];
            for (int j = s; j < e; j += 4) {                         // four gathers in flight per lane
                float4 p[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) p[k] = sorted[min(j + k, e - 1)];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = dist(p[k].x, p[k].y, p[k].z);
                    const int idx = __float_as_int(p[k].w);
                    if (j + k < e && (d < best || (d == best && idx < besti && best < 1e20f))) { best = d; besti = idx; }
                }
            }
        }
    }
    result[q] = besti;
}

// compact helper tables for k_nn_far: the representatives as (x, y, z, index) records and the first sorted slot of
// every cell row; both padded so that k_nn_far can read them eight entries at a time
__global__ __launch_bounds__(256) void k_nn_far_tables(const int *__restrict__ rep, const float *__restrict__ pts, int Gc3,
                                                       const int *__restrict__ start, int G, float4 *repList, int *nRep,
                                                       int *rowStart, float4 *sorted, size_t slice, int M)
{
    const int sb = blockIdx.y;
    pts += (size_t)sb * M * 3;
    SHAPE(rep); SHAPE(start); SHAPE(repList); SHAPE(nRep); SHAPE(rowStart); SHAPE(sorted);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Gc3) {
        const int r = rep[i];
        const unsigned long long m = __ballot(r >= 0);
        int base = 0;
        if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(nRep, __popcll(m));
        base = __shfl(base, 0);
        if (r >= 0)
            repList[base + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull))] =
                make_float4(pts[r * 3], pts[r * 3 + 1], pts[r * 3 + 2], __int_as_float(r));
    }
    const int total = start[G * G * G];
    if (i < G * G + 2 * kNNBatch) rowStart[i] = i < G * G ? start[i * G] : total;
    if (i < 64) sorted[total + i] = make_float4(INFINITY, INFINITY, INFINITY, 0.f);   // tile padding (never considered)
}

__global__ __launch_bounds__(64) void k_nn_far_pad(float4 *repList, const int *__restrict__ nRep, size_t slice)
{
    const int sb = blockIdx.x;
    SHAPE(repList); SHAPE(nRep);
    repList[*nRep + threadIdx.x] = make_float4(INFINITY, INFINITY, INFINITY, 0.f);   // tile padding (64 threads)
}

// Far queries (answer farther than one coarse ring, or a ball over more than kFarRows cell rows).  One lane per query,
// the queries SORTED by the Morton code of their cell so that a wave holds 64 neighbours, and everything a wave reads
// is wave-uniform (scalar loads, eight records per batch, points as SGPR operands — the vector memory pipe is idle):
//   k_nn_far_bound  A. every coarse cell's representative point bounds the answer from above;
//                   B. the points of the coarse cells holding the lanes' best representatives tighten the bound;
//   k_nn_far_rows   C. the cell rows (cz,cy) are visited; a row is skipped when its slab is farther than the current
//                      best of EVERY lane (same certified margins as k_nn_query), otherwise the x-range the lanes can
//                      still need is streamed;
//   k_nn_far_final  scatters the answers back to query order.
// Any point is a valid candidate for any lane (reading a few records past a row's end is harmless), and candidates are
// combined as the 64-bit word (distance bits, index) under min — distances are non-negative, so that is the
// lexicographic (distance, index) minimum = the reference's first strict minimum of an ascending scan — first in
// registers, then across the four waves of a block in LDS, then across blocks with one atomicMin per lane.
// A group of 64 queries at the centre of a sphere needs every point: 6.4 M distance evaluations that must not land on
// one CU, so the rows of every group are split over kFarSlices blocks.
// (Measured history, 80,640 uniform queries against 100,000 points on a sphere, plain scan 5.5 ms: far list appended
// with one same-address atomic per query and every far query scanning ALL points 7.2 ms; pruned rows, one wave per 64
// queries, one scalar load per record 14.3 ms; batches of eight and 4 / 16 waves per group 4.5 / 2.4 ms; A and B shared
// between the waves 1.55 ms — the group that needs every point then kept one CU busy for 1 ms.)
constexpr int kFarSlices = 8;            // blocks per group of 64 far queries in k_nn_far_rows
constexpr int kFarWaves = 4;            // waves per block; they split the block's records

struct FarLane {
    float qx, qy, qz, best;
    int besti;
    __device__ __forceinline__ void consider(const float4 p)
    {
        const float d = nn_dist(p.x, p.y, p.z, qx, qy, qz);
        const int idx = __float_as_int(p.w);
        if (d < best || (d == best && idx < besti && best < 1e20f)) { best = d; besti = idx; }
    }
    // records [s, e) of a wave-uniform table (and up to seven more: the tables are padded with d = inf records)
    __device__ __forceinline__ void stream(const float4 *__restrict__ src, int s, int e)
    {
        for (int j = s; j < e; j += kNNBatch) {
            float4 p[kNNBatch];
#pragma unroll
            for (int k = 0; k < kNNBatch; ++k) p[k] = src[j + k];
#pragma unroll
            for (int k = 0; k < kNNBatch; ++k) consider(p[k]);
        }
    }
};

// (keys carry the shape index above the key bits: within a shape's segment the comparison with its own notFar is the same)
__device__ __forceinline__ int far_count(const unsigned *__restrict__ farKeyS, int N, unsigned notFar)
{
    int lo = 0, hi = N;                                            // first sorted key == notFar
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (farKeyS[mid] < notFar) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kFarWaves * 64) void k_nn_far_bound(const float *__restrict__ queries, const NNGrid *__restrict__ gp,
                                                                 const int *__restrict__ start, const float4 *__restrict__ sorted,
                                                                 const float4 *__restrict__ repList, const int *__restrict__ nRepP,
                                                                 const float *__restrict__ pts, int N,
                                                                 const unsigned *__restrict__ farKeyS, const unsigned *__restrict__ farList,
                                                                 unsigned long long *bound, int *nFar, unsigned notFar, size_t slice,
                                                                 int M, int Nst, unsigned shapeShift)
{
    __shared__ unsigned long long s_pack[kFarWaves][64];
    const int sb = blockIdx.y;
    queries += (size_t)sb * N * 3; pts += (size_t)sb * M * 3; farKeyS += (size_t)sb * Nst; farList += (size_t)sb * Nst;
    SHAPE(gp); SHAPE(start); SHAPE(sorted); SHAPE(repList); SHAPE(nRepP); SHAPE(bound); SHAPE(nFar);
    const unsigned qbase = (unsigned)sb * (unsigned)Nst;            // farList holds positions in the all-shapes key array
    const int n = far_count(farKeyS, Nst, notFar | ((unsigned)sb << shapeShift));
    if (blockIdx.x == 0 && threadIdx.x == 0) *nFar = n;
    const int lane = threadIdx.x & 63;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform for the compiler too: scalar loads below
    const int i = blockIdx.x * 64 + lane;
    if (blockIdx.x * 64 >= n) return;                              // whole block idle
    const int q = (int)(farList[i < n ? i : n - 1] - qbase);        // idle lanes shadow the last far query
    const NNGrid g = *gp;
    const int G = g.G, Gc = g.Gc;
    FarLane L;
    L.qx = queries[q * 3]; L.qy = queries[q * 3 + 1]; L.qz = queries[q * 3 + 2];
    L.best = 1e20f;                                                 // nearest_neighbor_cuda.cu:28
    L.besti = 0;
    // ---- A: representatives, one batch per wave and turn
    {
        const int nRep = *nRepP;
        for (int j = part * kNNBatch; j < nRep; j += kFarWaves * kNNBatch) L.stream(repList, j, j + kNNBatch);
    }
    share_best<kFarWaves>(s_pack, part, lane, L.best, L.besti);
    // ---- B: the coarse cells of the lanes' best representatives (at most four distinct ones per block); a coarse cell
    //         is 4 x 4 rows of four cells: four rows per wave
    {
        const bool have = L.best < 1e20f;
        const int bi = have ? L.besti : 0;
        const float bx = pts[bi * 3], by = pts[bi * 3 + 1], bz = pts[bi * 3 + 2];
        const int mine = ((grid_cell(bz, g.o[2], g.inv[2], G) / kNNCoarse) * Gc + grid_cell(by, g.o[1], g.inv[1], G) / kNNCoarse) * Gc +
                         grid_cell(bx, g.o[0], g.inv[0], G) / kNNCoarse;
        unsigned long long todo = __ballot(have);
        for (int round = 0; round < 4 && todo; ++round) {
            const int c = __builtin_amdgcn_readlane(mine, __ffsll((long long)todo) - 1);
            todo &= ~__ballot(mine == c);
            const int x0 = (c % Gc) * kNNCoarse, x1 = min(x0 + kNNCoarse - 1, G - 1);
            const int cy0 = ((c / Gc) % Gc) * kNNCoarse, cz = (c / (Gc * Gc)) * kNNCoarse + part;
            int se[2 * kNNCoarse];
#pragma unroll
            for (int k = 0; k < kNNCoarse; ++k) {
                const int row = (min(cz, G - 1) * G + min(cy0 + k, G - 1)) * G;
                se[2 * k] = start[row + x0]; se[2 * k + 1] = start[row + x1 + 1];
            }
#pragma unroll
            for (int k = 0; k < kNNCoarse; ++k)
                if (cz < G && cy0 + k < G) L.stream(sorted, se[2 * k], se[2 * k + 1]);
        }
    }
    share_best<kFarWaves>(s_pack, part, lane, L.best, L.besti);
    if (part == 0 && i < n) bound[i] = pack_best(L.best, L.besti);
}

__global__ __launch_bounds__(kFarWaves * 64) void k_nn_far_rows(const float *__restrict__ queries, const NNGrid *__restrict__ gp,
                                                                const int *__restrict__ start, const float4 *__restrict__ sorted,
                                                                const int *__restrict__ rowStart, const int *__restrict__ nFar,
                                                                const unsigned *__restrict__ farList, unsigned long long *bound,
                                                                size_t slice, int N, int Nst)
{
    __shared__ unsigned long long s_pack[kFarWaves][64];
    const int sb = blockIdx.z;
    queries += (size_t)sb * N * 3; farList += (size_t)sb * Nst;
    SHAPE(gp); SHAPE(start); SHAPE(sorted); SHAPE(rowStart); SHAPE(nFar); SHAPE(bound);
    const unsigned qbase = (unsigned)sb * (unsigned)Nst;
    const int n = *nFar;
    const int lane = threadIdx.x & 63;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 64 + lane;
    if (blockIdx.x * 64 >= n) return;                              // whole block idle
    const int ii = i < n ? i : n - 1;                              // idle lanes shadow the last far query
    const int q = (int)(farList[ii] - qbase);
    const NNGrid g = *gp;
    const int G = g.G;
    FarLane L;
    L.qx = queries[q * 3]; L.qy = queries[q * 3 + 1]; L.qz = queries[q * 3 + 2];
    unpack_best(bound[ii], L.best, L.besti);                       // as k_nn_far_bound left it (other slices may have improved it)
    const int nb = (G + kNNBatch - 1) / kNNBatch;                   // work item = (layer cz, batch of eight rows cy0..cy0+7)
    for (int item = blockIdx.y * kFarWaves + part; item < G * nb; item += kFarWaves * kFarSlices) {
        const int cz = item / nb, cy0 = (item % nb) * kNNBatch;
        const float dz = slab_dist(g, 2, cz, L.qz);
        if (!__any(!(L.best * 1.00003f - dz * dz < 0.f))) continue; // the whole layer is out of reach of every lane
        int rs[kNNBatch + 1];
#pragma unroll
        for (int k = 0; k <= kNNBatch; ++k) rs[k] = rowStart[cz * G + cy0 + k];   // padded: reads past G*G return the total
        // first the slice [s, e) of each of the eight rows that some lane can still need (lane k of vs/ve keeps row k's;
        // the eight pairs of cell-start loads are independent), then ONE copy of the streaming loop walks them
        int vs = 0, ve = 0;
#pragma unroll
        for (int k = 0; k < kNNBatch; ++k) {
            const int cy = cy0 + k;
            int s = 0, e = 0;
            if (cy < G && rs[k] != rs[k + 1]) {
                const float dy = slab_dist(g, 1, cy, L.qy);
                // squared reach, inflated for the fp32 rounding of d and of the cell map (k_nn_query: R = sqrt(U) * 1.00001)
                const float rem = L.best * 1.00003f - dy * dy - dz * dz;
                const bool need = !(rem < 0.f);
                if (__any(need)) {
                    s = rs[k]; e = rs[k + 1];
                    if (e - s > 3 * kNNBatch) {                     // long row: only the x-range the lanes can reach
                        const float rx = sqrtf(fmaxf(rem, 0.f)) * 1.00001f;
                        int x0 = need ? grid_cell(L.qx - rx - g.slack[0], g.o[0], g.inv[0], G) : G - 1;
                        int x1 = need ? grid_cell(L.qx + rx + g.slack[0], g.o[0], g.inv[0], G) : 0;
                        if (need && !(rx < INFINITY)) { x0 = 0; x1 = G - 1; }
#pragma unroll  // wave_min's and wave_max's order (wave.hpp); written out, a call changes this kernel's instruction stream
                        for (int off = 32; off > 0; off >>= 1) {
                            x0 = min(x0, __shfl_xor(x0, off));
                            x1 = max(x1, __shfl_xor(x1, off));
                        }
                        x0 = __builtin_amdgcn_readfirstlane(x0);
                        x1 = __builtin_amdgcn_readfirstlane(x1);
                        const int row = (cz * G + cy) * G;
                        s = start[row + x0]; e = start[row + x1 + 1];
                    }
                }
            }
            vs = lane == k ? s : vs;
            ve = lane == k ? e : ve;
        }
#pragma unroll 1
        for (int k = 0; k < kNNBatch; ++k) L.stream(sorted, __builtin_amdgcn_readlane(vs, k), __builtin_amdgcn_readlane(ve, k));
    }
    share_best<kFarWaves>(s_pack, part, lane, L.best, L.besti);
    if (part == 0 && i < n) atomicMin(&bound[i], pack_best(L.best, L.besti));
}

__global__ __launch_bounds__(256) void k_nn_far_final(const unsigned long long *__restrict__ bound, const int *__restrict__ nFar,
                                                      const unsigned *__restrict__ farList, int *result, size_t slice, int N, int Nst)
{
    const int sb = blockIdx.y;
    farList += (size_t)sb * Nst; result += (size_t)sb * N;
    SHAPE(bound); SHAPE(nFar);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < *nFar) result[farList[i] - (unsigned)sb * (unsigned)Nst] = (int)(unsigned)bound[i];
}

}  // namespace surf
}  // namespace deftet

using namespace deftet;
using namespace deftet::surf;

static int nn_pick_G(int M)
{
    // 1.5x the cells per axis that ~4 points per cell of a VOLUME-filling cloud would give (round 2): the clouds of this
    // operator are surface samples, which leaves ~10 points in an occupied cell (round 2: ~35, and the 3x3x3 neighbourhood
    // every query scans first held ~300 points).  Measured on the geometry step (8 x 97 k points, 8 x 80 k queries):
    // 3.49 / 3.32 / 3.27 / 3.22 ms per step at 1 / 1.4 / 1.8 / 2.4 x; a single shape (one call, 80 k queries) 0.32 / 0.29 /
    // 0.41 / 0.39 ms — finer grids cost a lone call more in rows visited per query than they save in points per row.
    int G = (int)llround(1.5 * cbrt((double)(M > 0 ? M : 1) / 4.0));
    if (G < 1) G = 1;
    if (G > 160) G = 160;
    return G;
}

// The grid search's workspace for a launch group of nS shapes: one slice of per-shape scratch per shape (the members point into
// slice 0; the kernels rebase to their shape by `slice` bytes), and behind the slices the far keys / sorted keys / iota / sorted
// positions of ALL shapes of the group with the sort's temporary.
struct NNLayout {
    size_t slice, bytes, sortTmpBytes;
    float *part;
    NNGrid *grid;
    int *cells, *start, *rep;
    int2 *pcell;
    float4 *sorted, *repList;
    int *rowStart, *nRep;
    unsigned long long *bound;
    int *nFar;
    unsigned *farKey, *farKeyS, *iota, *farList;
    void *sortTmp;
};
static NNLayout nn_layout(int nS, int N, int M, void *ws)
{
    NNLayout L{};
    const int G = nn_pick_G(M);
    const size_t nc = (size_t)G * G * G + 1, Nn = (size_t)(N > 0 ? N : 0), Mn = (size_t)(M > 0 ? M : 0);
    Arena A(ws);
    L.part = A.take<float>(kNNBlocks * 6);
    L.grid = A.take<NNGrid>(1);
    L.cells = A.take<int>(nc); L.start = A.take<int>(nc); L.rep = A.take<int>(nc);
    L.pcell = A.take<int2>(Mn);
    L.sorted = A.take<float4>(Mn + 64);                                               // k_nn_far reads whole 64-record tiles
    L.repList = A.take<float4>(nc / (kNNCoarse * kNNCoarse) + 64 + 64);               // >= Gc^3 + pad
    L.rowStart = A.take<int>((size_t)G * G + 2 * kNNBatch); L.nRep = A.take<int>(4);
    L.bound = A.take<unsigned long long>(Nn + 1);
    L.nFar = A.take<int>(4);
    L.slice = A.end();
    const size_t nAll = (size_t)nS * (Nn + 1);
    Arena T(static_cast<char *>(ws) + L.slice * nS);
    L.farKey = T.take<unsigned>(nAll); L.farKeyS = T.take<unsigned>(nAll); L.iota = T.take<unsigned>(nAll); L.farList = T.take<unsigned>(nAll);
    L.sortTmpBytes = prims::radix_sort_temp_bytes<unsigned, unsigned>(nAll);
    L.sortTmp = T.take<char>(L.sortTmpBytes);
    L.bytes = L.slice * nS + T.end();
    return L;
}
extern "C" size_t deftet_nn_index_workspace_bytes(int B, int N, int M) { return nn_layout(group_shapes(B), N, M, nullptr).bytes; }

__global__ __launch_bounds__(256) void k_iota(unsigned *v, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (unsigned)i;
}

// the grid search for a GROUP of nS <= kBatchShapes shapes: one launch per kernel for the whole group
static int nn_group(const float *queries, const float *points, int32_t *result, int nS, int N, int M, const ShapeCounts &cnt, void *ws,
                    hipStream_t st)
{
    const int G = nn_pick_G(M), keyBits = nn_far_key_bits(G);
    const size_t nc = (size_t)G * G * G + 1;
    int nmax = 0;
    for (int i = 0; i < nS; ++i) nmax = std::max(nmax, cnt.n[i]);
    if (nmax == 0) return DEFTET_OK;
    const NNLayout L = nn_layout(nS, N, M, ws);                       // at most what nn_index_impl checked: a group is no larger than the largest
    const size_t slice = L.slice;
    const int Nst = N + 1;
    const size_t nAll = (size_t)nS * Nst;
    const unsigned shapeShift = (unsigned)keyBits + 1;
    const dim3 blk(256);
    DEFTET_LAUNCH(k_nn_bbox, dim3(kNNBlocks, nS), blk, st, points, M, L.part, slice, L.cells, L.rep, L.nRep, (int)nc);
    DEFTET_LAUNCH(k_nn_grid, dim3(nS), dim3(64), st, (const float *)L.part, G, L.grid, slice);
    DEFTET_LAUNCH(k_nn_bin, dim3(blocks_for(M, 256), nS), blk, st, points, M, (const NNGrid *)L.grid, L.cells, L.pcell, L.rep, slice);
    DEFTET_LAUNCH(k_scan_excl, dim3(scan_tiles(nc), nS), dim3(kScanThreads), st, (const int *)L.cells, L.start, (int)nc, slice, 0);
    DEFTET_LAUNCH(k_nn_scatter, dim3(blocks_for(M, 256), nS), blk, st, points, M, (const int2 *)L.pcell, (const int *)L.start, L.sorted, slice);
    DEFTET_LAUNCH(k_nn_query, dim3(blocks_for(Nst, 256), nS), blk, st, queries, N, (const NNGrid *)L.grid, (const int *)L.start,
                  (const float4 *)L.sorted, (const int *)L.rep, points, M, result, L.farKey, 1u << keyBits, slice, cnt, Nst, shapeShift);
    DEFTET_LAUNCH(k_iota, dim3(blocks_for(nAll, 256)), blk, st, L.iota, (long long)nAll);
    int shapeBitsN = 0;
    while ((1 << shapeBitsN) < nS) ++shapeBitsN;
    DEFTET_TRY(prims::radix_sort<unsigned, unsigned>(L.farKey, L.farKeyS, L.iota, reinterpret_cast<unsigned *>(L.farList), nAll,
                                                     keyBits + 1 + shapeBitsN, L.sortTmp, L.sortTmpBytes, st));
    const int Gc = (G + kNNCoarse - 1) / kNNCoarse, Gc3 = Gc * Gc * Gc, nt = std::max(Gc3, G * G + 2 * kNNBatch);
    DEFTET_LAUNCH(k_nn_far_tables, dim3(blocks_for(nt, 256), nS), blk, st, (const int *)L.rep, points, Gc3, (const int *)L.start, G, L.repList, L.nRep,
                  L.rowStart, L.sorted, slice, M);
    DEFTET_LAUNCH(k_nn_far_pad, dim3(nS), dim3(64), st, L.repList, (const int *)L.nRep, slice);
    DEFTET_LAUNCH(k_nn_far_bound, dim3(blocks_for(nmax, 64), nS), dim3(kFarWaves * 64), st, queries, (const NNGrid *)L.grid, (const int *)L.start,
                  (const float4 *)L.sorted, (const float4 *)L.repList, (const int *)L.nRep, points, N, (const unsigned *)L.farKeyS,
                  (const unsigned *)L.farList, L.bound, L.nFar, 1u << keyBits, slice, M, Nst, shapeShift);
    DEFTET_LAUNCH(k_nn_far_rows, dim3(blocks_for(nmax, 64), kFarSlices, nS), dim3(kFarWaves * 64), st, queries, (const NNGrid *)L.grid,
                  (const int *)L.start, (const float4 *)L.sorted, (const int *)L.rowStart, (const int *)L.nFar, (const unsigned *)L.farList, L.bound, slice,
                  N, Nst);
    DEFTET_LAUNCH(k_nn_far_final, dim3(blocks_for(nmax, 256), nS), blk, st, (const unsigned long long *)L.bound, (const int *)L.nFar,
                  (const unsigned *)L.farList, result, slice, N, Nst);
    return DEFTET_OK;
}

// n_query_host == NULL: every shape has N queries.  Otherwise shape b has n_query_host[b] <= N queries (rows beyond
// that are left untouched); the counts are HOST integers (the caller knows its face counts), strides stay N.
static int nn_index_impl(const float *queries, const float *points, int32_t *result, int B, int N, int M, const int *n_query_host,
                         void *workspace, size_t wsb, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && N >= 0 && M >= 0 && B <= 65535, "bad size");
    if (B == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(queries && result && (M == 0 || points), "null pointer");
    DEFTET_CHECK_ARG((long long)M * 3 < 2147483647LL && (long long)N * 3 < 2147483647LL, "too many points per shape");
    if (n_query_host)
        for (int b = 0; b < B; ++b) DEFTET_CHECK_ARG(n_query_host[b] >= 0 && n_query_host[b] <= N, "n_query[%d]=%d outside [0,%d]", b, n_query_host[b], N);
    hipStream_t st = as_stream(stream_);
    if (!workspace || M == 0) {
        if (!n_query_host) {
            DEFTET_LAUNCH(k_nn, dim3(blocks_for(N, 256), B), dim3(256), st, queries, points, N, M, result);
        } else {
            for (int b = 0; b < B; ++b)
                if (n_query_host[b] > 0)
                    DEFTET_LAUNCH(k_nn, dim3(blocks_for(n_query_host[b], 256), 1), dim3(256), st, queries + (size_t)b * N * 3, points + (size_t)b * M * 3,
                                  n_query_host[b], M, result + (size_t)b * N);
        }
        return DEFTET_OK;
    }
    DEFTET_TRY(workspace_ok("deftet_nn_index*", workspace, wsb, nn_layout(group_shapes(B), N, M, workspace).bytes));
    for (int b0 = 0; b0 < B; b0 += kBatchShapes) {                   // groups of kBatchShapes shapes reuse the workspace (stream order)
        const int nS = std::min(kBatchShapes, B - b0);
        ShapeCounts cnt{};
        for (int i = 0; i < nS; ++i) cnt.n[i] = n_query_host ? n_query_host[b0 + i] : N;
        DEFTET_TRY(nn_group(queries + (size_t)b0 * N * 3, points + (size_t)b0 * M * 3, result + (size_t)b0 * N, nS, N, M, cnt, workspace,
                            st));
    }
    return DEFTET_OK;
}

// workspace == NULL: the scalar-stream brute force; otherwise the grid search (both exact).
extern "C" int deftet_nn_index_f32(const float *queries, const float *points, int32_t *result, int B, int N, int M,
                                   void *workspace, size_t wsb, void *stream_)
{
    return nn_index_impl(queries, points, result, B, N, M, nullptr, workspace, wsb, stream_);
}

extern "C" int deftet_nn_index_ragged_f32(const float *queries, const float *points, int32_t *result, int B, int N_max, int M,
                                          const int *n_query_host, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_CHECK_ARG(n_query_host || B == 0, "null n_query_host");
    return nn_index_impl(queries, points, result, B, N_max, M, n_query_host, workspace, wsb, stream_);
}
