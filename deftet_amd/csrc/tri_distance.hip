// tri_distance.hip — the point-to-triangle distance layers.DefTet.forward calls per shape for
// CDNA4 / gfx950; what it shares with the other surface operators is in surface_batch.hpp.
//   A9  deftet_tri_dist_fwd/bwd   layers/DefTet/tet_analytic_distance_batch/tet_analytic_distance_for.cu:15-334
//                                  layers/DefTet/tet_analytic_distance_batch/tet_analytic_distance_back.cu:15-715
#pragma clang fp contract(off)
#include "common.hpp"
#include "grid_setup.hpp"
#include "prims.hpp"
#include "surface_batch.hpp"
#include "wave.hpp"

namespace deftet {
namespace surf {

// ---------------------------------------------------------------------------- A9 point -> triangle distance
__device__ __forceinline__ float divide_non_zero(float a)
{   // tet_analytic_distance_for.cu:40-52: `eps` is a double literal, the sum is formed in double
    if (a == 0) return (float)1e-10;
    if (a < 0) return (float)((double)a - 1e-10);
    if (a > 0) return (float)((double)a + 1e-10);
    return (float)1e-10;
}
__device__ __forceinline__ float abs_ref(float a) { return a > 0.0f ? a : -a; }                 // :20-28
__device__ __forceinline__ float min3(float a, float b, float c) { float m = a; if (b < m) m = b; if (c < m) m = c; return m; }
__device__ __forceinline__ float min3_idx(float a, float b, float c)
{   // tet_analytic_distance_back.cu:139-152
    float m = a, i = 0.f;
    if (b < m) { m = b; i = 1.f; }
    if (c < m) { m = c; i = 2.f; }
    return i;
}
__device__ __forceinline__ float dist_point_sq(const float *a, const float *b)
{   // :139-146
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}
__device__ __forceinline__ float distance_line_square(const float *A, const float *B, const float *P)
{   // :148-170
    float PA[3], BA[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { PA[k] = P[k] - A[k]; BA[k] = B[k] - A[k]; }
    const float t = dot3(PA, BA) / divide_non_zero(dot3(BA, BA));
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float tmp = BA[k] * t; d[k] = PA[k] - tmp; }
    const float distance = dot3(d, d);
    if (t >= 0 && t <= 1) return distance;
    return -distance;
}

template <bool WANT_IDX>
__device__ __forceinline__ void line_distance(const float *a, const float *b, const float *c, const float *p, float *ret,
                                              float max_dis)
{   // cuda_line_distance, for.cu:172-220 / back.cu:348-403
    const float k1 = (b[1] - c[1]) * (p[0] - c[0]) + (c[0] - b[0]) * (p[1] - c[1]);
    const float k2 = (a[0] - c[0]) * (p[1] - c[1]) + (c[1] - a[1]) * (p[0] - c[0]);
    const float k3 = (b[1] - c[1]) * (a[0] - c[0]) + (c[0] - b[0]) * (a[1] - c[1]);
    if (k3 == 0) { ret[0] = -1; return; }
    const float l1 = k1 / k3, l2 = k2 / k3, l3 = 1 - l1 - l2;
    float dis12 = distance_line_square(a, b, p);
    float dis23 = distance_line_square(b, c, p);
    float dis13 = distance_line_square(a, c, p);
    if (l1 >= 0 && l2 >= 0 && l3 >= 0) {
        ret[0] = 0;
        ret[1] = min3(abs_ref(dis12), abs_ref(dis23), abs_ref(dis13));
        if (WANT_IDX) ret[2] = min3_idx(abs_ref(dis12), abs_ref(dis23), abs_ref(dis13));
        return;
    }
    if (dis12 <= 0) dis12 = max_dis;
    if (dis23 <= 0) dis23 = max_dis;
    if (dis13 <= 0) dis13 = max_dis;
    const float min_line = min3(dis12, dis23, dis13);
    const float d1 = dist_point_sq(a, p), d2 = dist_point_sq(b, p), d3 = dist_point_sq(c, p);
    const float min_pt = min3(d1, d2, d3);
    if (min_line < min_pt) {
        ret[0] = 1; ret[1] = min_line;
        if (WANT_IDX) ret[2] = min3_idx(dis12, dis23, dis13);
    } else {
        ret[0] = 2; ret[1] = min_pt;
        if (WANT_IDX) ret[2] = min3_idx(d1, d2, d3);
    }
}

__device__ __forceinline__ void plane_project(const float *a, const float *b, const float *c, const float *p, float *ip,
                                              float &t_out)
{   // for.cu:227-238 / back.cu:411-421
    float r1[3], r2[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { r1[k] = b[k] - a[k]; r2[k] = c[k] - a[k]; }
    n[0] = r1[1] * r2[2] - r1[2] * r2[1];
    n[1] = r1[2] * r2[0] - r1[0] * r2[2];
    n[2] = r1[0] * r2[1] - r1[1] * r2[0];
    float length = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);   // cuda_normalize, :128-137
    length = divide_non_zero(length);
    n[0] = n[0] / length; n[1] = n[1] / length; n[2] = n[2] / length;
    const float t = dot3(n, a) - dot3(n, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float m = n[k] * t; ip[k] = p[k] + m; }
    t_out = t;
}

template <bool WANT_IDX>
__device__ __forceinline__ float min_triangle_distance(const float *a, const float *b, const float *c, const float *p,
                                                       float *ret, float *ip, float max_dis)
{   // for.cu:222-254 (MAX_DIS 10000) / back.cu:406-436 (MAX_DIS 9999999)
    float t;
    plane_project(a, b, c, p, ip, t);
    const float distance_1 = t * t;
    line_distance<WANT_IDX>(a, b, c, ip, ret, max_dis);
    if (ret[0] == 0) return distance_1;
    if (ret[0] < 0) return max_dis;
    return distance_1 + ret[1];
}

// The same evaluation with a wave-level early out between its two halves.  Whatever the inside test decides, the value is
// t^2, t^2 + (a non-negative term) or max_dis >= every best-so-far, i.e. never below the fp32 square of the plane offset t
// computed first; so when t^2 > best holds for every voting lane the face can neither lower nor tie any of them and the
// expensive half (three point-line distances, ~350 of ~400 instructions) is skipped.  Bit-identical results.
// Returns false when skipped.
__device__ __forceinline__ bool min_triangle_distance_voted(const float *a, const float *b, const float *c, const float *p,
                                                            float best, bool voter, float &dis)
{
    float t, ip[3], ret[3] = {0.f, 0.f, 0.f};
    plane_project(a, b, c, p, ip, t);
    const float distance_1 = t * t;
    if (!__any(voter && distance_1 <= best)) return false;
    line_distance<false>(a, b, c, ip, ret, 10000.0f);
    dis = ret[0] == 0 ? distance_1 : (ret[0] < 0 ? 10000.0f : distance_1 + ret[1]);
    return true;
}

__global__ __launch_bounds__(256) void k_tri_dist_fwd(const float *__restrict__ pts, const float *__restrict__ face,
                                                      const float *__restrict__ n_face_b, float *closest_d,
                                                      float *closest_f, int P, int Fmax)
{
    const int b = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = q < P;
    const float *pp = pts + ((size_t)b * P + (live ? q : 0)) * 3;
    const float p[3] = {pp[0], pp[1], pp[2]};
    const int nf = (int)n_face_b[b];                                // for.cu:285
    const float *__restrict__ fb = face + (size_t)b * Fmax * 9;     // wave-uniform stream
    float min_d = 10000.0f;                                         // :277
    int min_idx = -1;
    for (int f = 0; f < nf; ++f) {
        float fc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) fc[i] = fb[(size_t)f * 9 + i];
        float ret[3] = {0.f, 0.f, 0.f}, ip[3];
        const float dis = min_triangle_distance<false>(fc, fc + 3, fc + 6, p, ret, ip, 10000.0f);
        if (min_d > dis) { min_d = dis; min_idx = f; }              // :300-303
    }
    if (live) {
        closest_d[(size_t)b * P + q] = min_d;
        closest_f[(size_t)b * P + q] = (float)min_idx;              // __int2float_rz, :306
    }
}

// --- A9 forward, grid-accelerated (exact) -------------------------------------------------------------
// Faces are binned by bounding box into a uniform grid whose cells are about one mean face extent
// wide; a point evaluates the reference formula only on the faces listed in the 3x3x3 (then 5x5x5)
// cells around it, plus a "wide" list of faces that every point must see, and stops once the best
// value is below a certified lower bound for every face it has not seen.  Faces on the wide list:
// non-finite, spanning > 64 cells, |n| < 1e-5 (the reference's normalisation adds 1e-10 to |n|),
// or nearly vertical (|k3| < |n|/64): for those the reference's xy-only inside test can misfire
// and report a plane distance for a far-away point, so their value is not bounded below by the
// true distance.  For every other face the reference value is the true squared distance up to
// rounding, which is what the pruning bound needs.  Points that are not settled
// within two shells go to the streaming scan (k_tri_far).  Results are combined lexicographically
// (value, face index) == "first strict minimum of the ascending scan" (for.cu:300-303).
constexpr int kTGMax = 64;             // cells per axis (upper bound)
constexpr int kTMaxCells = 64;         // faces overlapping more cells go to the wide list
constexpr int kTParts = 64;

constexpr float kTCellScale = 1.0f;    // cell width in mean face extents

struct TGrid { float o[3], inv[3], cs[3], slack[3]; int g[3]; float abs_slack; };

__device__ __forceinline__ bool face_regular(const float *fc, float &lox, float &loy, float &loz, float &hix, float &hiy, float &hiz)
{
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite = finite && (fabsf(fc[k]) <= 1048576.0f);
    lox = fminf(fc[0], fminf(fc[3], fc[6])); hix = fmaxf(fc[0], fmaxf(fc[3], fc[6]));
    loy = fminf(fc[1], fminf(fc[4], fc[7])); hiy = fmaxf(fc[1], fmaxf(fc[4], fc[7]));
    loz = fminf(fc[2], fminf(fc[5], fc[8])); hiz = fmaxf(fc[2], fmaxf(fc[5], fc[8]));
    const float r1[3] = {fc[3] - fc[0], fc[4] - fc[1], fc[5] - fc[2]}, r2[3] = {fc[6] - fc[0], fc[7] - fc[1], fc[8] - fc[2]};
    const float nx = r1[1] * r2[2] - r1[2] * r2[1], ny = r1[2] * r2[0] - r1[0] * r2[2], nz = r1[0] * r2[1] - r1[1] * r2[0];
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    const float k3 = (fc[4] - fc[7]) * (fc[0] - fc[6]) + (fc[6] - fc[3]) * (fc[1] - fc[7]);    // as cuda_line_distance computes it
    return finite && len >= 1e-5f && fabsf(k3) * 64.0f >= len && fabsf(nz) * 64.0f >= len;
}

// (the same launch clears what the later kernels accumulate into: cell counters, fill cursors, the counters block and the
// coarse-cell representatives)
__global__ __launch_bounds__(256) void k_tri_face_stats(const float *__restrict__ face, const float *__restrict__ nfb, float *part,
                                                        size_t slice, int Fmax, int *cnt0, int *fill0, int *counters, int *rep, int nc,
                                                        int nRepCells, int *pcnt0)
{
    __shared__ float sh[4][8];
    const int sb = blockIdx.y;
    face += (size_t)sb * Fmax * 9; nfb += sb;
    SHAPE(part); SHAPE(cnt0); SHAPE(fill0); SHAPE(counters); SHAPE(rep); SHAPE(pcnt0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc; i += gridDim.x * blockDim.x) { cnt0[i] = 0; fill0[i] = 0; pcnt0[i] = 0; }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nRepCells; i += gridDim.x * blockDim.x) rep[i] = -1;
    if (blockIdx.x == 0 && threadIdx.x < 8) counters[threadIdx.x] = 0;
    const int nf = (int)nfb[0];
    BoxStats<3, 2> bs;                                              // sums: largest box extent of the regular faces, their number
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) {
        float fc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) fc[k] = face[(size_t)f * 9 + k];
        float l[3], h[3];
        if (face_regular(fc, l[0], l[1], l[2], h[0], h[1], h[2])) {
            bs.add_box(l, h);
            bs.add_sum(0, fmaxf(fmaxf(h[0] - l[0], h[1] - l[1]), h[2] - l[2]));
            bs.add_sum(1, 1.f);
        }
    }
    bs.block_store(sh, part + blockIdx.x * 8);
}

__global__ __launch_bounds__(64) void k_tri_grid(const float *__restrict__ part, TGrid *gp, size_t slice)
{
    const int sb = blockIdx.x;
    SHAPE(part); SHAPE(gp);
    const int lane = threadIdx.x;
    BoxStats<3, 2> bs;
    bs.load(part + lane * 8);
    bs.wave_reduce();
    if (lane == 0) {
        TGrid r;
        const float sw = bs.sum[0], cnt = bs.sum[1];
        const float meanw = cnt > 0.f ? sw / cnt : 0.f;
        float diag2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool ok = bs.hi[k] >= bs.lo[k];
            const float l = ok ? bs.lo[k] : 0.f, h = ok ? bs.hi[k] : 0.f, ext = h - l;
            float n = (meanw > 0.f && ext > 0.f) ? ceilf(ext / (meanw * kTCellScale)) : 1.f;
            n = fminf(fmaxf(n, 1.f), (float)kTGMax);
            r.g[k] = (int)n;
            r.o[k] = l;
            r.inv[k] = ext > 1e-30f ? n / ext : 0.f;
            r.cs[k] = ext > 1e-30f ? ext / n : INFINITY;
            r.slack[k] = 8e-6f * (fabsf(l) + fabsf(h)) + 1e-30f;
            diag2 += (fabsf(l) + fabsf(h)) * (fabsf(l) + fabsf(h));
        }
        r.abs_slack = 1e-8f * diag2;                               // see the bound in k_tri_query_coop
        *gp = r;
    }
}

// mode 0: count cells / append to the wide list; mode 1: fill the cell lists
constexpr int kTCoarse = 4;            // coarse cells (4x4x4 cells) keep one representative face each for the far path
constexpr int kTGc = kTGMax / kTCoarse;

__global__ __launch_bounds__(256) void k_tri_face_bin(const float *__restrict__ face, const float *__restrict__ nfb,
                                                      const TGrid *__restrict__ gp, int mode, int *cellCount,
                                                      const int *__restrict__ cellStart, int *cellFill, int *list, int *wide,
                                                      int *nWide, int *rep, size_t slice, int Fmax, float4 *sph, uint2 *frange)
{
    const int sb = blockIdx.y;
    face += (size_t)sb * Fmax * 9; nfb += sb;
    SHAPE(gp); SHAPE(cellCount); SHAPE(cellStart); SHAPE(cellFill); SHAPE(list); SHAPE(wide); SHAPE(nWide); SHAPE(rep); SHAPE(sph); SHAPE(frange);
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= (int)nfb[0]) return;
    const TGrid g = *gp;
    float fc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fc[k] = face[(size_t)f * 9 + k];
    float lox, loy, loz, hix, hiy, hiz;
    bool tiles = face_regular(fc, lox, loy, loz, hix, hiy, hiz);
    int x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
    if (tiles) {
        x0 = grid_cell(lox - g.slack[0], g.o[0], g.inv[0], g.g[0]); x1 = grid_cell(hix + g.slack[0], g.o[0], g.inv[0], g.g[0]);
        y0 = grid_cell(loy - g.slack[1], g.o[1], g.inv[1], g.g[1]); y1 = grid_cell(hiy + g.slack[1], g.o[1], g.inv[1], g.g[1]);
        z0 = grid_cell(loz - g.slack[2], g.o[2], g.inv[2], g.g[2]); z1 = grid_cell(hiz + g.slack[2], g.o[2], g.inv[2], g.g[2]);
        tiles = (x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1) <= kTMaxCells;
    }
    if (!tiles) {
        if (mode == 0) {
            wide[atomicAdd(nWide, 1)] = f;
            // the face's plane exactly as plane_project forms it (-ffp-contract=off: the same fp32 operations give the same
            // bits here and there): k_tri_query_coop gets the plane offset t of a point, which bounds the reference value
            // from below, from five operations instead of the whole projection
            float r1[3], r2[3], n[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { r1[k] = fc[3 + k] - fc[k]; r2[k] = fc[6 + k] - fc[k]; }
            n[0] = r1[1] * r2[2] - r1[2] * r2[1];
            n[1] = r1[2] * r2[0] - r1[0] * r2[2];
            n[2] = r1[0] * r2[1] - r1[1] * r2[0];
            float length = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            length = divide_non_zero(length);
            n[0] = n[0] / length; n[1] = n[1] / length; n[2] = n[2] / length;
            sph[f] = make_float4(n[0], n[1], n[2], dot3(n, fc));      // t(p) = w - dot3(n, p), as plane_project forms it
        }
        return;
    }
    if (mode == 0) {
        // bounding sphere about the centroid (a point OF the triangle): |p - c| - R <= distance(p, triangle) <= |p - c|.
        // k_tri_query_coop prunes with the lower bound; rounding of c and R is covered by the grid's per-axis slack there.
        float c[3], r2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (fc[k] + fc[3 + k] + fc[6 + k]) * (1.0f / 3.0f);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const float dx = fc[v * 3] - c[0], dy = fc[v * 3 + 1] - c[1], dz = fc[v * 3 + 2] - c[2];
            r2 = fmaxf(r2, dx * dx + dy * dy + dz * dz);
        }
        sph[f] = make_float4(c[0], c[1], c[2], sqrtf(r2) * 1.00001f);
        // its cell range, six bits per bound: what k_tri_query_coop's canonical-cell rule needs of the face
        frange[f] = make_uint2((unsigned)x0 | (unsigned)x1 << 6 | (unsigned)y0 << 12 | (unsigned)y1 << 18 | (unsigned)z0 << 24, (unsigned)z1);
    }
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const int c = (z * g.g[1] + y) * g.g[0] + x;
                if (mode == 0) atomicAdd(&cellCount[c], 1);
                else list[cellStart[c] + atomicAdd(&cellFill[c], 1)] = f | (x << 24);   // face | x cell (kTFaceBits)
            }
    if (mode == 0)                                                   // any face overlapping the coarse cell will do
        for (int z = z0 / kTCoarse; z <= z1 / kTCoarse; ++z)
            for (int y = y0 / kTCoarse; y <= y1 / kTCoarse; ++y)
                for (int x = x0 / kTCoarse; x <= x1 / kTCoarse; ++x) atomicMax(&rep[(z * kTGc + y) * kTGc + x], f);
}

// Points are sorted by their (clamped) grid cell — a counting sort: count + rank (one returning atomic per point), scan,
// scatter — so that the 64 lanes of a wave are neighbours in space, walk the same cells and fetch the same face records;
// the GT point cloud itself comes in arbitrary order.  (Round 2 used a library radix sort: ~20 launches per call.)  The
// order of the points inside a cell is whatever the atomics gave; no result depends on it.
__global__ __launch_bounds__(256) void k_tri_point_keys(const float *__restrict__ pts, int P, const TGrid *__restrict__ gp, int *pcount,
                                                        int2 *prank, size_t slice)
{
    const int sb = blockIdx.y;
    pts += (size_t)sb * P * 3;
    SHAPE(gp); SHAPE(pcount); SHAPE(prank);
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = q < P;                                         // (no early return: run_atomic_rank is a wave operation)
    const TGrid g = *gp;
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = grid_cell(pts[(live ? q : 0) * 3 + k], g.o[k], g.inv[k], g.g[k]);
    const int cell = live ? (c[2] * kTGMax + c[1]) * kTGMax + c[0] : -1;   // 18 bits: z, y, x
    const int rank = run_atomic_rank(pcount, cell);                    // one atomic per run of lanes in the same cell
    if (live) prank[q] = make_int2(cell, rank);
}

__global__ __launch_bounds__(256) void k_tri_point_scatter(int P, const int2 *__restrict__ prank, const int *__restrict__ pstart,
                                                           unsigned *order, unsigned *skey, size_t slice)
{
    // order / skey: ONE array of P entries per shape (outside the slices)
    const int sb = blockIdx.y;
    order += (size_t)sb * P; skey += (size_t)sb * P;
    SHAPE(prank); SHAPE(pstart);
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const int2 r = prank[q];
    const int slot = pstart[r.x] + r.y;
    order[slot] = (unsigned)q;
    skey[slot] = (unsigned)r.x;
}

// ---- the grid query, wave-cooperative ------------------------------------------------------------
// Points arrive sorted by grid cell (z, y, x with x fastest); a CHUNK is up to 64 consecutive points of one (y, z) ROW of
// cells, i.e. of the x-adjacent cells [xa, xb].  The search box of shell r is [xa-r, xb+r] x [y-r, y+r] x [z-r, z+r]; per
// (y', z') row of the box the face-list entries of its cells are ONE contiguous range of `list` (cells are stored x
// fastest), which the wave walks 64 entries at a time: lane k loads entry k, the entries that survive the filters are
// broadcast one by one (v_readlane) and every lane tests its own point against the broadcast bounding sphere.
// (Round 2 gave a wave the points of ONE cell — ~10 of 64 lanes at the training-time density — and walked the box cell
// by cell, 27 or 125 short lists per chunk: the per-list overhead was what the kernel spent its time on, 2.2 ms per 8
// shapes; see profiles/r03_pmc_tri_query.json.)  The boxes are taken around the CHUNK's cells; a lane's termination test
// uses its own distance to that box, so the bound holds unchanged.  Extra evaluations cannot change the lexicographic
// (distance, index) minimum.
constexpr int kTRows = kTGMax * kTGMax;     // (y, z) rows of the grid
constexpr int kTFaceBits = 24;              // list entries: face index | x cell << 24 (faces < 2^24 is checked at the boundary)
constexpr int kTFaceMask = (1 << kTFaceBits) - 1;

__global__ __launch_bounds__(256) void k_tri_chunks(const int *__restrict__ pstart, int *ptStart, int *chunkCount, size_t slice)
{
    const int sb = blockIdx.y;
    SHAPE(pstart); SHAPE(ptStart); SHAPE(chunkCount);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;               // row = cell >> 6
    if (r > kTRows) return;
    const int s0 = pstart[r << 6];                                     // pstart has 64^3 + 1 entries, the last = P
    ptStart[r] = s0;
    chunkCount[r] = r < kTRows ? (pstart[(r + 1) << 6] - s0 + 63) >> 6 : 0;
}

#ifdef TRI_STATS          // probe builds only (tools/probes/tri_stats_probe.py): where k_tri_query_coop spends its instructions
__device__ unsigned long long g_tri_stats[16];
#define TRI_STAT(i, v) do { if (lane == 0) atomicAdd(&g_tri_stats[i], (unsigned long long)(v)); } while (0)
#else
#define TRI_STAT(i, v)
#endif
constexpr int kTriChunkWaves = 4;      // waves per chunk of 64 points in k_tri_query_coop: they split the rows of the search box
constexpr int kTriCand = 8;            // per-lane candidate slots (LDS) between two drains in k_tri_query_coop

__device__ __forceinline__ void tri_query_chunk(int W, int part, float (*s_lb)[64], int (*s_cf)[64], int *s_q, unsigned long long *s_best,
                                                const uint2 *__restrict__ frange, const float4 *__restrict__ sph, const unsigned *__restrict__ skey,
                                                const float *__restrict__ pts, const float *__restrict__ face,
                                                const float *__restrict__ nfb, int P, const TGrid *__restrict__ gp,
                                                const int *__restrict__ cellStart, const int *__restrict__ list,
                                                const int *__restrict__ wide, const int *__restrict__ nWide, float *closest_d,
                                                float *closest_f, int *farFlag, const unsigned *__restrict__ order,
                                                const int *__restrict__ ptStart, const int *__restrict__ chunkStart,
                                                const int *__restrict__ rep)
{
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = kTRows;                                         // largest row with chunkStart[row] <= W
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunkStart[mid] <= W) lo = mid; else hi = mid;
    }
    const int row = lo;
    const int slot = ptStart[row] + (W - chunkStart[row]) * 64 + lane;
    const bool live = slot < ptStart[row + 1];
    const int q = live ? (int)order[slot] : 0;
    int xa = live ? (int)(skey[slot] & 63u) : 63, xb = live ? (int)(skey[slot] & 63u) : 0;   // the chunk's cells on x
#pragma unroll  // wave_min's and wave_max's order (wave.hpp); written out, a call changes this kernel's instruction stream
    for (int off = 32; off > 0; off >>= 1) {
        xa = min(xa, __shfl_xor(xa, off));
        xb = max(xb, __shfl_xor(xb, off));
    }
    xa = __builtin_amdgcn_readfirstlane(xa);
    xb = __builtin_amdgcn_readfirstlane(xb);
    const TGrid g = *gp;
    const float p[3] = {pts[q * 3], pts[q * 3 + 1], pts[q * 3 + 2]};
    const int nf = (int)nfb[0];
    if (live && part == 0) farFlag[slot] = 0;                      // every sorted slot belongs to exactly one live lane
    if (nf <= 0) {
        if (live && part == 0) { closest_d[q] = 10000.0f; closest_f[q] = -1.0f; }
        return;
    }
    const bool tame = fabsf(p[0]) <= 1048576.0f && fabsf(p[1]) <= 1048576.0f && fabsf(p[2]) <= 1048576.0f;
    float min_d = 10000.0f;                                         // for.cu:277
    int min_idx = -1;
    auto take = [&](int f, float dis) {
        if (min_d > dis || (min_d == dis && f < min_idx)) { min_d = dis; min_idx = f; }   // lexicographic (value, index)
    };
    // The four waves of the block work on the same 64 points (different rows of the box) and keep ONE best per point in
    // LDS, as a packed (value, index) word under atomicMin: a wave that only sees far rows prunes with what the wave on the
    // near rows has found.  Any published word is the value of an evaluated face, so pruning against it is as valid as
    // against the wave's own best, whenever it arrives; the final minimum does not depend on the timing.
    auto publish = [&]() { atomicMin(&s_best[lane], pack_best(min_d, min_idx)); };
    auto refresh = [&]() { unpack_best(s_best[lane], min_d, min_idx); };
    // wave-uniform evaluation (the wide list): every lane evaluates the broadcast face, with the plane-offset vote
    auto eval = [&](int f, const float *fc) {
        float dis;
        if (min_triangle_distance_voted(fc, fc + 3, fc + 6, p, min_d, live, dis)) take(f, dis);
    };
    // Regular faces are pruned per LANE with their bounding sphere: the reference value of a regular face is its true
    // squared distance up to rounding (the certificate the shell test below already relies on: value >= 0.9998 d^2 -
    // abs_slack), and d >= |p - c| - R.  A lane keeps the faces it cannot rule out in kTriCand LDS slots and evaluates
    // them itself (its own gather of the 36-byte record), nearest sphere first, re-testing each against the best so far:
    // a handful of evaluations per point instead of one per face of the neighbourhood and wave.  A face ruled out has a
    // value strictly above the lane's best, so it can neither lower nor tie it: same lexicographic minimum.
    const float sph_slack = g.slack[0] + g.slack[1] + g.slack[2];
    int ncand = 0;
    auto ruled_out = [&](float lb2) { return 0.9998f * lb2 - g.abs_slack > min_d; };
    auto eval_own = [&](int f) {
        const float *src = face + (size_t)f * 9;
        float fc[9], ret[3] = {0.f, 0.f, 0.f}, ip[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) fc[j] = src[j];
        take(f, min_triangle_distance<false>(fc, fc + 3, fc + 6, p, ret, ip, 10000.0f));
    };
    auto drain = [&]() {
        publish();
        refresh();
        // round 1: every lane evaluates its nearest candidate — after it the bests are tight
        int first = 0;
        float lbmin = INFINITY;
        for (int j = 0; j < kTriCand; ++j) {
            const float v = j < ncand ? s_lb[j][lane] : INFINITY;
            if (v < lbmin) { lbmin = v; first = j; }
        }
        if (ncand > 0 && !ruled_out(lbmin)) {
            eval_own(s_cf[first][lane]);
            publish();
        }
        // the candidates that survive the re-test go to a wave-wide queue of (lane, face) pairs and are evaluated 64 per
        // round whoever owns them: rounds = ceil(survivors / 64) instead of the largest per-lane count
        unsigned surv = 0u;
        for (int j = 0; j < kTriCand; ++j)
            if (j < ncand && j != first && !ruled_out(s_lb[j][lane])) surv |= 1u << j;
        const int mine = __popc(surv);
        const int incl = wave_incl_sum(mine, lane);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        TRI_STAT(4, 1);                                             // [4] drains
        TRI_STAT(6, (total + 63) >> 6);                             // [6] queue rounds
        TRI_STAT(7, total);                                         // [7] queued pair evaluations
        if (total > 0) {
            int pos = incl - mine;
            for (int j = 0; j < kTriCand; ++j)
                if (surv >> j & 1u) s_q[pos++] = (lane << kTFaceBits) | s_cf[j][lane];
            __builtin_amdgcn_wave_barrier();
            for (int base = 0; base < total; base += 64) {
                const int e = base + lane < total ? s_q[base + lane] : -1;
                const int pl = e >= 0 ? e >> kTFaceBits : lane;
                const float pp[3] = {__shfl(p[0], pl), __shfl(p[1], pl), __shfl(p[2], pl)};
                if (e >= 0) {
                    const int f = e & kTFaceMask;
                    const float *src = face + (size_t)f * 9;
                    float fc[9], ret[3] = {0.f, 0.f, 0.f}, ip[3];
#pragma unroll
                    for (int j = 0; j < 9; ++j) fc[j] = src[j];
                    const float dis = min_triangle_distance<false>(fc, fc + 3, fc + 6, pp, ret, ip, 10000.0f);
                    atomicMin(&s_best[pl], pack_best(dis, f));           // lexicographic (value, index): values are >= +0, NaN packs above all
                }
            }
            __builtin_amdgcn_wave_barrier();
            refresh();
        }
        ncand = 0;
    };
    // A face overlapping several cells is listed in each of them: inside a search box it is taken only from its CANONICAL
    // cell — of its cells inside the box, the one nearest to the chunk's cells on every axis — once per distinct face.
    // reach2 / plo / phi (set per shell below): a regular face whose box is farther than sqrt(reach2) from the box of the
    // wave's unsettled points cannot bring any of them under its certification threshold, so it is not looked at here —
    // either the lane is settled by a nearer face or it goes to the far path, which is exact.
    float reach2 = INFINITY, plo[3] = {0.f, 0.f, 0.f}, phi[3] = {0.f, 0.f, 0.f};
    float bestmax = INFINITY;                                       // largest best among the wave's live points (wide list only)
    int boxn[3] = {1, 1, 1};                                        // cells per axis of the current search box
    const int Clo[3] = {xa, row & (kTGMax - 1), row >> 6}, Chi[3] = {xb, row & (kTGMax - 1), row >> 6};   // the chunk's (clamped) cells
    // entries [s, e): the lists of the cells [bx0, bx1] of row (cy, cz) when filter, else a stretch of the wide list
    // (rmod, rsel): of the 64-entry rounds of the range, this wave takes those with index % rmod == rsel
    auto list_run = [&](const int *__restrict__ lst, int s, int e, bool filter, int cy, int cz, int bx0, int by0, int bz0, int rmod, int rsel) {
        for (int base = s + rsel * 64; base < e; base += 64 * rmod) {
            TRI_STAT(1, 1);                                         // [1] 64-entry rounds
            TRI_STAT(2, min(64, e - base));                         // [2] list entries loaded
            const int idx = base + lane;
            const bool have = idx < e;
            const int ent = have ? lst[idx] : 0;
            const int fm = ent & kTFaceMask;
            float fv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            bool use = have;
            float4 sp = make_float4(0.f, 0.f, 0.f, 0.f);             // regular faces: sphere; wide faces: plane
            float blo[3] = {0.f, 0.f, 0.f}, bhi[3] = {0.f, 0.f, 0.f}; // the face's bounding box
            if (have && filter) {
                // canonical cell: of the face's cells (as k_tri_face_bin listed them) inside the box, the one NEAREST to the
                // chunk's cells on every axis (so that a skipped row implies that all the face's cells are out of reach)
                const uint2 rg = frange[fm];
                const int f0[3] = {(int)(rg.x & 63u), (int)(rg.x >> 12 & 63u), (int)(rg.x >> 24 & 63u)};
                const int f1[3] = {(int)(rg.x >> 6 & 63u), (int)(rg.x >> 18 & 63u), (int)(rg.y & 63u)};
                const int cc[3] = {(int)((unsigned)ent >> kTFaceBits), cy, cz}, bb0[3] = {bx0, by0, bz0};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int lo_k = max(f0[k], bb0[k]), hi_k = min(f1[k], bb0[k] + boxn[k] - 1);
                    const int canon = lo_k > Chi[k] ? lo_k : (hi_k < Clo[k] ? hi_k : max(lo_k, Clo[k]));
                    use = use && cc[k] == canon;
                }
                if (use) {                                            // one listing in ~8 survives: only those fetch the record
#pragma unroll
                    for (int k = 0; k < 9; ++k) fv[k] = face[(size_t)fm * 9 + k];
                    sp = sph[fm];
                    float d2 = 0.f;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        blo[k] = fminf(fv[k], fminf(fv[3 + k], fv[6 + k]));
                        bhi[k] = fmaxf(fv[k], fmaxf(fv[3 + k], fv[6 + k]));
                        const float d = fmaxf(fmaxf(plo[k] - bhi[k], blo[k] - phi[k]), 0.f);
                        d2 += d * d;
                    }
                    use = !(d2 * 0.9999f > reach2);
                }
            }
            if (have && !filter) {
#pragma unroll
                for (int k = 0; k < 9; ++k) fv[k] = face[(size_t)fm * 9 + k];
                sp = sph[fm];
                // wide face: its plane offset t over the box of the wave's points lies in [tlo, thi] (up to rounding, mag
                // bounds the operands); when even the smallest |t| squared exceeds every lane's best, the vote below fails
                // for every lane — decided here for 64 faces at once instead of one broadcast each
                float smax = 0.f, smin = 0.f, mag = fabsf(sp.w);
                const float nn[3] = {sp.x, sp.y, sp.z};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float a = nn[k] * plo[k], b = nn[k] * phi[k];
                    smax += fmaxf(a, b); smin += fminf(a, b);
                    mag += fmaxf(fabsf(a), fabsf(b));
                }
                const float tlo = sp.w - smax, thi = sp.w - smin;
                const float tabs = fmaxf((tlo > 0.f ? tlo : (thi < 0.f ? -thi : 0.f)) - 1e-5f * mag, 0.f);
                use = !(tabs * tabs > bestmax);                           // NaN / Inf planes or boxes: looked at
            }
            unsigned long long todo = __ballot(use);
            TRI_STAT(filter ? 3 : 8, __popcll(todo));               // [3] faces broadcast (cell lists), [8] (wide list)
            while (todo) {
                const int k = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int f = __builtin_amdgcn_readlane(fm, k);
                if (filter) {
                    const float dx = p[0] - lane_bcast(sp.x, k), dy = p[1] - lane_bcast(sp.y, k), dz = p[2] - lane_bcast(sp.z, k);
                    const float lb = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz) - lane_bcast(sp.w, k) - sph_slack, 0.f);
                    float box2 = 0.f;                                  // ... and the point's distance to its bounding box
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float d = fmaxf(fmaxf(lane_bcast(blo[a], k) - p[a], p[a] - lane_bcast(bhi[a], k)), 0.f);
                        box2 += d * d;
                    }
                    const float lb2 = fmaxf(lb * lb, box2);
                    if (live && tame && !ruled_out(lb2)) {
                        s_lb[ncand][lane] = lb2;
                        s_cf[ncand][lane] = f;
                        ++ncand;
                    }
                    if (__any(ncand == kTriCand)) drain();
                } else {
                    // the vote of eval() from the precomputed plane (the same fp32 operations as plane_project: same t)
                    const float n[3] = {lane_bcast(sp.x, k), lane_bcast(sp.y, k), lane_bcast(sp.z, k)};
                    const float t = lane_bcast(sp.w, k) - dot3(n, p);
                    if (!__any(live && t * t <= min_d)) continue;
                    float fc[9];
#pragma unroll
                    for (int j = 0; j < 9; ++j) fc[j] = lane_bcast(fv[j], k);
                    eval(f, fc);
                }
            }
        }
    };
    {   // No face within the coarse cells (4x4x4 cells each) around the chunk's cells: the two shells below cannot
        // settle anything — the whole wave goes to the far path at once (the wide list is evaluated there as well).
        bool any_face = false;
        for (int z = max(Clo[2] / kTCoarse - 1, 0); z <= min(Clo[2] / kTCoarse + 1, kTGc - 1); ++z)
            for (int y = max(Clo[1] / kTCoarse - 1, 0); y <= min(Clo[1] / kTCoarse + 1, kTGc - 1); ++y)
                for (int x = max(xa / kTCoarse - 1, 0); x <= min(xb / kTCoarse + 1, kTGc - 1); ++x)
                    any_face = any_face || rep[(z * kTGc + y) * kTGc + x] >= 0;
        // Likewise when every point of the wave lies more than three cells outside the grid (the faces' bounding box, onto
        // whose boundary cells such points are clamped): the shells reach two cells.  Sending a point to the far path is
        // always exact, only the cost differs.
        float out2 = 0.f, csmax = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(g.cs[k] < INFINITY)) continue;
            const float d = fmaxf(fmaxf(g.o[k] - p[k], p[k] - (g.o[k] + (float)g.g[k] * g.cs[k])), 0.f);
            out2 += d * d;
            csmax = fmaxf(csmax, g.cs[k]);
        }
        const bool outside = out2 > 9.f * csmax * csmax;
        if (!any_face || __all(!live || outside)) {
            if (live && part == 0) farFlag[slot] = 1;
            return;
        }
    }
    if (part == 0) s_best[lane] = pack_best(10000.0f, -1);              // for.cu:277
    __syncthreads();
    bool done = false;
    TRI_STAT(0, 1);                                                 // [0] wave-chunks that search
    {
        const int nlive = __popcll(__ballot(live));
        TRI_STAT(10, nlive);                                        // [10] live lanes
        (void)nlive;
    }
    TRI_STAT(11, xb - xa + 1);                                      // [11] cells spanned on x
    for (int r = 1; r <= 2; ++r) {
        if (__all(done || !live || !tame)) break;
        TRI_STAT(11 + r, 1);                                        // [12] shells r = 1, [13] shells r = 2
        // the whole box [Clo-r, Chi+r] (clipped to the grid); r == 2 revisits the inner cells, which is cheap
        // with one look per distinct face and keeps the canonical rule simple
        const int b0[3] = {max(Clo[0] - r, 0), max(Clo[1] - r, 0), max(Clo[2] - r, 0)};
        const int b1[3] = {min(Chi[0] + r, g.g[0] - 1), min(Chi[1] + r, g.g[1] - 1), min(Chi[2] + r, g.g[2] - 1)};
        // every face not seen after this shell lies outside the box of cells [Clo-r, Chi+r]: distance >= m (per lane)
        float m = INFINITY;
        bool more = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(g.cs[k] < INFINITY)) continue;                     // flat axis: one slab
            if (Clo[k] - r > 0) {
                more = true;
                m = fminf(m, fmaxf(p[k] - (g.o[k] + (float)(Clo[k] - r) * g.cs[k]) - g.slack[k], 0.f));
            }
            if (Chi[k] + r < g.g[k] - 1) {
                more = true;
                m = fminf(m, fmaxf((g.o[k] + (float)(Chi[k] + r + 1) * g.cs[k]) - p[k] - g.slack[k], 0.f));
            }
        }
        {   // what the unsettled lanes of this wave can still use: the largest threshold radius and the box of their points
            const bool act = live && tame && !done;
            float r2 = act ? (more ? m * m : INFINITY) : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { plo[k] = act ? p[k] : INFINITY; phi[k] = act ? p[k] : -INFINITY; }
#pragma unroll  // wave_min's and wave_max's order (wave.hpp); written out, a call changes this kernel's instruction stream
            for (int off = 32; off > 0; off >>= 1) {
                r2 = fmaxf(r2, __shfl_xor(r2, off));
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    plo[k] = fminf(plo[k], __shfl_xor(plo[k], off));
                    phi[k] = fmaxf(phi[k], __shfl_xor(phi[k], off));
                }
            }
            reach2 = r2;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) boxn[k] = b1[k] - b0[k] + 1;
        // distance^2 from the box of the unsettled points to cell layer c on axis k (wave-uniform values)
        auto gap2 = [&](int k, int c) -> float {
            if (!(g.cs[k] < INFINITY)) return 0.f;
            const float l = g.o[k] + (float)c * g.cs[k] - g.slack[k], h = g.o[k] + (float)(c + 1) * g.cs[k] + g.slack[k];
            const float d = fmaxf(fmaxf(l - phi[k], plo[k] - h), 0.f);
            return d * d;
        };
        {   // the chunk's own row first, its rounds dealt to the four waves: it holds the nearest faces of most points, and
            // what they give is in the shared bests before the other rows are pruned against them
            const int rowc = (Clo[2] * g.g[1] + Clo[1]) * g.g[0];
            const int s0 = cellStart[rowc + b0[0]], e0 = cellStart[rowc + b1[0] + 1];
            if (s0 < e0) list_run(list, s0, e0, true, Clo[1], Clo[2], b0[0], b0[1], b0[2], kTriChunkWaves, part);
            drain();
            __syncthreads();
            refresh();
        }
        int nth = 0;
        for (int z = b0[2]; z <= b1[2]; ++z)
            for (int y = b0[1]; y <= b1[1]; ++y) {
                if (y == Clo[1] && z == Clo[2]) continue;
                if ((nth++ % kTriChunkWaves) != part) continue;                               // this wave's rows of the box
                if (__all((gap2(1, y) + gap2(2, z)) * 0.9999f > reach2)) continue;             // the whole row is out of reach
                const int rowc = (z * g.g[1] + y) * g.g[0];
                const int s0 = cellStart[rowc + b0[0]], e0 = cellStart[rowc + b1[0] + 1];       // the row's cells: one range
                if (s0 < e0) list_run(list, s0, e0, true, y, z, b0[0], b0[1], b0[2], 1, 0);
            }
        if (r == 1) {
            // the wide list, AFTER the first shell: the lanes' bests are then small and most wide faces (typically the nearly
            // vertical ones of a grid-like surface, hundreds of them) fail the plane-offset vote of eval() at once
            drain();
            bestmax = (live && tame) ? min_d : 0.f;
            bestmax = wave_max(bestmax);
            const int nw = *nWide;                                  // every wave of the block takes every kTriChunkWaves-th batch
            list_run(wide, 0, nw, false, 0, 0, 0, 0, 0, kTriChunkWaves, part);
        }
        drain();
        publish();
        __syncthreads();                                            // every wave's work of this shell is in the shared bests
        refresh();
        __syncthreads();
        if (!more) done = true;                                      // the box covers the grid: every listed face was seen
        else if (min_d < (m * m) * 0.9998f - g.abs_slack) done = true;
    }
    if (!live || part != 0) return;
    if (!tame || !done) { farFlag[slot] = 1; return; }              // NaN / Inf / huge points, unresolved ones: the far path
    closest_d[q] = min_d;
    closest_f[q] = (float)min_idx;
}

// The number of chunks is only known on the device and at most P/64 + (number of rows); a fixed grid strides over them.
constexpr int kTriQueryBlocks = 8192;

// (Register budget of FOUR waves per SIMD: the allocator takes 145 VGPRs = three waves when left alone; held to 128 it
// spills nine dwords and the kernel runs 0.76 -> 0.63 ms at 8 x 97 k points — five waves, 96 VGPRs with 176 bytes of
// scratch, and six are slower again: geometry step 2.80 / 2.68 / 2.85 / 3.24 ms for 3 / 4 / 5 / 6 waves.)
__attribute__((amdgpu_waves_per_eu(4, 8)))
__global__ __launch_bounds__(kTriChunkWaves * 64) void k_tri_query_coop(const float *__restrict__ pts, const float *__restrict__ face,
                                                                         const float *__restrict__ nfb, int P, const TGrid *__restrict__ gp,
                                                                         const int *__restrict__ cellStart, const int *__restrict__ list,
                                                                         const int *__restrict__ wide, const int *__restrict__ nWide,
                                                                         float *closest_d, float *closest_f, int *farFlag,
                                                                         const unsigned *__restrict__ order, const int *__restrict__ ptStart,
                                                                         const int *__restrict__ chunkStart, const int *__restrict__ rep,
                                                                         size_t slice, int Fmax, const float4 *__restrict__ sph,
                                                                         const unsigned *__restrict__ skey, const uint2 *__restrict__ frange)
{
    const int sb = blockIdx.y;
    pts += (size_t)sb * P * 3; face += (size_t)sb * Fmax * 9; nfb += sb; closest_d += (size_t)sb * P; closest_f += (size_t)sb * P;
    order += (size_t)sb * P; skey += (size_t)sb * P;
    SHAPE(gp); SHAPE(cellStart); SHAPE(list); SHAPE(wide); SHAPE(nWide); SHAPE(farFlag); SHAPE(ptStart); SHAPE(chunkStart); SHAPE(rep); SHAPE(sph); SHAPE(frange);
    // One block per chunk of 64 points, its waves splitting the rows of the search box: one wave per chunk ran its chain of
    // dependent loads (cell starts -> list entries -> vertices) unhidden.
    __shared__ float s_lb[kTriChunkWaves][kTriCand][64];
    __shared__ int s_cf[kTriChunkWaves][kTriCand][64];
    __shared__ int s_q[kTriChunkWaves][kTriCand * 64];
    __shared__ unsigned long long s_best[64];                         // one (value, index) word per point of the chunk, all waves
    const int total = chunkStart[kTRows];
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int W = blockIdx.x; W < total; W += gridDim.x)
        tri_query_chunk(W, part, s_lb[part], s_cf[part], s_q[part], s_best, frange, sph, skey, pts, face, nfb, P, gp, cellStart, list, wide, nWide, closest_d,
                        closest_f, farFlag, order, ptStart, chunkStart, rep);
}

// ---- A9 far path: points the two shells did not settle (a surface still far from the cloud, early in training) ------
// Same shape as the A10 far path.  The unsettled points stay in cell order (flags + exclusive scan), 64 neighbours per
// group.  k_tri_far_bound evaluates the wide list and one representative face per coarse cell: an upper bound for every
// lane.  k_tri_far_rows walks the cell rows (cz,cy): a cell is skipped when 0.9997 dist^2 - abs_slack exceeds the current
// best of EVERY lane (the certified bound of k_tri_query_coop: every face listed only in skipped cells is a regular face
// farther than that), otherwise the list slice of the x-range the lanes can still reach is loaded cooperatively (lane k
// holds face k) and broadcast.  A face listed in several visited cells is evaluated once per block (bitset in LDS).  The
// rows of a group are split over kTriSlices blocks x 4 waves; answers are combined as 64-bit words (value bits, index)
// under min — the values are non-negative, so that is the reference's "first strict minimum of an ascending scan".
// (Before: one same-address atomic per unsettled point and the streaming scan over ALL faces for each of them —
// 5.2-5.7 ms against 4.8 ms for the plain scan when the 100 k points sit 30 % off a 4,032-face surface.)
constexpr int kTriSlices = 8;
constexpr int kTriWaves = 4;
constexpr int kTriBitWords = 4096;      // LDS bitset (16 KB): 131,072 faces; beyond that duplicates are simply evaluated again
static_assert(kTriBitWords * 4 + kTriWaves * 64 * 8 <= 32 * 1024, "k_tri_far_rows: keep the static LDS of the far path small");

struct TriLane {
    float p[3], min_d;
    int min_idx;
    __device__ __forceinline__ void eval(int f, const float *fc)
    {
        float dis;
        if (!min_triangle_distance_voted(fc, fc + 3, fc + 6, p, min_d, true, dis)) return;
        if (min_d > dis || (min_d == dis && f < min_idx)) { min_d = dis; min_idx = f; }   // lexicographic (value, index)
    }
    // entries [s, e) of a face list: 64 per round trip, lane k loads face k, the wave evaluates them one by one
    template <bool DEDUPE>
    __device__ __forceinline__ void run(const float *__restrict__ face, const int *__restrict__ lst, int s, int e, unsigned *bits, int lane)
    {
        for (int base = s; base < e; base += 64) {
            const int idx = base + lane;
            const int fm = idx < e ? (lst[idx] & 0xFFFFFF) : -1;       // cell lists carry their x cell above bit 24
            bool use = fm >= 0;
            if (DEDUPE && use) {
                const unsigned bit = 1u << (fm & 31);
                use = (atomicOr(&bits[fm >> 5], bit) & bit) == 0u;
            }
            float fv[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) fv[k] = use ? face[(size_t)fm * 9 + k] : 0.f;
            unsigned long long todo = __ballot(use);
            while (todo) {
                const int k = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                float fc[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) fc[j] = lane_bcast(fv[j], k);
                eval(__builtin_amdgcn_readlane(fm, k), fc);
            }
        }
    }
};

// unsettled points, still in cell order (off = exclusive scan of the flags); the last slot publishes their number
__global__ __launch_bounds__(256) void k_tri_compact(const int *__restrict__ flag, const int *__restrict__ off, const unsigned *__restrict__ order,
                                                     int P, int *farList, int *nFar, size_t slice)
{
    const int sb = blockIdx.y;
    order += (size_t)sb * P;
    SHAPE(flag); SHAPE(off); SHAPE(farList); SHAPE(nFar);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    if (flag[i]) farList[off[i]] = (int)order[i];
    if (i == P - 1) *nFar = off[i] + flag[i];
}

__global__ __launch_bounds__(kTriWaves * 64) void k_tri_far_bound(const float *__restrict__ pts, const float *__restrict__ face,
                                                                  const TGrid *__restrict__ gp, const int *__restrict__ wide,
                                                                  const int *__restrict__ nWide, const int *__restrict__ rep,
                                                                  const int *__restrict__ farList, const int *__restrict__ nFar,
                                                                  unsigned long long *bound, size_t slice, int P, int Fmax)
{
    __shared__ unsigned long long s_pack[kTriWaves][64];
    const int sb = blockIdx.y;
    pts += (size_t)sb * P * 3; face += (size_t)sb * Fmax * 9;
    SHAPE(gp); SHAPE(wide); SHAPE(nWide); SHAPE(rep); SHAPE(farList); SHAPE(nFar); SHAPE(bound);
    const int n = *nFar;
    if ((int)blockIdx.x * 64 >= n) return;                          // whole block idle
    const int lane = threadIdx.x & 63;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 64 + lane;
    const int q = farList[i < n ? i : n - 1];                       // idle lanes shadow the last far point
    const TGrid g = *gp;
    TriLane L;
    L.p[0] = pts[q * 3]; L.p[1] = pts[q * 3 + 1]; L.p[2] = pts[q * 3 + 2];
    L.min_d = 10000.0f;                                             // for.cu:277
    L.min_idx = -1;
    const int nw = *nWide;
    for (int s = part * 64; s < nw; s += kTriWaves * 64) L.run<false>(face, wide, s, min(s + 64, nw), nullptr, lane);
    // One representative face per coarse cell (4x4x4 cells), in raster order, every fourth one per wave.  A representative
    // is evaluated only while its coarse cell is within reach of some lane's current best (same certified test as the rows
    // kernel; the face overlaps the cell, so it may also be closer: it is an upper bound either way), which leaves a few
    // dozen evaluations of the ~400-instruction distance formula instead of one per occupied coarse cell.
    const int gc[3] = {(g.g[0] + kTCoarse - 1) / kTCoarse, (g.g[1] + kTCoarse - 1) / kTCoarse, (g.g[2] + kTCoarse - 1) / kTCoarse};
    for (int cz = 0; cz < gc[2]; ++cz)
        for (int cy = 0; cy < gc[1]; ++cy)
            for (int cx0 = part * kNNBatch; cx0 < gc[0]; cx0 += kTriWaves * kNNBatch) {
                int r[kNNBatch];
#pragma unroll
                for (int k = 0; k < kNNBatch; ++k) r[k] = cx0 + k < gc[0] ? rep[(cz * kTGc + cy) * kTGc + cx0 + k] : -1;
#pragma unroll
                for (int k = 0; k < kNNBatch; ++k) {
                    if (r[k] < 0) continue;
                    float d2 = 0.f;
                    const int cc[3] = {cx0 + k, cy, cz};
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        if (!(g.cs[a] < INFINITY)) continue;
                        const float l = g.o[a] + (float)(cc[a] * kTCoarse) * g.cs[a] - g.slack[a];
                        const float h = g.o[a] + (float)min((cc[a] + 1) * kTCoarse, g.g[a]) * g.cs[a] + g.slack[a];
                        const float d = fmaxf(fmaxf(l - L.p[a], L.p[a] - h), 0.f);
                        d2 += d * d;
                    }
                    if (!__any(!(d2 * 0.9997f - g.abs_slack > L.min_d))) continue;
                    float fc[9];
#pragma unroll
                    for (int j = 0; j < 9; ++j) fc[j] = face[(size_t)r[k] * 9 + j];       // wave-uniform: scalar loads
                    L.eval(r[k], fc);
                }
            }
    share_best<kTriWaves>(s_pack, part, lane, L.min_d, L.min_idx);     // (index -1 is the largest)
    if (part == 0 && i < n) bound[i] = pack_best(L.min_d, L.min_idx);
}

__global__ __launch_bounds__(kTriWaves * 64) void k_tri_far_rows(const float *__restrict__ pts, const float *__restrict__ face,
                                                                 const float *__restrict__ nfb, const TGrid *__restrict__ gp,
                                                                 const int *__restrict__ cellStart, const int *__restrict__ list,
                                                                 const int *__restrict__ farList, const int *__restrict__ nFar,
                                                                 unsigned long long *bound, size_t slice, int P, int Fmax)
{
    __shared__ unsigned long long s_pack[kTriWaves][64];
    __shared__ unsigned bits[kTriBitWords];
    const int sb = blockIdx.z;
    pts += (size_t)sb * P * 3; face += (size_t)sb * Fmax * 9; nfb += sb;
    SHAPE(gp); SHAPE(cellStart); SHAPE(list); SHAPE(farList); SHAPE(nFar); SHAPE(bound);
    const int n = *nFar;
    if ((int)blockIdx.x * 64 >= n) return;                          // whole block idle
    const int lane = threadIdx.x & 63;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 64 + lane;
    const int ii = i < n ? i : n - 1;                               // idle lanes shadow the last far point
    const int q = farList[ii];
    const TGrid g = *gp;
    const int nf = (int)nfb[0];
    const bool dedupe = nf <= kTriBitWords * 32;
    if (dedupe) {
        for (int w = threadIdx.x; w < (nf + 31) / 32; w += kTriWaves * 64) bits[w] = 0u;
        __syncthreads();
    }
    TriLane L;
    L.p[0] = pts[q * 3]; L.p[1] = pts[q * 3 + 1]; L.p[2] = pts[q * 3 + 2];
    unpack_best(bound[ii], L.min_d, L.min_idx);                    // as k_tri_far_bound left it (other slices may have improved it)
    const int rows = g.g[1] * g.g[2];
    for (int r = blockIdx.y * kTriWaves + part; r < rows; r += kTriWaves * kTriSlices) {
        const int cy = r % g.g[1], cz = r / g.g[1];
        const float dy = slab_dist(g, 1, cy, L.p[1]), dz = slab_dist(g, 2, cz, L.p[2]);
        // a cell at distance d is out of reach when 0.9998 d^2 - abs_slack > best (k_tri_query_coop); 0.9997 covers the
        // rounding of this test itself
        const float rem = (L.min_d + g.abs_slack) * (1.0f / 0.9997f) - dy * dy - dz * dz;
        const bool need = !(rem < 0.f);                             // NaN points need everything (and select nothing)
        if (!__any(need)) continue;
        const float rx = sqrtf(fmaxf(rem, 0.f)) * 1.00001f;
        int x0 = need ? grid_cell(L.p[0] - rx - g.slack[0], g.o[0], g.inv[0], g.g[0]) : g.g[0] - 1;
        int x1 = need ? grid_cell(L.p[0] + rx + g.slack[0], g.o[0], g.inv[0], g.g[0]) : 0;
        if (need && !(rx < INFINITY)) { x0 = 0; x1 = g.g[0] - 1; }
#pragma unroll  // wave_min's and wave_max's order (wave.hpp); written out, a call changes this kernel's instruction stream
        for (int off = 32; off > 0; off >>= 1) {
            x0 = min(x0, __shfl_xor(x0, off));
            x1 = max(x1, __shfl_xor(x1, off));
        }
        x0 = __builtin_amdgcn_readfirstlane(x0);
        x1 = __builtin_amdgcn_readfirstlane(x1);
        const int c0 = r * g.g[0];
        const int s = cellStart[c0 + x0], e = cellStart[c0 + x1 + 1];
        if (dedupe) L.run<true>(face, list, s, e, bits, lane);
        else L.run<false>(face, list, s, e, bits, lane);
    }
    share_best<kTriWaves>(s_pack, part, lane, L.min_d, L.min_idx);
    if (part == 0 && i < n) atomicMin(&bound[i], pack_best(L.min_d, L.min_idx));
}

__global__ __launch_bounds__(256) void k_tri_far_final(const unsigned long long *__restrict__ bound, const int *__restrict__ nFar,
                                                       const int *__restrict__ farList, float *closest_d, float *closest_f, size_t slice, int P)
{
    const int sb = blockIdx.y;
    closest_d += (size_t)sb * P; closest_f += (size_t)sb * P;
    SHAPE(bound); SHAPE(nFar); SHAPE(farList);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *nFar) return;
    const unsigned long long v = bound[i];
    const int q = farList[i];
    closest_d[q] = __int_as_float((int)(v >> 32));
    closest_f[q] = (float)(int)(unsigned)v;
}

// per-point gradient contributions of the backward kernel (back.cu:591-686): up to 9 values
// for up to 3 vertices of the saved face.  Returns the number of (slot,value) pairs written.
// Gradient of one point's value with respect to the nine coordinates of its nearest face: g9[s], and the mask of the
// entries the reference's backward ADDS to (it also adds the zeros of the far edge endpoint, which matter only when the
// incoming gradient is not finite).  Everything is indexed statically — a (slot, value) list walked with a run-time count
// and corners addressed as fc + i * 3 put the lists and the corner array into scratch memory (48 bytes per lane, and 81
// compares per point to undo the list) in all three backward kernels.
__device__ __forceinline__ unsigned tri_dist_point_grad9(const float *fc, const float *p, float gp, float *g9)
{
    float ret[3] = {0.f, 0.f, 0.f}, ip[3];
    min_triangle_distance<true>(fc, fc + 3, fc + 6, p, ret, ip, 9999999.0f);     // back.cu:628
#pragma unroll
    for (int s = 0; s < 9; ++s) g9[s] = 0.f;
    auto corner = [&](int c, int k) { return c == 0 ? fc[k] : (c == 1 ? fc[3 + k] : fc[6 + k]); };
    if (ret[0] == 0) {                                              // :630-651, cuda_gradient_triangle_distance :439-483
        const float *a = fc, *b = fc + 3, *c = fc + 6;
        float ip2[3], t;
        plane_project(a, b, c, p, ip2, t);
        const float k1 = (b[1] - c[1]) * (ip2[0] - c[0]) + (c[0] - b[0]) * (ip2[1] - c[1]);
        const float k2 = (a[0] - c[0]) * (ip2[1] - c[1]) + (c[1] - a[1]) * (ip2[0] - c[0]);
        const float k3 = (b[1] - c[1]) * (a[0] - c[0]) + (c[0] - b[0]) * (a[1] - c[1]);
        float grad[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (k3 != 0) {
            const float l1 = k1 / k3, l2 = k2 / k3, l3 = 1 - l1 - l2;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                grad[k] = 2 * (ip2[k] - p[k]) * l1;
                grad[3 + k] = 2 * (ip2[k] - p[k]) * l2;
                grad[6 + k] = 2 * (ip2[k] - p[k]) * l3;
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) g9[k] = gp * grad[k];
        return 0x1FFu;
    }
    if (ret[0] == 1) {                                              // :652-670
        const int i1 = (int)ret[2], i2 = (i1 + 1) % 3;
        // cuda_gradient_line_distance (:291-317): the second assignment of grad[0..2] wins, grad[3..5] stays 0
        float A[3], B[3], PA[3], BA[3], v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { A[k] = corner(i1, k); B[k] = corner(i2, k); PA[k] = p[k] - A[k]; BA[k] = B[k] - A[k]; }
        const float t = dot3(PA, BA) / divide_non_zero(dot3(BA, BA));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float tmp = B[k] * t;
            float ipk = A[k] * (1 - t);
            ipk = ipk + tmp;
            v[k] = gp * (2 * (ipk - p[k]) * (t));
        }
        const float z = gp * 0.0f;
#pragma unroll
        for (int s = 0; s < 9; ++s) g9[s] = s / 3 == i1 ? v[s % 3] : (s / 3 == i2 ? z : 0.f);
        return (7u << (3 * i1)) | (7u << (3 * i2));
    }
    if (ret[0] == 2) {                                              // :671-685
        const int iv = (int)ret[2];
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            float gl = corner(s / 3, s % 3) - p[s % 3];
            gl = gl * 1.0f;
            g9[s] = s / 3 == iv ? 2 * gp * gl : 0.f;
        }
        return 7u << (3 * iv);
    }
    return 0u;
}

__global__ __launch_bounds__(256) void k_tri_dist_bwd_atomic(const float *__restrict__ pts, const float *__restrict__ face,
                                                             const float *__restrict__ closest_f,
                                                             const float *__restrict__ dl_dd, float *dldface, int P, int F)
{
    const int b = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const size_t i = (size_t)b * P + q;
    const int fi = (int)closest_f[i];                               // back.cu:618
    if (fi < 0 || fi >= F) return;                                  // the reference would read out of bounds
    float fc[9];
    const float *src = face + ((size_t)b * F + fi) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) fc[k] = src[k];
    const float p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
    float g9[9];
    const unsigned touched = tri_dist_point_grad9(fc, p, dl_dd[i], g9);
    float *g = dldface + ((size_t)b * F + fi) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if (touched >> k & 1u) unsafeAtomicAdd(g + k, g9[k]);                   // back.cu:640-683
}

// The same, walking the points in the FORWARD's order (sorted by grid cell): the 64 points of a wave are neighbours in
// space and share a handful of closest faces, so the wave adds up the contributions per distinct face first (butterfly over
// the lanes holding that face) and issues nine atomics per distinct face instead of up to nine per point — the atomics on
// ~36 k addresses per shape were what bounded the kernel above (0.37 ms per 8 x 97 k points).
__global__ __launch_bounds__(256) void k_tri_dist_bwd_grouped(const float *__restrict__ pts, const float *__restrict__ face,
                                                              const float *__restrict__ closest_f, const float *__restrict__ dl_dd,
                                                              const int *__restrict__ order, float *dldface, int P, int F)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    const int q = slot < P ? order[(size_t)b * P + slot] : -1;
    const size_t i = (size_t)b * P + (q >= 0 ? q : 0);
    int fi = q >= 0 ? (int)closest_f[i] : -1;                       // back.cu:618
    if (fi >= F) fi = -1;                                           // the reference would read out of bounds
    float gsum[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (fi >= 0) {
        float fc[9];
        const float *src = face + ((size_t)b * F + fi) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) fc[k] = src[k];
        const float p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
        float g9[9];
        const unsigned touched = tri_dist_point_grad9(fc, p, dl_dd[i], g9);
#pragma unroll
        for (int s = 0; s < 9; ++s)
            if (touched >> s & 1u) gsum[s] += g9[s];
    }
    unsigned long long todo = __ballot(fi >= 0);
    while (todo) {
        const int L = __ffsll((long long)todo) - 1;
        const int key = __builtin_amdgcn_readlane(fi, L);
        const bool mine = fi == key;
        todo &= ~__ballot(mine);
        float v[9];
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            v[s] = mine ? gsum[s] : 0.f;
#pragma unroll  // wave_sum's order (wave.hpp); written out, a call changes this kernel's instruction stream
            for (int off = 32; off > 0; off >>= 1) v[s] += __shfl_xor(v[s], off);
        }
        if (lane == L) {
            float *g = dldface + ((size_t)b * F + key) * 9;
#pragma unroll
            for (int s = 0; s < 9; ++s)
                if (v[s] != 0.f) unsafeAtomicAdd(g + s, v[s]);           // back.cu:640-683
        }
    }
}

// deterministic backward: (face, point) pairs sorted by face then point; one lane per face adds
// its points' contributions in ascending point order == the serial order of the CPU oracle.
__global__ __launch_bounds__(256) void k_bwd_keys(const float *__restrict__ closest_f, long long n, int P, int F,
                                                  unsigned long long *key)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / P);
    const int fi = (int)closest_f[i];
    const unsigned long long fkey = (fi < 0 || fi >= F) ? 0xFFFFFFFFull : (unsigned long long)((long long)b * F + fi);
    key[i] = (fkey << 32) | (unsigned long long)(i % P);
}

__global__ __launch_bounds__(256) void k_tri_dist_bwd_sorted(const float *__restrict__ pts, const float *__restrict__ face,
                                                             const float *__restrict__ dl_dd,
                                                             const unsigned long long *__restrict__ skey, long long n, int P,
                                                             int F, float *dldface)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = skey[i];
    const unsigned long long fkey = k >> 32;
    if (fkey == 0xFFFFFFFFull) return;
    if (i > 0 && (skey[i - 1] >> 32) == fkey) return;               // not the head of this face's segment
    const int b = (int)(fkey / (unsigned long long)F);
    float fc[9];
    const float *src = face + (size_t)fkey * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) fc[j] = src[j];
    float acc[9];
    float *g = dldface + (size_t)fkey * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = g[j];
    for (long long y = i; y < n && (skey[y] >> 32) == fkey; ++y) {
        const size_t pi = (size_t)b * P + (size_t)(skey[y] & 0xFFFFFFFFull);
        const float p[3] = {pts[pi * 3], pts[pi * 3 + 1], pts[pi * 3 + 2]};
        float g9[9];
        const unsigned touched = tri_dist_point_grad9(fc, p, dl_dd[pi], g9);
#pragma unroll
        for (int s = 0; s < 9; ++s)
            if (touched >> s & 1u) acc[s] += g9[s];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) g[j] = acc[j];
}

}  // namespace surf
}  // namespace deftet

using namespace deftet;
using namespace deftet::surf;

#ifdef TRI_STATS
extern "C" int deftet_debug_tri_stats(unsigned long long *out16, int reset)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tri_stats), sizeof(g_tri_stats)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_tri_stats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// the per-shape scratch slice of the grid search: ONE description of the layout, used for the size and for the pointers
struct TriSlice {
    float *part; TGrid *grid;
    int *cnt, *start, *fill, *list, *wide, *farList, *counters, *farFlag, *farOff;
    unsigned long long *bound;
    int *rep, *ptStart, *chunkCount, *chunkStart;
    float4 *sph;
    uint2 *frange;
    int *pcount, *pstart;
    int2 *prank;
    size_t lay(void *base, int P, int Fmax)
    {
        const size_t nc = (size_t)kTGMax * kTGMax * kTGMax + 1, F = (size_t)(Fmax > 0 ? Fmax : 0), Pn = (size_t)(P > 0 ? P : 0);
        Arena A(base);
        part = A.take<float>(kTParts * 8);
        grid = A.take<TGrid>(1);
        cnt = A.take<int>(nc); start = A.take<int>(nc); fill = A.take<int>(nc);
        list = A.take<int>(F * kTMaxCells + 1); wide = A.take<int>(F + 1);
        farList = A.take<int>(Pn + 1); counters = A.take<int>(8);
        farFlag = A.take<int>(Pn + 1); farOff = A.take<int>(Pn + 1);
        bound = A.take<unsigned long long>(Pn + 1);
        rep = A.take<int>(kTGc * kTGc * kTGc);
        ptStart = A.take<int>(kTRows + 2); chunkCount = A.take<int>(kTRows + 2); chunkStart = A.take<int>(kTRows + 2);
        sph = A.take<float4>(F + 1);
        frange = A.take<uint2>(F + 1);
        pcount = A.take<int>(nc); pstart = A.take<int>(nc + 1);
        prank = A.take<int2>(Pn + 1);
        return A.end();
    }
};
// per-shape scratch slices for a launch group of nS <= kBatchShapes shapes; behind them the cell keys and the point order of
// all shapes of the group in the cells' order (P entries per shape each, one spare)
struct TriLayout {
    TriSlice S;                                                       // slice 0; the kernels rebase to their shape by `slice` bytes
    size_t slice, bytes;
    unsigned *pskey, *order;
};
static TriLayout tri_layout(int nS, int P, int Fmax, void *ws)
{
    TriLayout L{};
    L.slice = L.S.lay(ws, P, Fmax);
    const size_t nAll = (size_t)nS * (size_t)(P > 0 ? P : 0);
    Arena T(static_cast<char *>(ws) + L.slice * nS);
    L.pskey = T.take<unsigned>(nAll + 1);
    L.order = T.take<unsigned>(nAll + 1);
    L.bytes = L.slice * nS + T.end();
    return L;
}
extern "C" size_t deftet_tri_dist_workspace_bytes(int B, int P, int Fmax) { return tri_layout(group_shapes(B), P, Fmax, nullptr).bytes; }

// the grid search for a GROUP of nS <= kBatchShapes shapes: one launch per kernel for the whole group
static int tri_dist_group(const float *pts, const float *face, const float *nfb, float *cd, float *cf, int nS, int P, int Fmax, void *ws,
                          hipStream_t st, int *order_out)
{
    const size_t nc = (size_t)kTGMax * kTGMax * kTGMax + 1;
    const TriLayout TL = tri_layout(nS, P, Fmax, ws);                 // at most what the entry checked: a group is no larger than the largest
    const TriSlice &L = TL.S;
    const size_t slice = TL.slice;
    const size_t nAll = (size_t)nS * P;
    unsigned *pskey = TL.pskey, *order = TL.order;
    const dim3 blk(256);
    DEFTET_LAUNCH(k_tri_face_stats, dim3(kTParts, nS), blk, st, face, nfb, L.part, slice, Fmax, L.cnt, L.fill, L.counters, L.rep, (int)nc, kTGc * kTGc * kTGc,
                  L.pcount);
    DEFTET_LAUNCH(k_tri_grid, dim3(nS), dim3(64), st, (const float *)L.part, L.grid, slice);
    DEFTET_LAUNCH(k_tri_face_bin, dim3(blocks_for(Fmax, 256), nS), blk, st, face, nfb, (const TGrid *)L.grid, 0, L.cnt, (const int *)L.start, L.fill, L.list, L.wide,
                  L.counters, L.rep, slice, Fmax, L.sph, L.frange);
    DEFTET_LAUNCH(k_scan_excl, dim3(scan_tiles(nc), nS), dim3(kScanThreads), st, (const int *)L.cnt, L.start, (int)nc, slice, 0);
    DEFTET_LAUNCH(k_tri_face_bin, dim3(blocks_for(Fmax, 256), nS), blk, st, face, nfb, (const TGrid *)L.grid, 1, L.cnt, (const int *)L.start, L.fill, L.list, L.wide,
                  L.counters, L.rep, slice, Fmax, L.sph, L.frange);
    DEFTET_LAUNCH(k_tri_point_keys, dim3(blocks_for(P, 256), nS), blk, st, pts, P, (const TGrid *)L.grid, L.pcount, L.prank, slice);
    DEFTET_LAUNCH(k_scan_excl, dim3(scan_tiles(nc), nS), dim3(kScanThreads), st, (const int *)L.pcount, L.pstart, (int)nc, slice, 0);
    DEFTET_LAUNCH(k_tri_point_scatter, dim3(blocks_for(P, 256), nS), blk, st, P, (const int2 *)L.prank, (const int *)L.pstart, order, pskey, slice);
    if (order_out) DEFTET_HIP(hipMemcpyAsync(order_out, order, nAll * 4, hipMemcpyDeviceToDevice, st));   // for the grouped backward
    DEFTET_LAUNCH(k_tri_chunks, dim3(blocks_for(kTRows + 1, 256), nS), blk, st, (const int *)L.pstart, L.ptStart, L.chunkCount, slice);
    DEFTET_LAUNCH(k_scan_excl, dim3(scan_tiles(kTRows + 1), nS), dim3(kScanThreads), st, (const int *)L.chunkCount, L.chunkStart, kTRows + 1, slice, 0);
    {
        const long long maxChunks = (long long)(P + 63) / 64 + (long long)kTRows;
        DEFTET_LAUNCH(k_tri_query_coop, dim3((unsigned)std::min<long long>(maxChunks, kTriQueryBlocks), nS), dim3(kTriChunkWaves * 64), st, pts,
                      face, nfb, P, (const TGrid *)L.grid, (const int *)L.start, (const int *)L.list, (const int *)L.wide, (const int *)L.counters, cd, cf,
                      L.farFlag, (const unsigned *)order, (const int *)L.ptStart, (const int *)L.chunkStart, (const int *)L.rep, slice, Fmax, (const float4 *)L.sph,
                      (const unsigned *)pskey, (const uint2 *)L.frange);
    }
    // the far path (counters: [0] wide faces, [1] far points)
    DEFTET_LAUNCH(k_scan_excl, dim3(scan_tiles(P), nS), dim3(kScanThreads), st, (const int *)L.farFlag, L.farOff, P, slice, 0);
    DEFTET_LAUNCH(k_tri_compact, dim3(blocks_for(P, 256), nS), blk, st, (const int *)L.farFlag, (const int *)L.farOff, (const unsigned *)order, P, L.farList,
                  L.counters + 1, slice);
    DEFTET_LAUNCH(k_tri_far_bound, dim3(blocks_for(P, 64), nS), dim3(kTriWaves * 64), st, pts, face, (const TGrid *)L.grid, (const int *)L.wide,
                  (const int *)L.counters, (const int *)L.rep, (const int *)L.farList, (const int *)(L.counters + 1), L.bound, slice, P, Fmax);
    DEFTET_LAUNCH(k_tri_far_rows, dim3(blocks_for(P, 64), kTriSlices, nS), dim3(kTriWaves * 64), st, pts, face, nfb, (const TGrid *)L.grid,
                  (const int *)L.start, (const int *)L.list, (const int *)L.farList, (const int *)(L.counters + 1), L.bound, slice, P, Fmax);
    DEFTET_LAUNCH(k_tri_far_final, dim3(blocks_for(P, 256), nS), blk, st, (const unsigned long long *)L.bound, (const int *)(L.counters + 1),
                  (const int *)L.farList, cd, cf, slice, P);
    return DEFTET_OK;
}

// workspace == NULL: the scalar-stream brute force; otherwise the grid search (both exact).
// order_out (int32 [B,P], may be NULL): the points of every shape in the order the grid search walked them (sorted by
// grid cell) — what deftet_tri_dist_bwd_order_f32 wants; written only on the grid path with n_max_face > 0.
extern "C" int deftet_tri_dist_fwd_order_f32(const float *pts, const float *face, const float *n_face_b, float *closest_d,
                                             float *closest_f, int32_t *order_out, int B, int P, int Fmax, void *workspace, size_t wsb,
                                             void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && P >= 0 && Fmax >= 0 && B <= 65535, "bad size");
    if (Fmax >= (1 << 24)) return set_error(DEFTET_ELIMIT, "n_face=%d does not fit a float-encoded index", Fmax);
    if (B == 0 || P == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(pts && n_face_b && closest_d && closest_f && (Fmax == 0 || face), "null pointer");
    hipStream_t st = as_stream(stream_);
    if (!workspace || Fmax == 0) {
        DEFTET_CHECK_ARG(!order_out, "the point order is only produced by the grid search (workspace and faces needed)");
        DEFTET_LAUNCH(k_tri_dist_fwd, dim3(blocks_for(P, 256), B), dim3(256), st, pts, face, n_face_b, closest_d, closest_f, P, Fmax);
        return DEFTET_OK;
    }
    DEFTET_TRY(workspace_ok("deftet_tri_dist_fwd*", workspace, wsb, tri_layout(group_shapes(B), P, Fmax, workspace).bytes));
    DEFTET_CHECK_ARG((long long)Fmax * kTMaxCells < 2147483647LL && (long long)P * 3 < 2147483647LL, "too many faces / points");
    for (int b0 = 0; b0 < B; b0 += kBatchShapes) {                   // groups of kBatchShapes shapes reuse the workspace (stream order)
        const int nS = std::min(kBatchShapes, B - b0);
        DEFTET_TRY(tri_dist_group(pts + (size_t)b0 * P * 3, face + (size_t)b0 * Fmax * 9, n_face_b + b0, closest_d + (size_t)b0 * P,
                                  closest_f + (size_t)b0 * P, nS, P, Fmax, workspace, st,
                                  order_out ? order_out + (size_t)b0 * P : nullptr));
    }
    return DEFTET_OK;
}

extern "C" int deftet_tri_dist_fwd_f32(const float *pts, const float *face, const float *n_face_b, float *closest_d,
                                       float *closest_f, int B, int P, int Fmax, void *workspace, size_t wsb, void *stream_)
{
    return deftet_tri_dist_fwd_order_f32(pts, face, n_face_b, closest_d, closest_f, nullptr, B, P, Fmax, workspace, wsb, stream_);
}

// The atomic backward with the forward's point order (deftet_tri_dist_fwd_order_f32): same sums, up to the order of the
// floating-point additions, from ~7x fewer atomics.
extern "C" int deftet_tri_dist_bwd_order_f32(const float *pts, const float *face, const float *closest_f, const float *dl_dd,
                                             const int32_t *order, float *dldface, int B, int P, int F, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && P >= 0 && F >= 0 && B <= 65535, "bad size");
    if (B == 0 || P == 0 || F == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(pts && face && closest_f && dl_dd && dldface && order, "null pointer");
    DEFTET_LAUNCH(k_tri_dist_bwd_grouped, dim3(blocks_for(P, 256), B), dim3(256), as_stream(stream_), pts, face, closest_f, dl_dd, order, dldface,
                  P, F);
    return DEFTET_OK;
}

// The deterministic backward between the allocation of its scratch and the release (the caller owns key, skey and tmp).
static int tri_dist_bwd_sorted(const float *pts, const float *face, const float *closest_f, const float *dl_dd, float *dldface, long long n,
                               int P, int F, unsigned long long *key, unsigned long long *skey, void *tmp, size_t tmpBytes, hipStream_t st)
{
    DEFTET_LAUNCH(k_bwd_keys, dim3(blocks_for(n, 256)), dim3(256), st, closest_f, n, P, F, key);
    DEFTET_TRY(prims::radix_sort_keys<unsigned long long>(key, skey, (size_t)n, 64, tmp, tmpBytes, st));
    DEFTET_LAUNCH(k_tri_dist_bwd_sorted, dim3(blocks_for(n, 256)), dim3(256), st, pts, face, dl_dd, skey, n, P, F, dldface);
    return DEFTET_OK;
}

extern "C" int deftet_tri_dist_bwd_f32(const float *pts, const float *face, const float *closest_f, const float *dl_dd,
                                       float *dldface, int B, int P, int F, int deterministic, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && P >= 0 && F >= 0 && B <= 65535, "bad size");
    if (B == 0 || P == 0 || F == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(pts && face && closest_f && dl_dd && dldface, "null pointer");
    hipStream_t st = as_stream(stream_);
    if (!deterministic) {
        DEFTET_LAUNCH(k_tri_dist_bwd_atomic, dim3(blocks_for(P, 256), B), dim3(256), st, pts, face, closest_f, dl_dd, dldface, P, F);
        return DEFTET_OK;
    }
    // deterministic mode allocates its own scratch (stream-ordered), it is a test/debug path
    const long long n = (long long)B * P;
    DEFTET_CHECK_ARG((long long)B * F < 0xFFFFFFFFLL, "too many faces for the deterministic path");
    // key, skey and the sort's temporary: released on every way out, and the first error is the one reported
    const size_t bytes[3] = {(size_t)n * 8, (size_t)n * 8, prims::radix_sort_temp_bytes<unsigned long long, unsigned>((size_t)n, false)};
    void *buf[3] = {nullptr, nullptr, nullptr};
    int rc = DEFTET_OK;
    for (int k = 0; k < 3 && rc == DEFTET_OK; ++k) {
        const hipError_t e = hipMallocAsync(&buf[k], bytes[k], st);
        if (e != hipSuccess) {
            buf[k] = nullptr;
            rc = set_error(DEFTET_ELAUNCH, "hipMallocAsync of %zu bytes failed: %s", bytes[k], hipGetErrorString(e));
        }
    }
    if (rc == DEFTET_OK)
        rc = tri_dist_bwd_sorted(pts, face, closest_f, dl_dd, dldface, n, P, F, (unsigned long long *)buf[0], (unsigned long long *)buf[1],
                                 buf[2], bytes[2], st);
    for (int k = 0; k < 3; ++k) {
        if (!buf[k]) continue;
        const hipError_t e = hipFreeAsync(buf[k], st);
        if (e != hipSuccess && rc == DEFTET_OK) rc = set_error(DEFTET_ELAUNCH, "hipFreeAsync failed: %s", hipGetErrorString(e));
    }
    return rc;
}
