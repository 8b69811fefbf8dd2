// tet_refine.hip — conforming selective refinement of a tet list: red-green closure on edge marks (gfx950).
//
// The reference refines selectively with generate_subdivision(subdiv_sig) (3_model/prepare_for_wz.py:255-301, driven by
// 3_model/deftet.py:369-392): a split tet puts midpoints on edges and faces its unsplit neighbour still owns whole.  Here the
// refinement is closed so that every interior face keeps exactly two owners.  Over the unique edge list and tet_edge [T,6] of
// deftet_tet_edges_i64 (local slots 0 ab, 1 ac, 2 ad, 3 bc, 4 bd, 5 cd):
//
//   marks     every edge of a selected tet is marked; then, until nothing changes, a face of a tet with two of its three edges
//             marked gets the third.  The rule only ever sets marks and what it sets depends on set marks alone (monotone), so
//             the closed set is the least fixed point: the same set whatever order the rule is applied in.
//   count     ranks of the marked edges (exclusive scan), children per tet (1, 2, 4, 4, 8 for 0, 1, 2, 3, 6 marked slots) and
//             their scan, the totals, and `bad`: a pattern that is none of {none, one edge, two opposite edges, the three
//             edges of a face, all six} — these five are the only sets of slots in which no face has exactly two, so closed
//             marks hold no other, whatever ids tet_edge holds —, a tet_edge entry outside [0, E) or a marked edge with an end
//             outside [0, P).
//   fill      vertex P + r = the midpoint of marked edge r, (x[a] + x[b]) / 2.0f as k_subdiv_points; the children of a tet
//             contiguous, tets in parent order.  Every child replaces corners of its parent by midpoints of the parent's own
//             edges at those corners, so it keeps the parent's orientation.
//
// Integer work only (the midpoints are one fp32 add and one division each): the same bits on every run.
#include "common.hpp"

#include "prims.hpp"
#include "wave.hpp"

namespace deftet {
namespace refine {

using u32 = unsigned int;

constexpr int kThreads = 256;
constexpr int kMaxSweeps = 64;                                           // sweeps one call may enqueue

__constant__ int kEnds[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};   // kEdgeEnds of builders.hip
__constant__ int kSlotOf[4][4] = {{-1, 0, 1, 2}, {0, -1, 3, 4}, {1, 3, -1, 5}, {2, 4, 5, -1}};
__constant__ int kFaceCorner[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};   // abc, abd, acd, bcd, corners ascending
// their slots {0,1,3}, {0,2,4}, {1,2,5}, {3,4,5} as bit masks
__host__ __device__ constexpr u32 face_mask(int f) { return f == 0 ? 0x0Bu : f == 1 ? 0x15u : f == 2 ? 0x26u : 0x38u; }

// the face rule inside one tet, to its fixed point: a pass that changes something completes a face and there are four faces, so
// four passes either meet a pass that changes nothing or end with every edge marked
__device__ __forceinline__ u32 close_local(u32 m)
{
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
#pragma unroll
        for (int f = 0; f < 4; ++f)
            if (__popc(m & face_mask(f)) >= 2) m |= face_mask(f);
    }
    return m;
}

// children of a closed pattern, -1 for an illegal one
__device__ __forceinline__ int children_of(u32 m)
{
    const int n = __popc(m);
    if (n == 0) return 1;
    if (n == 1) return 2;
    if (n == 6) return 8;
    if (n == 2) return (m == 0x21u || m == 0x12u || m == 0x0Cu) ? 4 : -1;   // slots e and 5 - e
    if (n == 3) return (m == face_mask(0) || m == face_mask(1) || m == face_mask(2) || m == face_mask(3)) ? 4 : -1;
    return -1;
}

__device__ __forceinline__ u32 mload(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the six edge ids of a tet; false (nothing to follow) when one lies outside [0, E)
__device__ __forceinline__ bool load_row(const long long *__restrict__ tet_edge, int t, int E, int (&e)[6])
{
    bool ok = true;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const long long x = tet_edge[(size_t)t * 6 + s];
        ok = ok && x >= 0 && x < (long long)E;
        e[s] = (int)x;
    }
    return ok;
}

// marks of a selected tet's edges.  Plain stores of 1 over a zeroed buffer: lanes that meet on an edge write the same word.
__global__ __launch_bounds__(kThreads) void k_refine_init(const long long *__restrict__ tet_edge, const unsigned char *__restrict__ select,
                                                          int T, int E, u32 *marks, int *bad)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    int e[6];
    if (!load_row(tet_edge, t, E, e)) { *bad = 1; return; }
    if (!select[t]) return;
#pragma unroll
    for (int s = 0; s < 6; ++s) marks[e[s]] = 1u;
}

// One in-place sweep, one tet per lane: read the six marks, close the pattern inside the tet, set what is missing.  Marks only go
// 0 -> 1 and no lane waits for another; a mark another lane sets during the sweep is seen or not, and either way the sweep only
// sets marks of the least fixed point.  *count = marks this sweep set (the old value of the atomic or tells who set it: every
// mark is counted once).  A lane that misses a mark set during the sweep may set nothing although the state is not closed yet;
// but then that other lane counted.  So a sweep that counts 0 saw, in every lane, a state that nobody wrote during the sweep —
// the state the launch began with, complete behind the launch boundary — and found nothing to add to it: count 0 proves closure.
__global__ __launch_bounds__(kThreads) void k_refine_sweep(const long long *__restrict__ tet_edge, int T, int E, u32 *marks, int *count)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    int added = 0;
    int e[6];
    if (t < T && load_row(tet_edge, t, E, e)) {
        u32 m = 0;
#pragma unroll
        for (int s = 0; s < 6; ++s) m |= (mload(marks + e[s]) & 1u) << s;
        const u32 add = close_local(m) & ~m;
#pragma unroll
        for (int s = 0; s < 6; ++s)
            if ((add >> s) & 1u)
                added += __hip_atomic_fetch_or(marks + e[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u ? 1 : 0;
    }
    added = wave_sum(added);                                             // (every lane of the wave is here: none has returned)
    if ((threadIdx.x & 63) == 0 && added) atomicAdd(count, added);
}

// a marked edge must have both ends in [0, P): the fill pass reads the points there
__global__ __launch_bounds__(kThreads) void k_refine_edge_check(const long long *__restrict__ edges, const u32 *__restrict__ marks, int E, int P,
                                                                int *bad)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= E || !marks[e]) return;
    const long long a = edges[(size_t)e * 2], b = edges[(size_t)e * 2 + 1];
    if (a < 0 || b < 0 || a >= (long long)P || b >= (long long)P) *bad = 1;
}

__device__ __forceinline__ u32 pattern_of(const u32 *__restrict__ marks, const int (&e)[6])
{
    u32 m = 0;
#pragma unroll
    for (int s = 0; s < 6; ++s) m |= (marks[e[s]] & 1u) << s;
    return m;
}

// a tet that cannot be refined (an entry out of range, an illegal pattern) is counted in bad and copied as one child
__global__ __launch_bounds__(kThreads) void k_refine_children(const long long *__restrict__ tet_edge, const u32 *__restrict__ marks, int T, int E,
                                                              int *n_child, int *bad)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    int e[6];
    int n = -1;
    if (load_row(tet_edge, t, E, e)) n = children_of(pattern_of(marks, e));
    if (n < 0) { *bad = 1; n = 1; }
    n_child[t] = n;
}

// totals[0] = M, totals[1] = T' (totals[2] is bad)
__global__ void k_refine_totals(const u32 *__restrict__ marks, const int *__restrict__ rank, int E, const int *__restrict__ n_child,
                                const int *__restrict__ child_pos, int T, int *totals)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = E > 0 ? rank[E - 1] + (int)(marks[E - 1] & 1u) : 0;
        totals[1] = T > 0 ? child_pos[T - 1] + n_child[T - 1] : 0;
    }
}

// rows [0, P) of dst are src; row P + rank[e] is the midpoint of marked edge e
__global__ __launch_bounds__(kThreads) void k_refine_copy(const float *__restrict__ src, long long n, float *dst)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

__global__ __launch_bounds__(kThreads) void k_refine_midpoints(const float *__restrict__ src, const long long *__restrict__ edges,
                                                               const u32 *__restrict__ marks, const int *__restrict__ rank, int P, int E, int K,
                                                               int M, float *dst)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)E * K) return;
    const int e = (int)(i / K), c = (int)(i % K);
    if (!marks[e]) return;
    const int r = rank[e];
    if (r < 0 || r >= M) return;                                         // (a workspace no count pass wrote: nothing is written)
    const long long a = edges[(size_t)e * 2], b = edges[(size_t)e * 2 + 1];
    if (a < 0 || b < 0 || a >= (long long)P || b >= (long long)P) return;  // (counted in bad by the count pass)
    dst[(size_t)(P + r) * K + c] = (src[(size_t)a * K + c] + src[(size_t)b * K + c]) / 2.0f;
}

__global__ __launch_bounds__(kThreads) void k_refine_split(const long long *__restrict__ edges, const u32 *__restrict__ marks,
                                                           const int *__restrict__ rank, int E, int M, long long *edges_split)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= E || !marks[e]) return;
    const int r = rank[e];
    if (r < 0 || r >= M) return;
    edges_split[(size_t)r * 2] = edges[(size_t)e * 2];
    edges_split[(size_t)r * 2 + 1] = edges[(size_t)e * 2 + 1];
}

struct ChildWriter {
    long long *tet_new, *parent;
    unsigned char *kind;
    long long at, cap;
    int t, k;
    __device__ __forceinline__ void put(long long a, long long b, long long c, long long d)
    {
        if (at >= 0 && at < cap) {                                       // (cap = the count pass's T': always inside)
            long long *o = tet_new + (size_t)at * 4;
            o[0] = a; o[1] = b; o[2] = c; o[3] = d;
            parent[at] = t;
            kind[at] = (unsigned char)k;
        }
        ++at;
    }
    __device__ __forceinline__ void put(const long long (&v)[4]) { put(v[0], v[1], v[2], v[3]); }
};

// the parent with corners replaced: i0 by m0, and i1 by m1 / i2 by m2 where given
__device__ __forceinline__ void put_with(ChildWriter &w, const long long (&v)[4], int i0, long long m0, int i1 = -1, long long m1 = 0, int i2 = -1,
                                         long long m2 = 0)
{
    long long c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = i == i0 ? m0 : i == i1 ? m1 : i == i2 ? m2 : v[i];
    w.put(c);
}

__global__ __launch_bounds__(kThreads) void k_refine_tets(const long long *__restrict__ tet, const long long *__restrict__ tet_edge,
                                                          const u32 *__restrict__ marks, const int *__restrict__ rank,
                                                          const int *__restrict__ child_pos, int T, int E, int P, long long cap,
                                                          long long *tet_new, long long *parent, unsigned char *kind)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    long long v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = tet[(size_t)t * 4 + i];
    int e[6];
    u32 m = 0;
    if (load_row(tet_edge, t, E, e)) m = pattern_of(marks, e);
    if (children_of(m) < 0) m = 0;                                       // (bad was raised by the count pass: one child, the parent)
    ChildWriter w{tet_new, parent, kind, (long long)child_pos[t], cap, t, (int)__popc(m)};
    long long mid[6];                                                    // midpoint vertex of a marked slot
#pragma unroll
    for (int s = 0; s < 6; ++s) mid[s] = ((m >> s) & 1u) ? (long long)P + rank[e[s]] : -1;
    const int n = __popc(m);
    if (n == 0) {
        w.put(v);
    } else if (n == 1) {                                                 // edge (p, q): v[q] = m, then v[p] = m
        const int s = __ffs((int)m) - 1, p = kEnds[s][0], q = kEnds[s][1];
        put_with(w, v, q, mid[s]);
        put_with(w, v, p, mid[s]);
    } else if (n == 2) {                                                 // opposite edges e0 < e1 = 5 - e0
        const int s0 = __ffs((int)m) - 1, s1 = 5 - s0;
        const int p0 = kEnds[s0][0], q0 = kEnds[s0][1], p1 = kEnds[s1][0], q1 = kEnds[s1][1];
        put_with(w, v, q0, mid[s0], q1, mid[s1]);
        put_with(w, v, q0, mid[s0], p1, mid[s1]);
        put_with(w, v, p0, mid[s0], q1, mid[s1]);
        put_with(w, v, p0, mid[s0], p1, mid[s1]);
    } else if (n == 3) {                                                 // one face, corners p < q < r; the fourth corner stays
        const int f = m == face_mask(0) ? 0 : m == face_mask(1) ? 1 : m == face_mask(2) ? 2 : 3;
        const int p = kFaceCorner[f][0], q = kFaceCorner[f][1], r = kFaceCorner[f][2];
        const long long pq = mid[kSlotOf[p][q]], pr = mid[kSlotOf[p][r]], qr = mid[kSlotOf[q][r]];
        put_with(w, v, q, pq, r, pr);
        put_with(w, v, p, pq, r, qr);
        put_with(w, v, p, pr, q, qr);
        put_with(w, v, p, pq, q, qr, r, pr);
    } else {                                                             // all six: the eight children of k_subdiv_tets, in its order
        const long long a = v[0], b = v[1], c = v[2], d = v[3];
        const long long ab = mid[0], ac = mid[1], ad = mid[2], bc = mid[3], bd = mid[4], cd = mid[5];
        w.put(a, ab, ac, ad); w.put(b, bc, ab, bd); w.put(c, ac, bc, cd); w.put(d, ad, cd, bd);
        w.put(ab, ac, ad, bd); w.put(ab, ac, bd, bc); w.put(cd, ac, bd, ad); w.put(cd, ac, bc, bd);
    }
}

// rank: exclusive scan of the marks; n_child / child_pos: children per tet and their exclusive scan
struct Layout {
    size_t bytes;
    int *rank, *n_child, *child_pos;
    void *scan;
    size_t scan_bytes;
};
static Layout layout(int T, int E, void *ws)
{
    Layout L{};
    Arena A(ws);
    L.rank = A.take<int>((size_t)E);
    L.n_child = A.take<int>((size_t)T);
    L.child_pos = A.take<int>((size_t)T);
    L.scan_bytes = prims::scan_temp_bytes<int>((size_t)(T > E ? T : E));
    L.scan = A.take<char>(L.scan_bytes);
    L.bytes = A.end();
    return L;
}

static int ex_scan(const Layout &L, const int *in, int *out, size_t n, hipStream_t st)
{
    return prims::scan<int, prims::Plus, true>(in, out, n, 0, prims::Plus(), L.scan, L.scan_bytes, st);
}

static int check_sizes(const char *who, int T, int E)
{
    DEFTET_CHECK_ARG(T >= 0 && E >= 0, "%s: negative size", who);
    DEFTET_CHECK_ARG(T <= 100000000, "%s: n_tet=%d too large (8 n_tet children must fit 31 bits)", who, T);
    DEFTET_CHECK_ARG((long long)E <= 6LL * T, "%s: n_edge=%d is more than 6 n_tet", who, E);
    return DEFTET_OK;
}

}  // namespace refine
}  // namespace deftet

using namespace deftet;
using namespace deftet::refine;

extern "C" size_t deftet_tet_refine_workspace_bytes(int n_tet, int n_edge)
{
    return layout(n_tet > 0 ? n_tet : 0, n_edge > 0 ? n_edge : 0, nullptr).bytes;
}

extern "C" int deftet_tet_refine_mark_i64(const int64_t *tet_edge_tx6, const uint8_t *select_t, int T, int E, int reset, int n_sweeps,
                                          uint32_t *marks_e, int32_t *sweep_counts, int32_t *bad, void *stream_)
{
    DEFTET_TRY(check_sizes("tet_refine_mark", T, E));
    DEFTET_CHECK_ARG(n_sweeps >= 0 && n_sweeps <= kMaxSweeps, "tet_refine_mark: n_sweeps=%d outside 0..%d", n_sweeps, kMaxSweeps);
    DEFTET_CHECK_ARG(bad && (n_sweeps == 0 || sweep_counts), "tet_refine_mark: null pointer: sweep_counts / bad");
    DEFTET_CHECK_ARG(E == 0 || marks_e, "tet_refine_mark: null pointer: marks");
    DEFTET_CHECK_ARG(T == 0 || (tet_edge_tx6 && (!reset || select_t)), "tet_refine_mark: null pointer: tet_edge / select");
    hipStream_t st = as_stream(stream_);
    if (n_sweeps) DEFTET_HIP(hipMemsetAsync(sweep_counts, 0, (size_t)n_sweeps * 4, st));
    if (reset) {
        DEFTET_HIP(hipMemsetAsync(bad, 0, 4, st));
        if (E) DEFTET_HIP(hipMemsetAsync(marks_e, 0, (size_t)E * 4, st));
        if (T) DEFTET_LAUNCH(k_refine_init, blocks_for(T, kThreads), dim3(kThreads), st, (const long long *)tet_edge_tx6, select_t, T, E, marks_e, bad);
    }
    if (T == 0 || E == 0) return DEFTET_OK;
    for (int s = 0; s < n_sweeps; ++s)
        DEFTET_LAUNCH(k_refine_sweep, blocks_for(T, kThreads), dim3(kThreads), st, (const long long *)tet_edge_tx6, T, E, marks_e, sweep_counts + s);
    return DEFTET_OK;
}

extern "C" int deftet_tet_refine_count_i64(const int64_t *tet_edge_tx6, const int64_t *edges_ex2, const uint32_t *marks_e, int n_point, int T,
                                           int E, int32_t *totals, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_sizes("tet_refine_count", T, E));
    DEFTET_CHECK_ARG(n_point >= 0, "tet_refine_count: negative size");
    DEFTET_CHECK_ARG(totals, "tet_refine_count: null pointer: totals");
    DEFTET_CHECK_ARG(T == 0 || tet_edge_tx6, "tet_refine_count: null pointer: tet_edge");
    DEFTET_CHECK_ARG(E == 0 || (edges_ex2 && marks_e), "tet_refine_count: null pointer: edges / marks");
    const Layout L = layout(T, E, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, L.bytes));
    hipStream_t st = as_stream(stream_);
    DEFTET_HIP(hipMemsetAsync(totals, 0, 12, st));
    if (E) {
        DEFTET_LAUNCH(k_refine_edge_check, blocks_for(E, kThreads), dim3(kThreads), st, (const long long *)edges_ex2, marks_e, E, n_point, totals + 2);
        DEFTET_TRY(ex_scan(L, (const int *)marks_e, L.rank, (size_t)E, st));
    }
    if (T) {
        DEFTET_LAUNCH(k_refine_children, blocks_for(T, kThreads), dim3(kThreads), st, (const long long *)tet_edge_tx6, marks_e, T, E, L.n_child, totals + 2);
        DEFTET_TRY(ex_scan(L, L.n_child, L.child_pos, (size_t)T, st));
    }
    DEFTET_LAUNCH(k_refine_totals, dim3(1), dim3(64), st, marks_e, (const int *)L.rank, E, (const int *)L.n_child, (const int *)L.child_pos, T, totals);
    return DEFTET_OK;
}

extern "C" int deftet_tet_refine_fill_f32(const int64_t *tet_tx4, const int64_t *tet_edge_tx6, const int64_t *edges_ex2, const uint32_t *marks_e,
                                          const float *points, const float *feat, int n_point, int T, int E, int n_feat, int n_split,
                                          long long n_tet_new, float *points_new, float *feat_new, int64_t *tet_new, int64_t *parent,
                                          uint8_t *kind, int64_t *edges_split, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_sizes("tet_refine_fill", T, E));
    DEFTET_CHECK_ARG(n_point >= 0 && n_feat >= 0 && n_split >= 0 && n_tet_new >= 0, "tet_refine_fill: negative size");
    DEFTET_CHECK_ARG(n_split <= E && n_tet_new <= 8LL * T, "tet_refine_fill: n_split / n_tet_new are not a count pass's totals");
    DEFTET_CHECK_ARG(T == 0 || (tet_tx4 && tet_edge_tx6), "tet_refine_fill: null pointer: tet / tet_edge");
    DEFTET_CHECK_ARG(E == 0 || (edges_ex2 && marks_e), "tet_refine_fill: null pointer: edges / marks");
    DEFTET_CHECK_ARG(n_point + n_split == 0 || (points && points_new), "tet_refine_fill: null pointer: points");
    DEFTET_CHECK_ARG(n_point + n_split == 0 || n_feat == 0 || (feat && feat_new), "tet_refine_fill: null pointer: features");
    DEFTET_CHECK_ARG(n_tet_new == 0 || (tet_new && parent && kind), "tet_refine_fill: null pointer: tet_new / parent / kind");
    DEFTET_CHECK_ARG(n_split == 0 || edges_split, "tet_refine_fill: null pointer: edges_split");
    const Layout L = layout(T, E, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, L.bytes));
    hipStream_t st = as_stream(stream_);
    const float *src[2] = {points, feat};
    float *dst[2] = {points_new, feat_new};
    const int width[2] = {3, n_feat};
    for (int k = 0; k < 2; ++k) {
        const int K = width[k];
        if (K == 0) continue;
        if (n_point)
            DEFTET_LAUNCH(k_refine_copy, blocks_for((size_t)n_point * K, kThreads), dim3(kThreads), st, src[k], (long long)n_point * K, dst[k]);
        if (n_split)
            DEFTET_LAUNCH(k_refine_midpoints, blocks_for((size_t)E * K, kThreads), dim3(kThreads), st, src[k], (const long long *)edges_ex2, marks_e,
                          (const int *)L.rank, n_point, E, K, n_split, dst[k]);
    }
    if (n_split)
        DEFTET_LAUNCH(k_refine_split, blocks_for(E, kThreads), dim3(kThreads), st, (const long long *)edges_ex2, marks_e, (const int *)L.rank, E, n_split,
                      (long long *)edges_split);
    if (T && n_tet_new)
        DEFTET_LAUNCH(k_refine_tets, blocks_for(T, kThreads), dim3(kThreads), st, (const long long *)tet_tx4, (const long long *)tet_edge_tx6, marks_e,
                      (const int *)L.rank, (const int *)L.child_pos, T, E, n_point, n_tet_new, (long long *)tet_new, (long long *)parent, kind);
    return DEFTET_OK;
}
