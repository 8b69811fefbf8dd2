// loop_subdivide.hip — Loop subdivision of triangle surfaces for CDNA4 / gfx950 (410): the topology of a face
// list (unique edges, the two incidence CSRs, crease / corner classification, the 1 -> 4 child faces), the operator S (new
// positions and attributes, [V+E] rows from [V]) or the limit projection ([V] rows from [V]), and the transpose of either.
//
// Rules (Warren's weights).  n = the number of edges at a vertex; an edge with a number of (face, local edge) incidences other
// than 2 is a CREASE (boundary and non-manifold edges alike); a vertex with no crease edge is smooth, with exactly two a crease
// vertex, with any other number a corner.
//   edge vertex   interior (a,b) with opposite corners (c,d):  3/8 a + 3/8 b + 1/8 c + 1/8 d;   crease: 1/2 a + 1/2 b
//   old vertex    smooth: (1 - n beta) v + beta sum of the neighbours, beta = 3/16 for n = 3, else 3/(8 n); n = 0: v
//                 crease: 3/4 v + 1/8 (the two crease neighbours);   corner: v
//   limit         smooth: (1 - n gamma) v + gamma sum, gamma = 1/(n + 3/(8 beta));  crease: 2/3 v + 1/6 (the two);  corner: v
//
// Orders of summation (fp32, no contraction, one accumulator from the first term, one term after the other — part of the result):
//   forward, old vertex: the own term, then the vertex's edge-end slots ascending (a crease vertex: its two crease edges, which
//     is the same order); forward, edge vertex: a = min end, b = max end, c, d in ascending incidence id 3 f + k;
//   backward, old vertex v: its own coefficient times g[v]; then per edge-end slot ascending the edge's weight times g[V + e],
//     then the far end's coefficient on v times g[far]; then per face-corner slot ascending 1/8 g[V + opposite edge] where
//     that edge is interior.  Terms whose coefficient is zero are left out.
// Nothing here uses a float atomic or a partial sum: one lane owns one output row, so the bits do not depend on the launch
// shape, on the batch or on the run.
#pragma clang fp contract(off)
#include "common.hpp"
#include "prims.hpp"
#include "wave.hpp"

namespace deftet {
namespace loopsub {

typedef unsigned long long u64;
typedef unsigned int u32;
constexpr int kThreads = 256;
constexpr int kMaxAttr = 8;

// ---------------------------------------------------------------------------- topology
// what the count entry leaves in the workspace for the fill entry, and the scratch of both
struct Layout {
    size_t bytes, n, sortBytes, scanBytes, csrBytes;
    u64 *k0, *k1;            // keys min V + max per incidence 3 f + k: unsorted, sorted
    u32 *v1;                 // the incidence ids in sorted order
    int *pos;                // [n + 1] exclusive scan of the run starts: pos[n] = E
    long long *edges64;      // [n, 2] the edges as the CSR builder reads them
    int *bad;                // the CSR builder's flag (indices are checked before)
    void *sortTmp, *scanTmp, *csrTmp;
};

static Layout make_layout(int V, int F, void *ws)
{
    Layout L{};
    const size_t n = (size_t)(F > 0 ? F : 0) * 3;
    L.n = n;
    Arena A(ws);
    L.k0 = A.take<u64>(n);
    L.k1 = A.take<u64>(n);
    L.v1 = A.take<u32>(n);
    L.pos = A.take<int>(n + 1);
    L.edges64 = A.take<long long>(2 * n);
    L.bad = A.take<int>(1);
    L.sortBytes = prims::radix_sort_temp_bytes<u64, u32>(n);
    L.sortTmp = A.take<char>(L.sortBytes);
    L.scanBytes = prims::scan_temp_bytes<int>(n + 1);
    L.scanTmp = A.take<char>(L.scanBytes);
    // E <= 3 F edges around V vertices, or F faces: the larger of the two CSR builds
    L.csrBytes = vtx::incidence_csr_workspace_bytes(1, V > 0 ? V : 0, (int)n, 2);
    L.csrTmp = A.take<char>(L.csrBytes);
    L.bytes = A.end();
    return L;
}

// key of incidence i = 3 f + k: the local edge (f_k, f_{k+1}) as min V + max (64 bits: V^2 passes 2^32 from V = 65,536)
__global__ __launch_bounds__(kThreads) void k_lt_keys(const long long *__restrict__ faces, long long n, int V, u64 *keys, int *counts)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long f = i / 3;
    const int k = (int)(i - 3 * f);
    const long long a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3];
    u64 key = 0ull;
    if (a < 0 || a >= V || b < 0 || b >= V) counts[1] = 1;                  // (the same value from every lane that writes)
    else if (a == b) counts[2] = 1;
    else key = (u64)(a < b ? a : b) * (u64)V + (u64)(a < b ? b : a);
    keys[i] = key;
}

__global__ __launch_bounds__(kThreads) void k_lt_flag(const u64 *__restrict__ key, long long n, int *flag)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// counts[0] = E; counts[3 + s] = the first edge whose min end is >= shape_off[s] (s = 0 .. n_shape): shapes that occupy ascending
// vertex ranges own ascending edge ranges
__global__ __launch_bounds__(kThreads) void k_lt_counts(const u64 *__restrict__ key, const int *__restrict__ pos, long long n, int V,
                                                        const int *__restrict__ shape_off, int n_shape, int *counts)
{
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s == 0) counts[0] = pos[n];
    if (s > n_shape || n_shape <= 0) return;
    const long long v0 = shape_off[s];
    const u64 want = (u64)(v0 < 0 ? 0 : v0) * (u64)V;
    long long lo = 0, hi = n;                                               // first i with key[i] >= want
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    counts[3 + s] = pos[lo];
}

// per sorted incidence: the edge id of its local edge; per run start: the edge, its incidence count, its opposite corners
__global__ __launch_bounds__(kThreads) void k_lt_edges(const long long *__restrict__ faces, const u64 *__restrict__ key,
                                                       const u32 *__restrict__ inc, const int *__restrict__ pos, long long n, int V, int E,
                                                       int *edges, long long *edges64, int *face_edge, int *edge_nface, int *edge_opp)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    const bool start = i == 0 || key[i - 1] != k;
    const int e = pos[i] + (start ? 0 : -1);                                // pos counts the run starts before i
    if (e < 0 || e >= E) return;
    const u32 me = inc[i];
    if ((long long)me < n) face_edge[me] = e;
    if (!start) return;
    long long j = i + 1;
    while (j < n && key[j] == k) ++j;
    const int cnt = (int)(j - i);
    const int a = (int)(k / (u64)V), b = (int)(k % (u64)V);
    edges[2 * e] = a;
    edges[2 * e + 1] = b;
    edges64[2 * e] = a;
    edges64[2 * e + 1] = b;
    edge_nface[e] = cnt;
    int o0 = -1, o1 = -1;
    if (cnt == 2) {                                                         // (a stable sort: the run is in ascending incidence id)
        const u32 i0 = me, i1 = inc[i + 1];
        o0 = (int)faces[(long long)(i0 / 3) * 3 + (i0 % 3 + 2) % 3];
        o1 = (int)faces[(long long)(i1 / 3) * 3 + (i1 % 3 + 2) % 3];
    }
    edge_opp[2 * e] = o0;
    edge_opp[2 * e + 1] = o1;
}

__global__ __launch_bounds__(kThreads) void k_lt_children(const long long *__restrict__ faces, const int *__restrict__ face_edge, int F, int V,
                                                          long long *child)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const long long a = faces[3 * (long long)f], b = faces[3 * (long long)f + 1], c = faces[3 * (long long)f + 2];
    const long long mab = (long long)V + face_edge[3 * (long long)f], mbc = (long long)V + face_edge[3 * (long long)f + 1],
                    mca = (long long)V + face_edge[3 * (long long)f + 2];
    long long *o = child + 12 * (long long)f;
    o[0] = a;   o[1] = mab;  o[2] = mca;
    o[3] = b;   o[4] = mbc;  o[5] = mab;
    o[6] = c;   o[7] = mca;  o[8] = mbc;
    o[9] = mab; o[10] = mbc; o[11] = mca;
}

// vertex_kind: 0 smooth (no crease edge), 1 crease (exactly two), 2 corner; crease_nbr: the far ends of the two, ascending edge id
__global__ __launch_bounds__(kThreads) void k_lt_kinds(const int *__restrict__ ev_off, const int *__restrict__ ev_slot, const int *__restrict__ edges,
                                                       const int *__restrict__ edge_nface, int V, int E, unsigned char *kind, int *crease_nbr)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    int cnt = 0, n0 = -1, n1 = -1;
    const int q1 = ev_off[v + 1];
    for (int q = ev_off[v]; q < q1; ++q) {
        const int slot = ev_slot[q], e = slot >> 1;
        if (e < 0 || e >= E || edge_nface[e] == 2) continue;
        const int far = edges[2 * e + (1 - (slot & 1))];
        if (cnt == 0) n0 = far;
        else if (cnt == 1) n1 = far;
        ++cnt;
    }
    kind[v] = cnt == 0 ? 0 : cnt == 2 ? 1 : 2;
    crease_nbr[2 * v] = cnt == 2 ? n0 : -1;
    crease_nbr[2 * v + 1] = cnt == 2 ? n1 : -1;
}

// ---------------------------------------------------------------------------- the operator
struct Topo {
    const int2 *edges;          // [E] (min, max)
    const int *edge_nface;      // [E]
    const int2 *edge_opp;       // [E]
    const unsigned char *kind;  // [V]
    const int2 *crease_nbr;     // [V]
    const int *ev_off, *ev_slot;   // vertex -> edge ends, slots 2 e + side
    const int *face_edge;       // [3 F]            (backward only)
    const int *fv_off, *fv_slot;   // vertex -> face corners, slots 3 f + k   (backward only)
    int V, E, F;
};

// the old-vertex rule of a smooth vertex of valence n: own and per-neighbour coefficient (mode 0 = subdivide, 1 = limit)
__device__ __forceinline__ void smooth_coef(int mode, int n, float &own, float &nb)
{
    if (n == 0) { own = 1.0f; nb = 0.0f; return; }
    const float fn = (float)n;
    const float beta = n == 3 ? 0.1875f : 3.0f / (8.0f * fn);
    nb = mode == 0 ? beta : 1.0f / (fn + 3.0f / (8.0f * beta));
    own = 1.0f - fn * nb;
}
__device__ __forceinline__ float crease_own(int mode) { return mode == 0 ? 0.75f : 2.0f / 3.0f; }
__device__ __forceinline__ float crease_nb(int mode) { return mode == 0 ? 0.125f : 1.0f / 6.0f; }

// one accumulator row: 3 position components and up to 8 attribute components
template <bool ATTR>
struct Row {
    float p[3], a[ATTR ? kMaxAttr : 1];
    __device__ __forceinline__ void set(float w, const float *x, const float *y, size_t r, int C)
    {
        if (x)
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = w * x[r * 3 + k];
        if (ATTR && y)
#pragma unroll
            for (int k = 0; k < kMaxAttr; ++k)
                if (k < C) a[k] = w * y[r * C + k];
    }
    __device__ __forceinline__ void add(float w, const float *x, const float *y, size_t r, int C)
    {
        if (x)
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = p[k] + w * x[r * 3 + k];
        if (ATTR && y)
#pragma unroll
            for (int k = 0; k < kMaxAttr; ++k)
                if (k < C) a[k] = a[k] + w * y[r * C + k];
    }
    __device__ __forceinline__ void store(float *x, float *y, size_t r, int C) const
    {
        if (x)
#pragma unroll
            for (int k = 0; k < 3; ++k) x[r * 3 + k] = p[k];
        if (ATTR && y)
#pragma unroll
            for (int k = 0; k < kMaxAttr; ++k)
                if (k < C) y[r * C + k] = a[k];
    }
};

// forward: one lane per output row (old vertices 0 .. V-1, then the edge vertices of mode 0), blockIdx.y = shape
template <bool ATTR>
__global__ __launch_bounds__(kThreads) void k_loop_fwd(Topo t, const float *__restrict__ verts, const float *__restrict__ attr, int C, int mode,
                                                       float *out_verts, float *out_attr)
{
    const int r = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    const int rows = mode == 0 ? t.V + t.E : t.V;
    if (r >= rows) return;
    const size_t in0 = (size_t)b * t.V, out0 = (size_t)b * rows;
    Row<ATTR> acc;
    if (r < t.V) {
        const int kind = t.kind[r];
        if (kind == 0) {
            const int q0 = t.ev_off[r], q1 = t.ev_off[r + 1];
            float own, nb;
            smooth_coef(mode, q1 - q0, own, nb);
            acc.set(own, verts, attr, in0 + r, C);
            for (int q = q0; q < q1; ++q) {
                const int slot = t.ev_slot[q], e = slot >> 1;
                if (e < 0 || e >= t.E) continue;
                const int2 ed = t.edges[e];
                const int far = (slot & 1) ? ed.x : ed.y;
                if (far < 0 || far >= t.V) continue;
                acc.add(nb, verts, attr, in0 + far, C);
            }
        } else if (kind == 1) {
            const int2 nbr = t.crease_nbr[r];
            acc.set(crease_own(mode), verts, attr, in0 + r, C);
            if (nbr.x >= 0 && nbr.x < t.V) acc.add(crease_nb(mode), verts, attr, in0 + nbr.x, C);
            if (nbr.y >= 0 && nbr.y < t.V) acc.add(crease_nb(mode), verts, attr, in0 + nbr.y, C);
        } else {
            acc.set(1.0f, verts, attr, in0 + r, C);
        }
    } else {
        const int e = r - t.V;
        const int2 ed = t.edges[e];
        const int2 op = t.edge_opp[e];
        const bool inner = t.edge_nface[e] == 2 && op.x >= 0 && op.x < t.V && op.y >= 0 && op.y < t.V;
        const int a = min(max(ed.x, 0), t.V - 1), c = min(max(ed.y, 0), t.V - 1);
        const float w = inner ? 0.375f : 0.5f;
        acc.set(w, verts, attr, in0 + a, C);
        acc.add(w, verts, attr, in0 + c, C);
        if (inner) {
            acc.add(0.125f, verts, attr, in0 + op.x, C);
            acc.add(0.125f, verts, attr, in0 + op.y, C);
        }
    }
    acc.store(out_verts, out_attr, out0 + r, C);
}

// backward (the transpose): one lane per old vertex walks both CSRs in the order of the file's header
template <bool ATTR>
__global__ __launch_bounds__(kThreads) void k_loop_bwd(Topo t, const float *__restrict__ g_verts, const float *__restrict__ g_attr, int C, int mode,
                                                       float *grad_verts, float *grad_attr)
{
    const int v = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (v >= t.V) return;
    const int rows = mode == 0 ? t.V + t.E : t.V;
    const size_t g0 = (size_t)b * rows;
    const int kind = t.kind[v];
    const int q0 = t.ev_off[v], q1 = t.ev_off[v + 1];
    float own, nb;
    if (kind == 0) smooth_coef(mode, q1 - q0, own, nb);
    else own = kind == 1 ? crease_own(mode) : 1.0f;
    Row<ATTR> acc;
    acc.set(own, g_verts, g_attr, g0 + v, C);
    for (int q = q0; q < q1; ++q) {
        const int slot = t.ev_slot[q], e = slot >> 1;
        if (e < 0 || e >= t.E) continue;
        const bool crease = t.edge_nface[e] != 2;
        if (mode == 0) acc.add(crease ? 0.5f : 0.375f, g_verts, g_attr, g0 + t.V + e, C);
        const int2 ed = t.edges[e];
        const int u = (slot & 1) ? ed.x : ed.y;
        if (u < 0 || u >= t.V) continue;
        const int ku = t.kind[u];
        if (ku == 0) {
            float uo, un;
            smooth_coef(mode, t.ev_off[u + 1] - t.ev_off[u], uo, un);
            acc.add(un, g_verts, g_attr, g0 + u, C);
        } else if (ku == 1 && crease) {
            acc.add(crease_nb(mode), g_verts, g_attr, g0 + u, C);
        }
    }
    if (mode == 0) {
        const int p1 = t.fv_off[v + 1];
        for (int p = t.fv_off[v]; p < p1; ++p) {
            const int slot = t.fv_slot[p];
            if (slot < 0 || slot >= 3 * t.F) continue;
            const int f = slot / 3, k = slot - 3 * f;
            const int e = t.face_edge[3 * f + (k + 1) % 3];
            if (e < 0 || e >= t.E || t.edge_nface[e] != 2) continue;
            acc.add(0.125f, g_verts, g_attr, g0 + t.V + e, C);
        }
    }
    acc.store(grad_verts, grad_attr, (size_t)b * t.V + v, C);
}

static int check_sizes(int V, int F)
{
    DEFTET_CHECK_ARG(F > 0 && V > 0, "n_face=%d, n_vertex=%d must be positive", F, V);
    DEFTET_CHECK_ARG(4LL * F < 2147483648LL, "4 n_face = %lld does not fit 31 bits", 4LL * F);
    return DEFTET_OK;
}

static int check_op(int B, int V, int E, int C, int mode)
{
    DEFTET_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && E > 0, "n_batch=%d (1..65535), n_vertex=%d, n_edge=%d must be positive", B, V, E);
    DEFTET_CHECK_ARG(mode == 0 || mode == 1, "mode=%d is neither 0 (subdivide) nor 1 (limit)", mode);
    DEFTET_CHECK_ARG(C >= 0 && C <= kMaxAttr, "n_attr=%d outside 0..8", C);
    DEFTET_CHECK_ARG((long long)V + E < 2147483648LL && (long long)B * ((long long)V + E) < 2147483648LL,
                     "n_vertex + n_edge or n_batch * (n_vertex + n_edge) does not fit 31 bits");
    return DEFTET_OK;
}

}  // namespace loopsub
}  // namespace deftet

using namespace deftet;
using namespace deftet::loopsub;

extern "C" size_t deftet_loop_topology_workspace_bytes(int V, int F)
{
    return V <= 0 || F <= 0 || 4LL * F >= 2147483648LL ? 256 : make_layout(V, F, nullptr).bytes;
}

extern "C" int deftet_loop_topology_count_i64(const int64_t *faces_fx3, int F, int V, const int32_t *shape_offsets, int n_shape,
                                              int32_t *counts, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_sizes(V, F));
    DEFTET_CHECK_ARG(n_shape >= 0 && (n_shape == 0) == (shape_offsets == nullptr), "n_shape=%d and shape_offsets do not go together", n_shape);
    DEFTET_CHECK_ARG(faces_fx3 && counts, "null pointer: faces / counts");
    const Layout L = make_layout(V, F, workspace);
    DEFTET_TRY(workspace_ok("deftet_loop_topology*", workspace, wsb, L.bytes));
    hipStream_t st = as_stream(stream_);
    const long long n = (long long)L.n;
    int bits = 1;
    while (bits < 64 && ((u64)V * (u64)V) >> bits) ++bits;
    DEFTET_HIP(hipMemsetAsync(counts, 0, (size_t)(3 + (n_shape ? n_shape + 1 : 0)) * 4, st));
    DEFTET_LAUNCH(k_lt_keys, dim3(blocks_for(n, kThreads)), dim3(kThreads), st, (const long long *)faces_fx3, n, V, L.k0, (int *)counts);
    DEFTET_TRY((prims::radix_sort_from<u64, u32>(prims::PtrLoad<u64>{L.k0}, L.k1, prims::IotaLoad{}, L.v1, (size_t)n, bits, L.sortTmp, L.sortBytes, st)));
    DEFTET_LAUNCH(k_lt_flag, dim3(blocks_for(n + 1, kThreads)), dim3(kThreads), st, (const u64 *)L.k1, n, L.pos);
    DEFTET_TRY((prims::scan<int, prims::Plus, true>(L.pos, L.pos, (size_t)n + 1, 0, prims::Plus(), L.scanTmp, L.scanBytes, st)));
    DEFTET_LAUNCH(k_lt_counts, dim3(blocks_for((size_t)n_shape + 1, kThreads)), dim3(kThreads), st, (const u64 *)L.k1, (const int *)L.pos, n, V,
                  (const int *)shape_offsets, n_shape, (int *)counts);
    return DEFTET_OK;
}

extern "C" int deftet_loop_topology_fill_i64(const int64_t *faces_fx3, int F, int V, int E, int32_t *edges_ex2, int32_t *face_edge_fx3,
                                             int32_t *edge_nface, int32_t *edge_opp_ex2, uint8_t *vertex_kind, int32_t *crease_nbr_vx2,
                                             int32_t *ev_offsets, int32_t *ev_slots, int32_t *fv_offsets, int32_t *fv_slots,
                                             int64_t *child_faces, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_TRY(check_sizes(V, F));
    DEFTET_CHECK_ARG(E > 0 && E <= 3LL * F, "n_edge=%d outside 1..3 n_face", E);
    DEFTET_CHECK_ARG((long long)V + E < 2147483648LL, "n_vertex + n_edge does not fit 31 bits");
    DEFTET_CHECK_ARG(faces_fx3 && edges_ex2 && face_edge_fx3 && edge_nface && edge_opp_ex2 && vertex_kind && crease_nbr_vx2 && ev_offsets &&
                         ev_slots && fv_offsets && fv_slots && child_faces, "null pointer");
    const Layout L = make_layout(V, F, workspace);
    DEFTET_TRY(workspace_ok("deftet_loop_topology*", workspace, wsb, L.bytes));
    hipStream_t st = as_stream(stream_);
    const long long n = (long long)L.n;
    DEFTET_LAUNCH(k_lt_edges, dim3(blocks_for(n, kThreads)), dim3(kThreads), st, (const long long *)faces_fx3, (const u64 *)L.k1, (const u32 *)L.v1,
                  (const int *)L.pos, n, V, E, (int *)edges_ex2, L.edges64, (int *)face_edge_fx3, (int *)edge_nface, (int *)edge_opp_ex2);
    DEFTET_LAUNCH(k_lt_children, dim3(blocks_for(F, kThreads)), dim3(kThreads), st, (const long long *)faces_fx3, (const int *)face_edge_fx3, F, V,
                  (long long *)child_faces);
    // the two incidence CSRs: deftet_edge_vertex_csr_i32's (slots 2 e + side) and deftet_face_vertex_csr_i32's (slots 3 f + corner)
    DEFTET_TRY(vtx::incidence_csr((const int64_t *)L.edges64, ev_offsets, ev_slots, L.bad, 1, V, E, 2, L.csrTmp, L.csrBytes, st));
    DEFTET_TRY(vtx::incidence_csr(faces_fx3, fv_offsets, fv_slots, L.bad, 1, V, F, 3, L.csrTmp, L.csrBytes, st));
    DEFTET_LAUNCH(k_lt_kinds, dim3(blocks_for(V, kThreads)), dim3(kThreads), st, (const int *)ev_offsets, (const int *)ev_slots, (const int *)edges_ex2,
                  (const int *)edge_nface, V, E, (unsigned char *)vertex_kind, (int *)crease_nbr_vx2);
    return DEFTET_OK;
}

static int make_topo(Topo &t, const int32_t *edges, const int32_t *edge_nface, const int32_t *edge_opp, const uint8_t *kind,
                     const int32_t *crease_nbr, const int32_t *ev_off, const int32_t *ev_slot, int V, int E)
{
    DEFTET_CHECK_ARG(edges && edge_nface && edge_opp && kind && crease_nbr && ev_off && ev_slot, "null pointer: a topology table");
    DEFTET_CHECK_ARG(aligned(edges, 8) && aligned(edge_opp, 8) && aligned(crease_nbr, 8), "edges_ex2 / edge_opp_ex2 / crease_nbr_vx2 must be 8-byte aligned");
    t = Topo{(const int2 *)edges, edge_nface, (const int2 *)edge_opp, kind, (const int2 *)crease_nbr, ev_off, ev_slot, nullptr, nullptr, nullptr, V, E, 0};
    return DEFTET_OK;
}

extern "C" int deftet_loop_subdivide_fwd_f32(const float *verts_bxvx3, const float *attr_bxvxc, int C, const int32_t *edges_ex2,
                                             const int32_t *edge_nface, const int32_t *edge_opp_ex2, const uint8_t *vertex_kind,
                                             const int32_t *crease_nbr_vx2, const int32_t *ev_offsets, const int32_t *ev_slots, int B, int V,
                                             int E, int mode, float *out_verts, float *out_attr, void *stream_)
{
    DEFTET_TRY(check_op(B, V, E, C, mode));
    DEFTET_CHECK_ARG((attr_bxvxc == nullptr) == (C == 0) && (attr_bxvxc == nullptr) == (out_attr == nullptr),
                     "attr_bxvxc, n_attr=%d and out_attr do not go together", C);
    DEFTET_CHECK_ARG(verts_bxvx3 && out_verts, "null pointer: verts / out_verts");
    Topo t;
    DEFTET_TRY(make_topo(t, edges_ex2, edge_nface, edge_opp_ex2, vertex_kind, crease_nbr_vx2, ev_offsets, ev_slots, V, E));
    const int rows = mode == 0 ? V + E : V;
    const dim3 grid(blocks_for(rows, kThreads), B);
    hipStream_t st = as_stream(stream_);
    if (C == 0) DEFTET_LAUNCH(k_loop_fwd<false>, grid, dim3(kThreads), st, t, verts_bxvx3, attr_bxvxc, C, mode, out_verts, out_attr);
    else DEFTET_LAUNCH(k_loop_fwd<true>, grid, dim3(kThreads), st, t, verts_bxvx3, attr_bxvxc, C, mode, out_verts, out_attr);
    return DEFTET_OK;
}

extern "C" int deftet_loop_subdivide_bwd_f32(const float *grad_out_verts, const float *grad_out_attr, int C, const int32_t *edges_ex2,
                                             const int32_t *edge_nface, const int32_t *edge_opp_ex2, const uint8_t *vertex_kind,
                                             const int32_t *crease_nbr_vx2, const int32_t *ev_offsets, const int32_t *ev_slots,
                                             const int32_t *face_edge_fx3, const int32_t *fv_offsets, const int32_t *fv_slots, int B, int V,
                                             int E, int F, int mode, float *grad_verts, float *grad_attr, void *stream_)
{
    DEFTET_TRY(check_op(B, V, E, C, mode));
    DEFTET_CHECK_ARG(F > 0 && 3LL * F < 2147483648LL, "n_face=%d must be positive and 3 n_face fit 31 bits", F);
    DEFTET_CHECK_ARG((grad_out_verts == nullptr) == (grad_verts == nullptr) && (grad_out_attr == nullptr) == (grad_attr == nullptr),
                     "every gradient read goes with the gradient written from it");
    DEFTET_CHECK_ARG(grad_verts || grad_attr, "null pointer: every output");
    DEFTET_CHECK_ARG(!grad_attr || C > 0, "grad_attr without attributes");
    Topo t;
    DEFTET_TRY(make_topo(t, edges_ex2, edge_nface, edge_opp_ex2, vertex_kind, crease_nbr_vx2, ev_offsets, ev_slots, V, E));
    DEFTET_CHECK_ARG(face_edge_fx3 && fv_offsets && fv_slots, "null pointer: a topology table");
    t.face_edge = face_edge_fx3;
    t.fv_off = fv_offsets;
    t.fv_slot = fv_slots;
    t.F = F;
    const dim3 grid(blocks_for(V, kThreads), B);
    hipStream_t st = as_stream(stream_);
    if (!grad_attr) DEFTET_LAUNCH(k_loop_bwd<false>, grid, dim3(kThreads), st, t, grad_out_verts, grad_out_attr, C, mode, grad_verts, grad_attr);
    else DEFTET_LAUNCH(k_loop_bwd<true>, grid, dim3(kThreads), st, t, grad_out_verts, grad_out_attr, C, mode, grad_verts, grad_attr);
    return DEFTET_OK;
}
