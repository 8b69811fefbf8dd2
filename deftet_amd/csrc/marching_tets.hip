// marching_tets.hip — marching tetrahedra on a per-vertex field: a welded iso-surface mesh of every shape of a batch, and the
// gradient of its vertices with respect to the tet vertices, their attributes and the field (gfx950).
//
// A corner is inside iff field > iso (fp32, strict; NaN is outside).  An edge of the unique (min,max) edge list crosses iff its two
// ends differ; every crossing edge of every shape gets ONE output vertex, computed in the edge's canonical order
//     t = (iso - f_min) / (f_max - f_min),   p = p_min + t * (p_max - p_min)          (no fused multiply-add: -ffp-contract=off)
// so both tets on an edge index the same vertex and the mesh is welded by construction.  A tet's case code is
// sum(inside_k << k); kTri holds, per code, the crossing local edges (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) = 0..5 in cyclic order
// from the lowest id, directed so that on a positively oriented tet the normal points from the inside corners to the outside
// ones; a quad q0..q3 is the triangles (q0,q1,q2), (q0,q2,q3).  A negatively oriented tet comes out with flipped winding.
//
// Count: ONE launch writes the crossing flag of every (b,e) and the triangle count of every (b,t) into one int32 array, one
// exclusive scan (prims.hpp) turns it into output rows, one launch writes edge_vertex [B,E] (the vertex of an edge inside its
// shape, -1 where it does not cross) and the [2,B+1] offsets the caller reads back.  Fill: ONE launch over the same index range
// writes the vertex rows (crossing edges) and the face rows (mixed tets: 24 bytes of tet_edge through edge_vertex).
// Backward: one thread per (b,v) walks the vertex's row of the edge-end CSR in slot order and skips the edges whose
// edge_vertex entry is -1: no atomics, a fixed order of summation.
#include "common.hpp"
#include "prims.hpp"

namespace deftet {
namespace mt {

constexpr int kThreads = 256;

// n | q0 << 2 | q1 << 5 | q2 << 8 | q3 << 11 with n = triangles of the code
__device__ const unsigned short kTri[16] = {0x0000, 0x0221, 0x0381, 0x1c46, 0x0565, 0x1562, 0x0d82, 0x0589,
                                            0x04a9, 0x2522, 0x1d42, 0x03a5, 0x1466, 0x0461, 0x0141, 0x0000};
// the same counts, two bits per code, for the count pass (a literal: no load)
constexpr unsigned kTriCount = 0x16696994u;        // codes 0..15: 0 1 1 2 1 2 2 1 1 2 2 1 2 1 1 0

struct Shape {
    const float *field;       // [B,V]
    const int2 *edges;        // [E] (min, max)
    const int4 *tets;         // [T]
    int B, V, T, E;
    float iso;
};

__device__ __forceinline__ bool inside(float f, float iso) { return f > iso; }

__device__ __forceinline__ unsigned case_code(const Shape &s, int b, int t)
{
    const float *f = s.field + (size_t)b * s.V;
    const int4 q = s.tets[t];
    return (inside(f[q.x], s.iso) ? 1u : 0u) | (inside(f[q.y], s.iso) ? 2u : 0u) | (inside(f[q.z], s.iso) ? 4u : 0u) |
           (inside(f[q.w], s.iso) ? 8u : 0u);
}

// cnt[i], i < B*E: 1 iff edge i % E of shape i / E crosses; cnt[B*E + j], j < B*T: triangles of tet j % T of shape j / T;
// cnt[B*E + B*T] = 0 (the scan's last element: its exclusive value is the total)
__global__ __launch_bounds__(kThreads) void k_mt_count(Shape s, int *cnt)
{
    const long long nE = (long long)s.B * s.E, n = nE + (long long)s.B * s.T;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    int c = 0;
    if (i < nE) {
        const int b = (int)(i / s.E), e = (int)(i - (long long)b * s.E);
        const float *f = s.field + (size_t)b * s.V;
        const int2 ed = s.edges[e];
        c = inside(f[ed.x], s.iso) != inside(f[ed.y], s.iso) ? 1 : 0;
    } else if (i < n) {
        const long long j = i - nE;
        const int b = (int)(j / s.T), t = (int)(j - (long long)b * s.T);
        c = (int)((kTriCount >> (2u * case_code(s, b, t))) & 3u);
    }
    cnt[i] = c;
}

// pos = the scanned cnt.  edge_vertex[b,e] = the edge's vertex inside shape b, or -1; offsets[0][b] = first vertex row of shape b,
// offsets[1][b] = first face row, [.][B] = the totals
__global__ __launch_bounds__(kThreads) void k_mt_finish(const int *__restrict__ pos, int B, int T, int E, int *edge_vertex, int *offsets)
{
    const long long nE = (long long)B * E;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i <= B) {
        offsets[i] = pos[i * E];
        offsets[B + 1 + i] = pos[nE + i * T] - pos[nE];
    }
    if (i >= nE) return;
    const int b = (int)(i / E);
    const int p = pos[i];
    edge_vertex[i] = pos[i + 1] != p ? p - pos[(long long)b * E] : -1;
}

struct Out {
    const float *pos;         // [B,V,3]
    const float *attr;        // [B,V,C] or null
    const int *tet_edge;      // [T,6]
    const int *edge_vertex;   // [B,E]
    float *verts;             // [Nv,3]
    float *vert_attr;         // [Nv,C] or null
    long long *faces;         // [Nf,3]
    long long *edge_id;       // [Nv] or null
    float *t;                 // [Nv] or null
    long long *tet_id;        // [Nf] or null
    long long cap_v, cap_f;   // rows the outputs hold
    int C;
};

__global__ __launch_bounds__(kThreads) void k_mt_fill(Shape s, Out o, const int *__restrict__ pos)
{
    const long long nE = (long long)s.B * s.E, n = nE + (long long)s.B * s.T;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int row = pos[i], rows = pos[i + 1] - row;
    if (rows <= 0 || row < 0) return;
    if (i < nE) {
        if (rows != 1 || (long long)row >= o.cap_v) return;            // (a foreign workspace writes nothing out of bounds)
        const int b = (int)(i / s.E), e = (int)(i - (long long)b * s.E);
        const int2 ed = s.edges[e];
        const float *f = s.field + (size_t)b * s.V;
        const float f0 = f[ed.x], f1 = f[ed.y];
        const float t = (s.iso - f0) / (f1 - f0);
        const float *p0 = o.pos + ((size_t)b * s.V + ed.x) * 3, *p1 = o.pos + ((size_t)b * s.V + ed.y) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) o.verts[(size_t)row * 3 + k] = p0[k] + t * (p1[k] - p0[k]);
        if (o.vert_attr) {
            const float *a0 = o.attr + ((size_t)b * s.V + ed.x) * o.C, *a1 = o.attr + ((size_t)b * s.V + ed.y) * o.C;
            for (int k = 0; k < o.C; ++k) o.vert_attr[(size_t)row * o.C + k] = a0[k] + t * (a1[k] - a0[k]);
        }
        if (o.edge_id) o.edge_id[row] = e;
        if (o.t) o.t[row] = t;
    } else {
        const long long j = i - nE;
        const int b = (int)(j / s.T), tt = (int)(j - (long long)b * s.T);
        const unsigned w = kTri[case_code(s, b, tt)];
        if ((int)(w & 3u) != rows) return;                             // (the field changed since the count pass: nothing is written)
        const long long base = (long long)row - pos[nE];
        if (base < 0 || base + rows > o.cap_f) return;
        const int *te = o.tet_edge + (size_t)tt * 6;
        const int *ev = o.edge_vertex + (size_t)b * s.E;
        const long long q0 = ev[te[(w >> 2) & 7u]], q1 = ev[te[(w >> 5) & 7u]], q2 = ev[te[(w >> 8) & 7u]];
        long long *fa = o.faces + base * 3;
        fa[0] = q0, fa[1] = q1, fa[2] = q2;
        if (o.tet_id) o.tet_id[base] = tt;
        if (rows == 2) {
            fa[3] = q0, fa[4] = q2, fa[5] = ev[te[(w >> 11) & 7u]];
            if (o.tet_id) o.tet_id[base + 1] = tt;
        }
    }
}

// One thread per (b,v).  Everything in double: the sums are compared with a float64 reference, and a vertex has about 14 edges.
template <int CMAX>
__global__ __launch_bounds__(kThreads) void k_mt_bwd(Shape s, const float *__restrict__ pos, const float *__restrict__ attr, int C,
                                                     const int *__restrict__ csr_off, const int *__restrict__ csr_slot,
                                                     const int *__restrict__ edge_vertex, const int *__restrict__ offsets,
                                                     const float *__restrict__ g_verts, const float *__restrict__ g_attr, long long n_rows,
                                                     float *grad_pos, float *grad_field, float *grad_attr)
{
    const int v = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (v >= s.V) return;
    const size_t bv = (size_t)b * s.V;
    const float *f = s.field + bv;
    const int *ev = edge_vertex + (size_t)b * s.E;
    const long long row0 = offsets[b];
    const double iso = (double)s.iso;
    double gp[3] = {0.0, 0.0, 0.0}, gf = 0.0, ga[CMAX > 0 ? CMAX : 1];
#pragma unroll
    for (int k = 0; k < CMAX; ++k) ga[k] = 0.0;
    const int s1 = csr_off[v + 1];
    for (int q = csr_off[v]; q < s1; ++q) {
        const int slot = csr_slot[q], e = slot >> 1, side = slot & 1;
        if (e < 0 || e >= s.E) continue;
        const int r = ev[e];
        if (r < 0) continue;
        const long long row = row0 + r;
        if (row >= n_rows) continue;
        const int2 ed = s.edges[e];
        const double f0 = (double)f[ed.x], f1 = (double)f[ed.y], d = f1 - f0;
        const double t = (iso - f0) / d;
        const double wgt = side ? t : 1.0 - t;
        const double dtdf = side ? -(iso - f0) / (d * d) : (iso - f1) / (d * d);
        double dot = 0.0;
        if (g_verts) {
            const float *p0 = pos + (bv + ed.x) * 3, *p1 = pos + (bv + ed.y) * 3, *g = g_verts + (size_t)row * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double gk = (double)g[k];
                gp[k] += wgt * gk;
                dot += gk * ((double)p1[k] - (double)p0[k]);
            }
        }
        if (CMAX > 0 && g_attr) {
            const float *a0 = attr + (bv + ed.x) * C, *a1 = attr + (bv + ed.y) * C, *g = g_attr + (size_t)row * C;
#pragma unroll
            for (int k = 0; k < CMAX; ++k)
                if (k < C) {
                    const double gk = (double)g[k];
                    ga[k] += wgt * gk;
                    dot += gk * ((double)a1[k] - (double)a0[k]);
                }
        }
        gf += dtdf * dot;
    }
    if (grad_pos)
#pragma unroll
        for (int k = 0; k < 3; ++k) grad_pos[(bv + v) * 3 + k] = (float)gp[k];
    if (grad_field) grad_field[bv + v] = (float)gf;
    if (CMAX > 0 && grad_attr)
#pragma unroll
        for (int k = 0; k < CMAX; ++k)
            if (k < C) grad_attr[(bv + v) * C + k] = (float)ga[k];
}

static inline size_t n_count(int B, int T, int E) { return (size_t)B * E + (size_t)B * T + 1; }

// the counts of every (shape, edge) and (shape, tet), scanned in place: the count entry writes them, the fill entry reads them
struct Layout {
    size_t bytes, n, scanTmpBytes;
    int *cnt;
    void *scanTmp;
};

static Layout make_layout(int B, int T, int E, void *ws)
{
    Layout L{};
    L.n = n_count(B, T, E);
    Arena A(ws);
    L.cnt = A.take<int>(L.n);
    L.scanTmpBytes = prims::scan_temp_bytes<int>(L.n);
    L.scanTmp = A.take<char>(L.scanTmpBytes);
    L.bytes = A.end();
    return L;
}

static int check_shape(int B, int V, int T, int E, float iso, void *workspace, size_t wsb, Layout &L)
{
    DEFTET_CHECK_ARG(B > 0 && T > 0 && E > 0 && V > 0, "n_batch=%d, n_vertex=%d, n_tet=%d, n_edge=%d must be positive", B, V, T, E);
    DEFTET_CHECK_ARG(iso == iso && iso - iso == 0.0f, "iso is not finite");
    DEFTET_CHECK_ARG((long long)B * E < 2147483648LL && (long long)B * T < 2147483648LL, "n_batch * n_edge or n_batch * n_tet does not fit 31 bits");
    DEFTET_CHECK_ARG((long long)B * E + 2LL * B * T < 2147483647LL && (long long)B * V < 2147483648LL,
                     "n_batch * (n_edge + 2 n_tet) or n_batch * n_vertex does not fit 31 bits");
    L = make_layout(B, T, E, workspace);
    DEFTET_TRY(workspace_ok("deftet_marching_tets*", workspace, wsb, L.bytes));
    return DEFTET_OK;
}

}  // namespace mt
}  // namespace deftet

using namespace deftet;
using namespace deftet::mt;

extern "C" size_t deftet_edge_vertex_csr_workspace_bytes(int V, int E) { return vtx::incidence_csr_workspace_bytes(1, V, E, 2); }

extern "C" int deftet_edge_vertex_csr_i32(const int64_t *edges_ex2, int32_t *offsets, int32_t *slots, int32_t *bad_flag, int V, int E,
                                          void *workspace, size_t wsb, void *stream_)
{
    DEFTET_CHECK_ARG(V > 0 && E > 0, "n_vertex=%d, n_edge=%d must be positive", V, E);
    DEFTET_CHECK_ARG(edges_ex2 && offsets && slots && bad_flag, "null pointer");
    // the (vertex, 2*e+side) incidences sorted by vertex: the stable sort keeps the slots of a vertex ascending
    return vtx::incidence_csr(edges_ex2, offsets, slots, bad_flag, 1, V, E, 2, workspace, wsb, as_stream(stream_));
}

extern "C" size_t deftet_marching_tets_workspace_bytes(int B, int T, int E)
{
    return B <= 0 || T <= 0 || E <= 0 ? 256 : make_layout(B, T, E, nullptr).bytes;
}

extern "C" int deftet_marching_tets_count_f32(const float *field_bxv, const int32_t *edges_ex2, const int32_t *tet_idx_tx4, int B, int V,
                                              int T, int E, float iso, int32_t *edge_vertex_bxe, int32_t *offsets_2xb1, void *workspace,
                                              size_t wsb, void *stream_)
{
    Layout L;
    DEFTET_TRY(check_shape(B, V, T, E, iso, workspace, wsb, L));
    DEFTET_CHECK_ARG(field_bxv && edges_ex2 && tet_idx_tx4 && edge_vertex_bxe && offsets_2xb1, "null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)edges_ex2 & 7) == 0 && ((uintptr_t)tet_idx_tx4 & 15) == 0, "misaligned edges_ex2 / tet_idx_tx4");
    hipStream_t st = as_stream(stream_);
    const size_t n = L.n;
    const Shape s{field_bxv, (const int2 *)edges_ex2, (const int4 *)tet_idx_tx4, B, V, T, E, iso};
    DEFTET_LAUNCH(k_mt_count, dim3(blocks_for(n, kThreads)), dim3(kThreads), st, s, L.cnt);
    DEFTET_TRY(prims::scan<int, prims::Plus, true>(L.cnt, L.cnt, n, 0, prims::Plus(), L.scanTmp, L.scanTmpBytes, st));
    const size_t nf = (size_t)B * E > (size_t)B + 1 ? (size_t)B * E : (size_t)B + 1;
    DEFTET_LAUNCH(k_mt_finish, dim3(blocks_for(nf, kThreads)), dim3(kThreads), st, (const int *)L.cnt, B, T, E, edge_vertex_bxe,
                  offsets_2xb1);
    return DEFTET_OK;
}

extern "C" int deftet_marching_tets_fill_f32(const float *pos_bxvx3, const float *field_bxv, const float *attr_bxvxc, int C,
                                             const int32_t *edges_ex2, const int32_t *tet_idx_tx4, const int32_t *tet_edge_tx6,
                                             const int32_t *edge_vertex_bxe, int B, int V, int T, int E, float iso, long long n_vert,
                                             long long n_face, float *verts, float *vert_attr, int64_t *faces, int64_t *edge_id, float *t,
                                             int64_t *tet_id, void *workspace, size_t wsb, void *stream_)
{
    Layout L;
    DEFTET_TRY(check_shape(B, V, T, E, iso, workspace, wsb, L));
    DEFTET_CHECK_ARG(C >= 0 && C <= 8 && (attr_bxvxc == nullptr) == (C == 0), "n_attr=%d outside 0..8, or attr_bxvxc does not go with it", C);
    DEFTET_CHECK_ARG(n_vert >= 0 && n_face >= 0, "negative capacity");
    DEFTET_CHECK_ARG(pos_bxvx3 && field_bxv && edges_ex2 && tet_idx_tx4 && tet_edge_tx6 && edge_vertex_bxe, "null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)edges_ex2 & 7) == 0 && ((uintptr_t)tet_idx_tx4 & 15) == 0, "misaligned edges_ex2 / tet_idx_tx4");
    if (n_vert == 0 && n_face == 0) return DEFTET_OK;                  // (no row: the outputs may be empty, hence null)
    DEFTET_CHECK_ARG(verts && faces && (attr_bxvxc == nullptr) == (vert_attr == nullptr), "null output, or attr_bxvxc and vert_attr do not go together");
    hipStream_t st = as_stream(stream_);
    const size_t n = L.n;
    const Shape s{field_bxv, (const int2 *)edges_ex2, (const int4 *)tet_idx_tx4, B, V, T, E, iso};
    const Out o{pos_bxvx3, attr_bxvxc, tet_edge_tx6, edge_vertex_bxe, verts, vert_attr, (long long *)faces, (long long *)edge_id, t,
                (long long *)tet_id, n_vert, n_face, C};
    DEFTET_LAUNCH(k_mt_fill, dim3(blocks_for(n - 1, kThreads)), dim3(kThreads), st, s, o, (const int *)L.cnt);
    return DEFTET_OK;
}

extern "C" int deftet_marching_tets_bwd_f32(const float *grad_verts, const float *grad_vert_attr, long long n_vert, const float *pos_bxvx3,
                                            const float *field_bxv, const float *attr_bxvxc, int C, const int32_t *edges_ex2,
                                            const int32_t *csr_offsets, const int32_t *csr_slots, const int32_t *edge_vertex_bxe,
                                            const int32_t *offsets_2xb1, int B, int V, int E, float iso, float *grad_pos, float *grad_field,
                                            float *grad_attr, void *stream_)
{
    DEFTET_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && E > 0, "n_batch=%d (1..65535), n_vertex=%d, n_edge=%d must be positive", B, V, E);
    DEFTET_CHECK_ARG((long long)B * E < 2147483648LL && (long long)B * V < 2147483648LL, "n_batch * n_edge or n_batch * n_vertex does not fit 31 bits");
    DEFTET_CHECK_ARG(iso == iso && iso - iso == 0.0f, "iso is not finite");
    DEFTET_CHECK_ARG(C >= 0 && C <= 8 && (attr_bxvxc == nullptr) == (C == 0), "n_attr=%d outside 0..8, or attr_bxvxc does not go with it", C);
    DEFTET_CHECK_ARG(n_vert >= 0 && (n_vert == 0 || grad_verts || grad_vert_attr), "negative n_vert, or no gradient to read");
    DEFTET_CHECK_ARG(!grad_vert_attr || C > 0, "grad_vert_attr without attributes");
    DEFTET_CHECK_ARG(pos_bxvx3 && field_bxv && edges_ex2 && csr_offsets && csr_slots && edge_vertex_bxe && offsets_2xb1, "null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)edges_ex2 & 7) == 0, "misaligned edges_ex2");
    DEFTET_CHECK_ARG(grad_pos || grad_field || grad_attr, "null pointer: every output");
    DEFTET_CHECK_ARG(!grad_attr || C > 0, "grad_attr without attributes");
    hipStream_t st = as_stream(stream_);
    const Shape s{field_bxv, (const int2 *)edges_ex2, nullptr, B, V, 0, E, iso};
    const dim3 grid(blocks_for(V, kThreads), B);
    if (C == 0)
        DEFTET_LAUNCH(k_mt_bwd<0>, grid, dim3(kThreads), st, s, pos_bxvx3, attr_bxvxc, C, csr_offsets, csr_slots, edge_vertex_bxe, offsets_2xb1,
                      grad_verts, grad_vert_attr, n_vert, grad_pos, grad_field, grad_attr);
    else if (C <= 4)
        DEFTET_LAUNCH(k_mt_bwd<4>, grid, dim3(kThreads), st, s, pos_bxvx3, attr_bxvxc, C, csr_offsets, csr_slots, edge_vertex_bxe, offsets_2xb1,
                      grad_verts, grad_vert_attr, n_vert, grad_pos, grad_field, grad_attr);
    else
        DEFTET_LAUNCH(k_mt_bwd<8>, grid, dim3(kThreads), st, s, pos_bxvx3, attr_bxvxc, C, csr_offsets, csr_slots, edge_vertex_bxe, offsets_2xb1,
                      grad_verts, grad_vert_attr, n_vert, grad_pos, grad_field, grad_attr);
    return DEFTET_OK;
}
