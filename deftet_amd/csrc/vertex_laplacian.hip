// vertex_laplacian.hip — the vertex Laplacian regulariser, r = M·x − x over a sparse vertex adjacency M, then r²:
//   training  DefTet.laplacian_sparse (layers/DefTet/deftet.py:340-343): M = D⁻¹A as a sparse [V,V] matrix (torch.sparse.mm),
//             the loss is Σ_{i,c} r² per shape;
//   render    Deftet.get_featlap (diff_render/diftet_6_subdiv/3_model/deftet.py:221-241): M = (sum over a padded neighbour
//             table) / w, the loss is r² per entry (mse_loss(..., reduction='none')).
// The adjacency is turned ONCE into a CSR and its transpose (stable radix sort of prims.hpp, as deftet_tet_vertex_csr_i32 does).
// The forward gathers the neighbours of a vertex along its CSR row; the backward dx_j = Σ_{i: j ∈ row i} a_ij u_i − u_j,
// u = 2·g·r, gathers along the row of j in the TRANSPOSED CSR.  Both sum in a fixed order: no atomics, bit-reproducible.
#include "prims.hpp"

#include "common.hpp"

namespace deftet {
namespace vlap {

using u64 = unsigned long long;

// entry e -> (major << minorBits) | minor, major = row (col for the transpose); minorBits == 0: the major index alone, so that
// the stable sort keeps the input order inside a row.  An entry with an index outside [0, V) gets all ones: it sorts behind
// every row (its major part is >= V) and is never referenced by the offsets; the flag is raised.
template <typename I>
__global__ __launch_bounds__(256) void k_vadj_keys(const I *__restrict__ rows, const I *__restrict__ cols, int nnz, int V, int transpose,
                                                   int minorBits, u64 *key, int *bad)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const long long r = (long long)rows[e], c = (long long)cols[e];
    const bool ok = r >= 0 && r < V && c >= 0 && c < V;
    if (!ok) *bad = 1;
    const u64 hi = (u64)(transpose ? c : r), lo = (u64)(transpose ? r : c);
    key[e] = ok ? (hi << minorBits) | (minorBits ? lo : 0ull) : ~0ull;
}

// position i of the sorted entries: the minor index and the value of the entry it came from, and offsets[k] = first position
// whose major index is >= k, for k in [0, V]
template <typename I>
__global__ __launch_bounds__(256) void k_vadj_fill(const u64 *__restrict__ skey, const unsigned *__restrict__ perm, int nnz, int V,
                                                   int minorBits, const I *__restrict__ minor, const float *__restrict__ vals,
                                                   int *out_idx, float *out_vals, int *offsets)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > nnz) return;
    if (i < nnz) {
        const unsigned e = perm[i];
        out_idx[i] = (int)minor[e];
        if (out_vals) out_vals[i] = vals ? vals[e] : 1.f;
    }
    auto major = [&](int k) -> long long {
        const u64 m = skey[k] >> minorBits;
        return m < (u64)V ? (long long)m : (long long)V;     // the invalid tail counts as row V
    };
    const long long prev = i == 0 ? -1 : major(i - 1), cur = i == nnz ? V : major(i);
    for (long long k = prev + 1; k <= cur; ++k) offsets[k] = i;
}

// entries per lane and trip of the row walks: all column loads of a trip, then all feature loads, are in flight together
template <int CM>
struct Unroll {
    static constexpr int value = CM <= 4 ? 8 : CM <= 8 ? 4 : 2;
};

// One lane per (shape, vertex).  nei_i = Σ_k v_k x[col_k] (fmaf, CSR order) or (Σ_k x[col_k]) / w_i (adds in table order, one
// IEEE division); r = nei − x written to r; then r² to out (NONE) or Σ_c r² of the lane into a per-workgroup partial (SHAPE),
// part[b][logical block]: a butterfly over the wave, then the four waves as (w0 + w1) + (w2 + w3).
template <int CM, bool ROWDIV, bool SHAPE>
__global__ __launch_bounds__(256) void k_vlap_fwd(const float *__restrict__ x, const int *__restrict__ offsets, const int *__restrict__ cols,
                                                  const float *__restrict__ vals, const float *__restrict__ w, int V, int C, float *r,
                                                  float *out, float *part)
{
    constexpr int U = Unroll<CM>::value;
    const int b = blockIdx.y, lb = xcd_logical_block();
    const int i = lb * 256 + threadIdx.x;
    const size_t xb = (size_t)b * V * C;
    float sq = 0.f;
    if (i < V) {
        float acc[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) acc[c] = 0.f;
        const int k0 = offsets[i], k1 = offsets[i + 1];
        for (int k = k0; k < k1; k += U) {
            int j[U];
            float a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                j[u] = k + u < k1 ? cols[k + u] : -1;
                if (!ROWDIV) a[u] = k + u < k1 ? vals[k + u] : 0.f;
            }
            float xj[U][CM];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < CM; ++c)
                    if (j[u] >= 0 && c < C) xj[u][c] = x[xb + (size_t)j[u] * C + c];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j[u] >= 0) {
#pragma unroll
                    for (int c = 0; c < CM; ++c)
                        if (c < C) acc[c] = ROWDIV ? acc[c] + xj[u][c] : fmaf(a[u], xj[u][c], acc[c]);
                }
        }
        const float wi = ROWDIV ? w[i] : 1.f;
        const size_t o = xb + (size_t)i * C;
#pragma unroll
        for (int c = 0; c < CM; ++c)
            if (c < C) {
                const float nei = ROWDIV ? acc[c] / wi : acc[c];
                const float rc = nei - x[o + c];
                r[o + c] = rc;
                if (SHAPE) sq += rc * rc;
                else out[o + c] = rc * rc;
            }
    }
    if (SHAPE) {
        __shared__ float wsum[4];
#pragma unroll  // wave_sum's order (wave.hpp); written out, a call changes this kernel's instruction stream
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) part[(size_t)b * gridDim.x + lb] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
}

// out[b] = Σ of the n partials of shape b: thread t adds partials t, t + 256, ... in order, then the same tree as above
__global__ __launch_bounds__(256) void k_vlap_final(const float *__restrict__ part, int n, float *out)
{
    __shared__ float wsum[4];
    const int b = blockIdx.x;
    float s = 0.f;
    for (int k = threadIdx.x; k < n; k += 256) s += part[(size_t)b * n + k];
#pragma unroll  // wave_sum's order (wave.hpp); written out, a call changes this kernel's instruction stream
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[b] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One lane per (shape, vertex j): dx_j = Σ_k a_k u[row_k] − u_j along the row of j in the transposed CSR (its order), with
// u = (2 g) r — g[b] for SHAPE, g[b,i,c] for NONE — and a_k u = fmaf(v_k, u, ·) (values) or u / w[row_k] (row divisor).
template <int CM, bool ROWDIV, bool SHAPE>
__global__ __launch_bounds__(256) void k_vlap_bwd(const float *__restrict__ r, const float *__restrict__ g, const int *__restrict__ toffsets,
                                                  const int *__restrict__ trows, const float *__restrict__ tvals,
                                                  const float *__restrict__ w, int V, int C, float *dx)
{
    constexpr int U = Unroll<CM>::value;
    const int b = blockIdx.y;
    const int j = xcd_logical_block() * 256 + threadIdx.x;
    if (j >= V) return;
    const size_t xb = (size_t)b * V * C;
    const float g2 = SHAPE ? 2.f * g[b] : 0.f;
    float acc[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) acc[c] = 0.f;
    const int k0 = toffsets[j], k1 = toffsets[j + 1];
    for (int k = k0; k < k1; k += U) {
        int i[U];
        float a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) i[u] = k + u < k1 ? trows[k + u] : -1;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i[u] >= 0) a[u] = ROWDIV ? w[i[u]] : tvals[k + u];
        float ui[U][CM];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < CM; ++c)
                if (i[u] >= 0 && c < C) {
                    const size_t o = xb + (size_t)i[u] * C + c;
                    ui[u][c] = (SHAPE ? g2 : 2.f * g[o]) * r[o];
                }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i[u] >= 0) {
#pragma unroll
                for (int c = 0; c < CM; ++c)
                    if (c < C) acc[c] = ROWDIV ? acc[c] + ui[u][c] / a[u] : fmaf(a[u], ui[u][c], acc[c]);
            }
    }
    const size_t o = xb + (size_t)j * C;
#pragma unroll
    for (int c = 0; c < CM; ++c)
        if (c < C) dx[o + c] = acc[c] - (SHAPE ? g2 : 2.f * g[o + c]) * r[o + c];
}

inline int bit_length(unsigned v)
{
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

inline unsigned grid_x(int V) { return (unsigned)align_up(blocks_for(V, 256), 8); }

inline size_t sort_tmp_bytes(size_t n) { return prims::radix_sort_temp_bytes<u64, unsigned>(n); }

struct CsrLayout {
    size_t bytes, sortTmpBytes;
    u64 *key, *skey;
    unsigned *perm;
    void *sortTmp;
};

inline CsrLayout csr_layout(int nnz, void *ws)
{
    CsrLayout L{};
    Arena A(ws);
    L.key = A.take<u64>((size_t)nnz);
    L.skey = A.take<u64>((size_t)nnz);
    L.perm = A.take<unsigned>((size_t)nnz);
    L.sortTmpBytes = sort_tmp_bytes((size_t)nnz);
    L.sortTmp = A.take<char>(L.sortTmpBytes);
    L.bytes = A.end();
    return L;
}

template <typename I>
int build_csr(const I *rows, const I *cols, const float *vals, int nnz, int V, int order, int32_t *offsets, int32_t *out_cols,
              float *out_vals, int32_t *t_offsets, int32_t *t_rows, float *t_vals, int32_t *bad, const CsrLayout &L, hipStream_t st)
{
    const int mb = bit_length((unsigned)V);                  // 2^mb > V: an all-ones major part is never a vertex
    const unsigned gk = blocks_for(nnz, 256), gf = blocks_for(nnz + 1, 256);
    for (int t = 0; t < 2; ++t) {
        const int minorBits = t == 0 && order == DEFTET_VADJ_ROW_INPUT ? 0 : mb;
        DEFTET_LAUNCH((k_vadj_keys<I>), dim3(gk), dim3(256), st, rows, cols, nnz, V, t, minorBits, L.key, bad);
        DEFTET_TRY(prims::radix_sort_from<u64, unsigned>(prims::PtrLoad<u64>{L.key}, L.skey, prims::IotaLoad{}, L.perm, (size_t)nnz,
                                                         mb + minorBits, L.sortTmp, L.sortTmpBytes, st));
        if (t == 0)
            DEFTET_LAUNCH((k_vadj_fill<I>), dim3(gf), dim3(256), st, (const u64 *)L.skey, (const unsigned *)L.perm, nnz, V, minorBits, cols, vals,
                          out_cols, out_vals, offsets);
        else
            DEFTET_LAUNCH((k_vadj_fill<I>), dim3(gf), dim3(256), st, (const u64 *)L.skey, (const unsigned *)L.perm, nnz, V, minorBits, rows, vals,
                          t_rows, t_vals, t_offsets);
    }
    return DEFTET_OK;
}

template <int CM>
int launch_fwd(bool rowdiv, bool shape, dim3 grid, hipStream_t st, const float *x, const int *offsets, const int *cols, const float *vals,
               const float *w, int V, int C, float *r, float *out, float *part)
{
    if (rowdiv && shape) DEFTET_LAUNCH((k_vlap_fwd<CM, true, true>), grid, dim3(256), st, x, offsets, cols, vals, w, V, C, r, out, part);
    else if (rowdiv) DEFTET_LAUNCH((k_vlap_fwd<CM, true, false>), grid, dim3(256), st, x, offsets, cols, vals, w, V, C, r, out, part);
    else if (shape) DEFTET_LAUNCH((k_vlap_fwd<CM, false, true>), grid, dim3(256), st, x, offsets, cols, vals, w, V, C, r, out, part);
    else DEFTET_LAUNCH((k_vlap_fwd<CM, false, false>), grid, dim3(256), st, x, offsets, cols, vals, w, V, C, r, out, part);
    return DEFTET_OK;
}

template <int CM>
int launch_bwd(bool rowdiv, bool shape, dim3 grid, hipStream_t st, const float *r, const float *g, const int *toffsets, const int *trows,
               const float *tvals, const float *w, int V, int C, float *dx)
{
    if (rowdiv && shape) DEFTET_LAUNCH((k_vlap_bwd<CM, true, true>), grid, dim3(256), st, r, g, toffsets, trows, tvals, w, V, C, dx);
    else if (rowdiv) DEFTET_LAUNCH((k_vlap_bwd<CM, true, false>), grid, dim3(256), st, r, g, toffsets, trows, tvals, w, V, C, dx);
    else if (shape) DEFTET_LAUNCH((k_vlap_bwd<CM, false, true>), grid, dim3(256), st, r, g, toffsets, trows, tvals, w, V, C, dx);
    else DEFTET_LAUNCH((k_vlap_bwd<CM, false, false>), grid, dim3(256), st, r, g, toffsets, trows, tvals, w, V, C, dx);
    return DEFTET_OK;
}

}  // namespace vlap
}  // namespace deftet

using namespace deftet;

extern "C" size_t deftet_vertex_adjacency_workspace_bytes(int nnz, int n_vertex)
{
    return nnz < 0 || n_vertex < 0 ? 0 : vlap::csr_layout(nnz, nullptr).bytes;
}

extern "C" int deftet_vertex_adjacency_csr_i32(const void *row_idx, const void *col_idx, int index_bytes, const float *values, int nnz,
                                               int n_vertex, int order, int32_t *offsets, int32_t *cols, float *vals, int32_t *t_offsets,
                                               int32_t *t_rows, float *t_vals, int32_t *bad_flag, void *workspace,
                                               size_t workspace_bytes, void *stream_)
{
    DEFTET_CHECK_ARG(nnz >= 0 && n_vertex >= 0 && n_vertex < 0x7FFFFFFF, "bad size (nnz=%d, n_vertex=%d)", nnz, n_vertex);
    DEFTET_CHECK_ARG(index_bytes == 4 || index_bytes == 8, "index_bytes must be 4 or 8 (got %d)", index_bytes);
    DEFTET_CHECK_ARG(order == DEFTET_VADJ_ROW_COL || order == DEFTET_VADJ_ROW_INPUT, "unknown order %d", order);
    DEFTET_CHECK_ARG(offsets && t_offsets && bad_flag, "null pointer");
    DEFTET_CHECK_ARG(nnz == 0 || (row_idx && col_idx && cols && t_rows), "null pointer");
    DEFTET_CHECK_ARG(aligned(row_idx, index_bytes) && aligned(col_idx, index_bytes), "indices must be %d-byte aligned",
                     index_bytes);
    DEFTET_CHECK_ARG(aligned(values, 4) && aligned(offsets, 4) && aligned(cols, 4) && aligned(vals, 4) &&
                         aligned(t_offsets, 4) && aligned(t_rows, 4) && aligned(t_vals, 4) && aligned(bad_flag, 4),
                     "outputs and values must be 4-byte aligned");
    const vlap::CsrLayout L = vlap::csr_layout(nnz, workspace);
    if (nnz > 0) DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    hipStream_t st = as_stream(stream_);
    DEFTET_HIP(hipMemsetAsync(bad_flag, 0, 4, st));
    if (nnz == 0) {
        DEFTET_HIP(hipMemsetAsync(offsets, 0, ((size_t)n_vertex + 1) * 4, st));
        DEFTET_HIP(hipMemsetAsync(t_offsets, 0, ((size_t)n_vertex + 1) * 4, st));
        return DEFTET_OK;
    }
    if (index_bytes == 4)
        return vlap::build_csr(static_cast<const int32_t *>(row_idx), static_cast<const int32_t *>(col_idx), values, nnz, n_vertex, order,
                               offsets, cols, vals, t_offsets, t_rows, t_vals, bad_flag, L, st);
    return vlap::build_csr(static_cast<const int64_t *>(row_idx), static_cast<const int64_t *>(col_idx), values, nnz, n_vertex, order,
                           offsets, cols, vals, t_offsets, t_rows, t_vals, bad_flag, L, st);
}

extern "C" size_t deftet_vertex_laplacian_workspace_bytes(int n_batch, int n_vertex)
{
    if (n_batch < 0 || n_vertex < 0) return 0;
    return align_up((size_t)n_batch * vlap::grid_x(n_vertex) * 4, 256);
}

// the checks both directions share
static int vlap_check(int weighting, int reduction, int n_batch, int n_vertex, int n_chan, int nnz, const int32_t *offsets,
                      const int32_t *idx, const float *vals, const float *row_weights)
{
    DEFTET_CHECK_ARG(n_batch >= 0 && n_batch <= 65535 && n_vertex >= 0 && nnz >= 0, "bad size (n_batch=%d, n_vertex=%d, nnz=%d)",
                     n_batch, n_vertex, nnz);
    DEFTET_CHECK_ARG((long long)n_vertex * 256 < 0x7FFFFFFFLL, "n_vertex=%d too large", n_vertex);
    DEFTET_CHECK_ARG(n_chan >= 1 && n_chan <= 16, "n_chan must be in 1..16 (got %d)", n_chan);
    DEFTET_CHECK_ARG(weighting == DEFTET_VLAP_VALUES || weighting == DEFTET_VLAP_ROW_DIVISOR, "unknown weighting %d", weighting);
    DEFTET_CHECK_ARG(reduction == DEFTET_VLAP_NONE || reduction == DEFTET_VLAP_SHAPE, "unknown reduction %d", reduction);
    DEFTET_CHECK_ARG(offsets && (nnz == 0 || idx), "null pointer");
    DEFTET_CHECK_ARG(weighting != DEFTET_VLAP_VALUES || nnz == 0 || vals, "null values");
    DEFTET_CHECK_ARG(weighting != DEFTET_VLAP_ROW_DIVISOR || n_vertex == 0 || row_weights, "null row weights");
    DEFTET_CHECK_ARG(aligned(offsets, 4) && aligned(idx, 4) && aligned(vals, 4) && aligned(row_weights, 4),
                     "CSR and weights must be 4-byte aligned");
    return DEFTET_OK;
}

extern "C" int deftet_vertex_laplacian_fwd_f32(const float *x, const int32_t *offsets, const int32_t *cols, const float *vals,
                                               const float *row_weights, int weighting, int reduction, int n_batch, int n_vertex,
                                               int n_chan, int nnz, float *r, float *out, void *workspace, size_t workspace_bytes,
                                               void *stream_)
{
    DEFTET_TRY(vlap_check(weighting, reduction, n_batch, n_vertex, n_chan, nnz, offsets, cols, vals, row_weights));
    const bool shape = reduction == DEFTET_VLAP_SHAPE, rowdiv = weighting == DEFTET_VLAP_ROW_DIVISOR;
    DEFTET_CHECK_ARG(out && (n_vertex == 0 || (x && r)), "null pointer");
    DEFTET_CHECK_ARG(aligned(x, 4) && aligned(r, 4) && aligned(out, 4), "x, r and out must be 4-byte aligned");
    if (shape) DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, deftet_vertex_laplacian_workspace_bytes(n_batch, n_vertex)));
    if (n_batch == 0) return DEFTET_OK;
    hipStream_t st = as_stream(stream_);
    if (n_vertex == 0) {
        if (shape) DEFTET_HIP(hipMemsetAsync(out, 0, (size_t)n_batch * 4, st));
        return DEFTET_OK;
    }
    const unsigned gx = vlap::grid_x(n_vertex);
    const dim3 grid(gx, n_batch);
    float *part = static_cast<float *>(workspace);
    int s;
    if (n_chan <= 4) s = vlap::launch_fwd<4>(rowdiv, shape, grid, st, x, offsets, cols, vals, row_weights, n_vertex, n_chan, r, out, part);
    else if (n_chan <= 8) s = vlap::launch_fwd<8>(rowdiv, shape, grid, st, x, offsets, cols, vals, row_weights, n_vertex, n_chan, r, out, part);
    else s = vlap::launch_fwd<16>(rowdiv, shape, grid, st, x, offsets, cols, vals, row_weights, n_vertex, n_chan, r, out, part);
    DEFTET_TRY(s);
    if (shape) DEFTET_LAUNCH(vlap::k_vlap_final, dim3(n_batch), dim3(256), st, (const float *)part, (int)gx, out);
    return DEFTET_OK;
}

extern "C" int deftet_vertex_laplacian_bwd_f32(const float *r, const float *grad_out, const int32_t *t_offsets, const int32_t *t_rows,
                                               const float *t_vals, const float *row_weights, int weighting, int reduction, int n_batch,
                                               int n_vertex, int n_chan, int nnz, float *grad_x, void *stream_)
{
    DEFTET_TRY(vlap_check(weighting, reduction, n_batch, n_vertex, n_chan, nnz, t_offsets, t_rows, t_vals, row_weights));
    const bool shape = reduction == DEFTET_VLAP_SHAPE, rowdiv = weighting == DEFTET_VLAP_ROW_DIVISOR;
    DEFTET_CHECK_ARG(grad_out && (n_vertex == 0 || (r && grad_x)), "null pointer");
    DEFTET_CHECK_ARG(aligned(r, 4) && aligned(grad_out, 4) && aligned(grad_x, 4),
                     "r, grad_out and grad_x must be 4-byte aligned");
    if (n_batch == 0 || n_vertex == 0) return DEFTET_OK;
    const dim3 grid(vlap::grid_x(n_vertex), n_batch);
    hipStream_t st = as_stream(stream_);
    if (n_chan <= 4) return vlap::launch_bwd<4>(rowdiv, shape, grid, st, r, grad_out, t_offsets, t_rows, t_vals, row_weights, n_vertex, n_chan, grad_x);
    if (n_chan <= 8) return vlap::launch_bwd<8>(rowdiv, shape, grid, st, r, grad_out, t_offsets, t_rows, t_vals, row_weights, n_vertex, n_chan, grad_x);
    return vlap::launch_bwd<16>(rowdiv, shape, grid, st, r, grad_out, t_offsets, t_rows, t_vals, row_weights, n_vertex, n_chan, grad_x);
}
