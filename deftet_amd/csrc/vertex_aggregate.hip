// vertex_aggregate.hip — the wide-channel vertex aggregation out = M·x over a sparse vertex adjacency M: the sparse product of
// the GCN position decoder, GraphConv.forward (layers/gcn_decoder.py:55-56) through sparse_batch_matmul
// (utils/matrix_utils.py:22-33), x f32 [B,V,C] with C = 128 or 256 at the training sizes.  M is the CSR that
// deftet_vertex_adjacency_csr_i32 (vertex_laplacian.hip) builds once per topology; the backward dx = Mᵀ·g is the SAME kernel on
// the transposed CSR.  Where vertex_laplacian walks a row with one lane (C <= 16), here a group of lanes owns a row and the lanes
// cover the channels, so every neighbour row of x is read as contiguous 16-byte loads.
// Every channel of every path: acc = 0.f, then one fmaf per entry in CSR order — no atomics, bit-reproducible, and a channel's
// result does not depend on C or on the path that ran.
#include "common.hpp"

namespace deftet {
namespace vagg {

template <int VEC>
struct Chan;
template <>
struct Chan<1> {
    float v;
    __device__ __forceinline__ void zero() { v = 0.f; }
    __device__ __forceinline__ void load(const float *p) { v = *p; }
    __device__ __forceinline__ void store(float *p) const { *p = v; }
    __device__ __forceinline__ void fma(float a, const Chan &x) { v = fmaf(a, x.v, v); }
};
template <>
struct Chan<4> {
    float4 v;
    __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
    __device__ __forceinline__ void load(const float *p) { v = *reinterpret_cast<const float4 *>(p); }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = v; }
    __device__ __forceinline__ void fma(float a, const Chan &x)
    {
        v.x = fmaf(a, x.v.x, v.x);
        v.y = fmaf(a, x.v.y, v.y);
        v.z = fmaf(a, x.v.z, v.z);
        v.w = fmaf(a, x.v.w, v.w);
    }
};

// LPR lanes own one row of one shape (64 / LPR rows per wave, four waves per workgroup); lane g of the group covers the VEC
// channels from (c0 + g)·VEC of every chunk c0 = 0, LPR, 2·LPR, ... (VEC = 4: 256 channels per chunk and wave at LPR = 64, one
// 16-byte load per lane and neighbour; VEC = 1: the scalar path for C % 4 != 0).  The row's entries are loaded LPR at a time by
// the group's lanes (one coalesced read of idx and of vals) and handed round with shuffles; a row longer than LPR entries
// reloads that window.  U neighbour rows are in flight per lane and trip.  The trip counts are those of the longest row of the
// wave, so that every shuffle runs with all lanes: a shorter row's missing entries are -1 and skipped.
template <int VEC, int LPR>
__global__ __launch_bounds__(256) void k_vagg(const float *__restrict__ x, const int *__restrict__ offsets, const int *__restrict__ idx,
                                              const float *__restrict__ vals, int V, int C, float *__restrict__ out)
{
    constexpr int RPW = 64 / LPR, U = VEC == 4 ? 4 : 8;
    static_assert(LPR % U == 0, "a trip never crosses the window");
    const int lane = threadIdx.x & 63, g = lane & (LPR - 1);
    const long long row = ((long long)xcd_logical_block() * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool live = row < V;
    const int i = live ? (int)row : 0;
    const size_t xb = (size_t)blockIdx.y * V * C;
    const int k0 = live ? offsets[i] : 0, k1 = live ? offsets[i + 1] : 0;
    int nmax = k1 - k0;
#pragma unroll  // across the row groups of the wave, offsets LPR upward: an order of its own, not wave.hpp's wave_max (int max: same value)
    for (int off = LPR; off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off));
    const int CV = C / VEC;
    for (int c0 = 0; c0 < CV; c0 += LPR) {
        const int cv = c0 + g;
        const bool on = live && cv < CV;
        const float *xc = x + xb + (size_t)cv * VEC;
        Chan<VEC> acc;
        acc.zero();
        for (int w = 0; w < nmax; w += LPR) {
            const int kw = k0 + w + g;
            const int jw = kw < k1 ? idx[kw] : -1;
            const float aw = kw < k1 ? vals[kw] : 0.f;
            const int wn = min(nmax - w, LPR);
            for (int t = 0; t < wn; t += U) {
                int j[U];
                float a[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    j[u] = __shfl(jw, t + u, LPR);
                    a[u] = __shfl(aw, t + u, LPR);
                }
                Chan<VEC> xj[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    xj[u].zero();
                    if (on && j[u] >= 0) xj[u].load(xc + (size_t)j[u] * C);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j[u] >= 0) acc.fma(a[u], xj[u]);
            }
        }
        if (on) acc.store(out + xb + (size_t)i * C + (size_t)cv * VEC);
    }
}

template <int VEC, int LPR>
int launch(hipStream_t st, const float *x, const int *offsets, const int *idx, const float *vals, int B, int V, int C, float *out)
{
    const long long rowsPerBlock = 4 * (64 / LPR);
    const long long blocks = ((long long)V + rowsPerBlock - 1) / rowsPerBlock;
    const dim3 grid((unsigned)(blocks_for(blocks, 8) * 8), (unsigned)B);
    DEFTET_LAUNCH((k_vagg<VEC, LPR>), grid, dim3(256), st, x, offsets, idx, vals, V, C, out);
    return DEFTET_OK;
}

template <int VEC>
int launch_width(hipStream_t st, const float *x, const int *offsets, const int *idx, const float *vals, int B, int V, int C, float *out)
{
    const int cv = C / VEC;                                  // lanes a row can use: narrow rows share a wave
    if (cv <= 16) return launch<VEC, 16>(st, x, offsets, idx, vals, B, V, C, out);
    if (cv <= 32) return launch<VEC, 32>(st, x, offsets, idx, vals, B, V, C, out);
    return launch<VEC, 64>(st, x, offsets, idx, vals, B, V, C, out);
}

}  // namespace vagg
}  // namespace deftet

using namespace deftet;

extern "C" int deftet_vertex_aggregate_f32(const float *x, const int32_t *offsets, const int32_t *idx, const float *vals, int n_batch,
                                           int n_vertex, int n_channel, int nnz, float *out, void *stream_)
{
    DEFTET_CHECK_ARG(n_batch >= 0 && n_batch <= 65535 && n_vertex >= 0 && nnz >= 0, "bad size (n_batch=%d, n_vertex=%d, nnz=%d)", n_batch,
                     n_vertex, nnz);
    DEFTET_CHECK_ARG(n_channel >= 1, "n_channel must be at least 1 (got %d)", n_channel);
    DEFTET_CHECK_ARG(n_vertex < 0x7FFFFFFF, "n_vertex=%d too large", n_vertex);
    DEFTET_CHECK_ARG(offsets && (nnz == 0 || (idx && vals)), "null CSR pointer");
    const bool work = n_batch > 0 && n_vertex > 0;
    DEFTET_CHECK_ARG(!work || (x && out), "null pointer");
    DEFTET_CHECK_ARG(aligned(x, 4) && aligned(out, 4) && aligned(offsets, 4) && aligned(idx, 4) &&
                         aligned(vals, 4),
                     "x, out and the CSR must be 4-byte aligned");
    if (!work) return DEFTET_OK;
    hipStream_t st = as_stream(stream_);
    if (n_channel % 4 == 0 && aligned(x, 16) && aligned(out, 16))
        return vagg::launch_width<4>(st, x, offsets, idx, vals, n_batch, n_vertex, n_channel, out);
    return vagg::launch_width<1>(st, x, offsets, idx, vals, n_batch, n_vertex, n_channel, out);
}
