// tet_field_sample.hip — a per-vertex field read at query points that the indexed point-in-tet query has located:
//   value(p) = sum_k w_k(p) * field[vertex k of the tet that holds p]
// from (field, tet list, cond, bary): one forward launch, one launch for the gradient on the weights (which the existing
// deftet_point_in_tet_indexed_bwd_to_vertices_f32 takes on to the vertex positions and the points), and the gradient on the field
// as a gather over the incidence CSR.  No float atomics; every sum has one order:
//   value     ((w0 f(v0,c) + w1 f(v1,c)) + w2 f(v2,c)) + w3 f(v3,c), every product and sum rounded
//   to w      grad_w[b,q,k] = sum over c ascending of grad_out[b,q,c] * f(v_k,c): one accumulator from 0
//   to field  grad_field[b,v,c] = one accumulator from 0 over the incidences (4 t + corner, ascending) of v, per incidence over
//             the queries of shape b with cond == t in ascending q, of the rounded product bary[b,q,corner] * grad_out[b,q,c]
#include "cell_gather.hpp"

namespace deftet {
namespace {

constexpr int kTfsNarrow = 8;                                        // up to here one lane owns a query and its whole row

__device__ __forceinline__ float tfs_nan() { return __int_as_float(0x7FC00000); }

// the tet of query i = b Q + q: 0 a miss, 1 a hit with all four vertices inside [0,V) (vi holds them), -1 an index not to follow
__device__ __forceinline__ int tfs_locate(const float *__restrict__ cond, const int32_t *__restrict__ tet_idx, size_t i, int b, int V,
                                          int T, int idx_batch, int4 &vi)
{
    const float cf = cond[i];
    if (!(cf >= 0.0f)) return 0;                                     // -1, or a NaN
    if (!(cf < (float)T)) return -1;
    const int t = (int)cf;
    vi = *reinterpret_cast<const int4 *>(tet_idx + ((idx_batch > 1 ? (size_t)b * T : 0) + t) * 4);
    const bool ok = (unsigned)vi.x < (unsigned)V && (unsigned)vi.y < (unsigned)V && (unsigned)vi.z < (unsigned)V && (unsigned)vi.w < (unsigned)V;
    return ok ? 1 : -1;
}

__device__ __forceinline__ float tfs_value(const float4 w, float f0, float f1, float f2, float f3)
{
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w.x, f0), __fmul_rn(w.y, f1)), __fmul_rn(w.z, f2)), __fmul_rn(w.w, f3));
}

// grid (Q / 256, B): one lane per query, C <= kTfsNarrow.  VEC4: C == 4 with 16-byte aligned field and out, rows as one float4.
template <bool VEC4>
__global__ __launch_bounds__(kPvBlock) void k_tfs_fwd(const float *__restrict__ field, const int32_t *__restrict__ tet_idx,
                                                      const float *__restrict__ cond, const float *__restrict__ bary, float *out,
                                                      int32_t *bad, float fill, int V, int T, int Q, int C, int idx_batch)
{
    const int q = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (q >= Q) return;
    const size_t i = (size_t)b * Q + q;
    int4 vi;
    const int hit = tfs_locate(cond, tet_idx, i, b, V, T, idx_batch, vi);
    if (hit < 0 && bad) *bad = 1;
    float *o = out + i * C;
    if (hit <= 0) {
        const float r = hit == 0 ? fill : tfs_nan();
        if (VEC4) *reinterpret_cast<float4 *>(o) = make_float4(r, r, r, r);
        else
            for (int c = 0; c < C; ++c) o[c] = r;
        return;
    }
    const float4 w = *reinterpret_cast<const float4 *>(bary + i * 4);
    const float *f = field + (size_t)b * V * C;
    if (VEC4) {
        const float4 f0 = *reinterpret_cast<const float4 *>(f + (size_t)vi.x * 4), f1 = *reinterpret_cast<const float4 *>(f + (size_t)vi.y * 4),
                     f2 = *reinterpret_cast<const float4 *>(f + (size_t)vi.z * 4), f3 = *reinterpret_cast<const float4 *>(f + (size_t)vi.w * 4);
        *reinterpret_cast<float4 *>(o) = make_float4(tfs_value(w, f0.x, f1.x, f2.x, f3.x), tfs_value(w, f0.y, f1.y, f2.y, f3.y),
                                                     tfs_value(w, f0.z, f1.z, f2.z, f3.z), tfs_value(w, f0.w, f1.w, f2.w, f3.w));
    } else {
        const float *f0 = f + (size_t)vi.x * C, *f1 = f + (size_t)vi.y * C, *f2 = f + (size_t)vi.z * C, *f3 = f + (size_t)vi.w * C;
        for (int c = 0; c < C; ++c) o[c] = tfs_value(w, f0[c], f1[c], f2[c], f3[c]);
    }
}

// grid (Q C / 256, B): wide rows, one lane per (query, channel), the lanes of a row next to each other
__global__ __launch_bounds__(kPvBlock) void k_tfs_fwd_wide(const float *__restrict__ field, const int32_t *__restrict__ tet_idx,
                                                           const float *__restrict__ cond, const float *__restrict__ bary, float *out,
                                                           int32_t *bad, float fill, int V, int T, int Q, int C, int idx_batch)
{
    const long long e = (long long)blockIdx.x * kPvBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)Q * C) return;
    const int q = (int)(e / C), c = (int)(e - (long long)q * C);
    const size_t i = (size_t)b * Q + q;
    int4 vi;
    const int hit = tfs_locate(cond, tet_idx, i, b, V, T, idx_batch, vi);
    if (hit < 0 && bad && c == 0) *bad = 1;
    float r = hit == 0 ? fill : tfs_nan();
    if (hit > 0) {
        const float4 w = *reinterpret_cast<const float4 *>(bary + i * 4);
        const float *f = field + (size_t)b * V * C + c;
        r = tfs_value(w, f[(size_t)vi.x * C], f[(size_t)vi.y * C], f[(size_t)vi.z * C], f[(size_t)vi.w * C]);
    }
    out[i * C + c] = r;
}

// grid (4 Q / 256, B): one lane per (query, corner); the four lanes of a query read the same grad_out row
__global__ __launch_bounds__(kPvBlock) void k_tfs_bwd_w(const float *__restrict__ field, const int32_t *__restrict__ tet_idx,
                                                        const float *__restrict__ cond, const float *__restrict__ gout, float *gw, int V,
                                                        int T, int Q, int C, int idx_batch)
{
    const long long e = (long long)blockIdx.x * kPvBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)Q * 4) return;
    const int q = (int)(e >> 2), k = (int)(e & 3);
    const size_t i = (size_t)b * Q + q;
    int4 vi;
    float acc = 0.0f;
    if (tfs_locate(cond, tet_idx, i, b, V, T, idx_batch, vi) > 0) {
        const int v = k == 0 ? vi.x : k == 1 ? vi.y : k == 2 ? vi.z : vi.w;
        const float *f = field + ((size_t)b * V + v) * C, *g = gout + i * C;
        for (int c = 0; c < C; ++c) acc = __fadd_rn(acc, __fmul_rn(g[c], f[c]));
    }
    gw[i * 4 + k] = acc;
}

// the sort key of query i = b Q + q: its shape's block of T + 1 keys, a miss (or an index past the list) on the last one
__global__ __launch_bounds__(kPvBlock) void k_tfs_keys(const float *__restrict__ cond, unsigned *keys, long long n, int Q, int T)
{
    const long long i = (long long)blockIdx.x * kPvBlock + threadIdx.x;
    if (i >= n) return;
    const float cf = cond[i];
    const int t = cf >= 0.0f && cf < (float)T ? (int)cf : T;
    keys[i] = (unsigned)((i / Q) * ((long long)T + 1) + t);
}

// grid (V C / 256, B): one lane per (vertex, channel).  seg / perm from the stable sort of the keys above, perm holding b Q + q;
// seg == nullptr: no query at all, the zeros are written all the same.
__global__ __launch_bounds__(kPvBlock) void k_tfs_bwd_field(const float *__restrict__ gout, const float *__restrict__ bary,
                                                            const int32_t *__restrict__ offsets, const int32_t *__restrict__ slots,
                                                            const int32_t *__restrict__ seg, const int32_t *__restrict__ perm,
                                                            float *gfield, int V, int T, int C, int idx_batch, int accumulate)
{
    const long long e = (long long)blockIdx.x * kPvBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)V * C) return;
    const int v = (int)(e / C), c = (int)(e - (long long)v * C);
    float acc = 0.0f;
    if (seg) {
        const size_t row = (idx_batch > 1 ? (size_t)b * V : 0) + v;
        const int i0 = offsets[row], i1 = offsets[row + 1];
        const int32_t *sg = seg + (size_t)b * ((size_t)T + 1);
        for (int i = i0; i < i1; ++i) {
            const int s = slots[i], t = s >> 2, k = s & 3;
            const int j1 = sg[t + 1];
            for (int j = sg[t]; j < j1; ++j) {
                const size_t p = (size_t)perm[j];
                acc = __fadd_rn(acc, __fmul_rn(bary[p * 4 + k], gout[p * C + c]));
            }
        }
    }
    float *o = gfield + ((size_t)b * V + v) * C + c;
    *o = accumulate ? __fadd_rn(*o, acc) : acc;
}

// the workspace of the gradient on the field: the sort of the B Q located tets, the queries in (shape, tet) order and the table
// seg[B (T + 1) + 1]
struct TfsLayout {
    size_t bytes;
    SortBufs s;
    int32_t *perm, *seg;
};
TfsLayout tfs_layout(size_t B, size_t T, size_t Q, void *ws)
{
    TfsLayout L{};
    Arena A(ws);
    take_sort(A, B * Q, L.s);
    L.perm = A.take<int32_t>(B * Q);
    L.seg = A.take<int32_t>(B * (T + 1) + 1);
    L.bytes = A.end();
    return L;
}

int tfs_check(int B, int V, int T, int Q, int C, int idx_batch, const char *what)
{
    if (B < 0 || V < 0 || T < 0 || Q < 0) return set_error(DEFTET_EINVAL, "%s: negative size", what);
    if (C < 1) return set_error(DEFTET_EINVAL, "%s: the field needs at least one channel (got %d)", what, C);
    if (B > 65535) return set_error(DEFTET_ELIMIT, "%s: more than 65535 shapes", what);
    if (idx_batch != 1 && idx_batch != B) return set_error(DEFTET_EINVAL, "%s: tet list batch must be 1 or n_batch (got %d)", what, idx_batch);
    if (T >= (1 << 24)) return set_error(DEFTET_ELIMIT, "%s: a float cond names at most 2^24 tets", what);
    if ((long long)B * V >= 0x7FFFFFFFll || (long long)B * Q >= 0x7FFFFFFFll || (long long)B * ((long long)T + 1) >= 0x7FFFFFFFll ||
        (long long)idx_batch * T * 4 >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: B V, B Q, B (T + 1) or 4 T does not fit 31 bits", what);
    if (((long long)Q * C + kPvBlock - 1) / kPvBlock >= 0x7FFFFFFFll || ((long long)V * C + kPvBlock - 1) / kPvBlock >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: Q C or V C exceeds what one grid covers", what);
    return DEFTET_OK;
}

}  // namespace
}  // namespace deftet

using namespace deftet;

extern "C" {

size_t deftet_tet_field_sample_workspace_bytes(int n_batch, int n_tet, int n_query)
{
    if (n_batch < 0 || n_tet < 0 || n_query < 0) return 0;
    return tfs_layout((size_t)n_batch, (size_t)n_tet, (size_t)n_query, nullptr).bytes;
}

int deftet_tet_field_sample_fwd_f32(const float *field, const int32_t *tet_idx, const float *cond, const float *bary, float *out,
                                    int32_t *bad_flag, float fill, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_query,
                                    int n_channel, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, Q = n_query, C = n_channel;
    DEFTET_TRY(tfs_check(B, V, T, Q, C, idx_batch, "tet_field_sample"));
    if (B == 0 || Q == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(cond && bary && out && (field || V == 0) && (tet_idx || T == 0), "tet_field_sample: null pointer");
    DEFTET_CHECK_ARG((((uintptr_t)tet_idx | (uintptr_t)bary) & 15) == 0, "tet_field_sample: tet_idx and bary must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (C > kTfsNarrow) {
        DEFTET_LAUNCH(k_tfs_fwd_wide, dim3(blocks_for((long long)Q * C, kPvBlock), (unsigned)B), dim3(kPvBlock), st, field, tet_idx, cond, bary, out,
                      bad_flag, fill, V, T, Q, C, idx_batch);
    } else if (C == 4 && (((uintptr_t)field | (uintptr_t)out) & 15) == 0) {
        DEFTET_LAUNCH(k_tfs_fwd<true>, dim3(blocks_for(Q, kPvBlock), (unsigned)B), dim3(kPvBlock), st, field, tet_idx, cond, bary, out, bad_flag, fill, V,
                      T, Q, C, idx_batch);
    } else {
        DEFTET_LAUNCH(k_tfs_fwd<false>, dim3(blocks_for(Q, kPvBlock), (unsigned)B), dim3(kPvBlock), st, field, tet_idx, cond, bary, out, bad_flag, fill, V,
                      T, Q, C, idx_batch);
    }
    return DEFTET_OK;
}

int deftet_tet_field_sample_bwd_w_f32(const float *field, const int32_t *tet_idx, const float *cond, const float *grad_out, float *grad_w,
                                      int n_batch, int n_vertex, int n_tet, int idx_batch, int n_query, int n_channel, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, Q = n_query, C = n_channel;
    DEFTET_TRY(tfs_check(B, V, T, Q, C, idx_batch, "tet_field_sample_bwd_w"));
    if (B == 0 || Q == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(cond && grad_out && grad_w && (field || V == 0) && (tet_idx || T == 0), "tet_field_sample_bwd_w: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_field_sample_bwd_w: tet_idx must be 16-byte aligned");
    DEFTET_LAUNCH(k_tfs_bwd_w, dim3(blocks_for((long long)Q * 4, kPvBlock), (unsigned)B), dim3(kPvBlock), as_stream(stream), field, tet_idx, cond,
                  grad_out, grad_w, V, T, Q, C, idx_batch);
    return DEFTET_OK;
}

int deftet_tet_field_sample_bwd_field_f32(const float *grad_out, const float *cond, const float *bary, const int32_t *offsets,
                                          const int32_t *slots, float *grad_field, int n_batch, int n_vertex, int n_tet, int idx_batch,
                                          int n_query, int n_channel, int accumulate, void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, Q = n_query, C = n_channel;
    DEFTET_TRY(tfs_check(B, V, T, Q, C, idx_batch, "tet_field_sample_bwd_field"));
    const bool sorted = B > 0 && Q > 0;
    const TfsLayout L = tfs_layout((size_t)B, (size_t)T, (size_t)Q, workspace);
    if (sorted) DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(offsets && grad_field && (T == 0 || slots) && (Q == 0 || (grad_out && cond && bary)),
                     "tet_field_sample_bwd_field: null pointer");
    hipStream_t st = as_stream(stream);
    if (sorted) {
        const long long n = (long long)B * Q;
        DEFTET_LAUNCH(k_tfs_keys, dim3(blocks_for(n, kPvBlock)), dim3(kPvBlock), st, cond, L.s.keys, n, Q, T);
        DEFTET_TRY(sort_and_segment(L.s, L.perm, L.seg, (size_t)n, (unsigned)((long long)B * ((long long)T + 1)), st));
    }
    DEFTET_LAUNCH(k_tfs_bwd_field, dim3(blocks_for((long long)V * C, kPvBlock), (unsigned)B), dim3(kPvBlock), st, grad_out, bary, offsets, slots,
                  sorted ? (const int32_t *)L.seg : (const int32_t *)nullptr, sorted ? (const int32_t *)L.perm : (const int32_t *)nullptr,
                  grad_field, V, T, C, idx_batch, accumulate);
    return DEFTET_OK;
}

}  // extern "C"
