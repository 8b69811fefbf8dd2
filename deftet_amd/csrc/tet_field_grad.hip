// tet_field_grad.hip — the gradient of a per-vertex field on the tets, its two energies, and per-tet values carried to the
// vertices.  For one tet with vertices v0..v3 at x0..x3 and the rows e0 = x1 - x0, e1 = x2 - x0, e2 = x3 - x0:
//   n0 = e1 x e2, n1 = e2 x e0, n2 = e0 x e1, det = e0 . n0, vol = det / 6
//   g_c = (n0 df0 + n1 df1 + n2 df2) / det with df_k = f(v_{k+1},c) - f(v0,c)         (the adjugate form of E^-1 df)
// A tet is LIVE iff det > 0 in fp32 and its four indices lie in [0,V); a dead tet (NaN, flat, inverted) has gradient 0 and
// volume 0 and takes part in no energy and no backward.  With m_0 = -(n0 + n1 + n2) and m_k = n_{k-1} (the gradient of corner
// k's hat function times det):
//   d g_c / d f(v_k,c) = m_k / det          d vol / d x_k = m_k / 6          d g_c / d x_k = -(m_k / det) g_c^T
// No float atomics; every sum has one order:
//   to field     grad_field[b,v,c] = one accumulator from 0 over the incidences (4 t + corner, ascending) of v of (m_k . G_c) / det
//   to pos       grad_pos[b,v] = one accumulator from 0 over the same incidences of the row
//                (sum over c ascending of -((m_k . G_c) / det) g_c, from 0) + gvol m_k / 6
//   energies     per thread a double per sum over its tets in ascending t, the wave butterfly, the waves of a workgroup in
//                ascending order, then the 64 workgroups of a shape by the butterfly again (k_tfe_final)
//   to vertices  num = sum of fl(w_t val_t), den = sum of w_t over the incidences in CSR order, one fp32 accumulator each from 0,
//                out = num / den; back: gval[t,c] = w_t * (sum over the corners 0..3 of gout[v_k,c] / den[v_k], from 0)
// G_c is the gradient arriving on g_c: read from memory (tet_field_gradient) or formed from the energies' saved sums.
#include "common.hpp"
#include "tet_frame.hpp"                                             // tet_frame: the tet's adjugate rows, det and whether it is live
#include "wave.hpp"

namespace deftet {
namespace {

constexpr int kTfgBlock = 256;
constexpr int kTfeMaxC = 8;                                          // channels of the energies (as marching_tets' attr)
constexpr int kTfeParts = 64;                                        // workgroups per shape of the energy pass: one partial per lane of k_tfe_final
constexpr int kTfeStats = 1 + 2 * kTfeMaxC;                          // W, then S0_c / W, then S1_c / W

// g_c of a live tet; f points at channel c of vertex 0 of the shape's field
__device__ __forceinline__ void tfg_grad(const float *__restrict__ f, int C, const int vi[4], const float n[3][3], float det, float g[3])
{
    const float f0 = f[(size_t)vi[0] * C];
    const float d0 = f[(size_t)vi[1] * C] - f0, d1 = f[(size_t)vi[2] * C] - f0, d2 = f[(size_t)vi[3] * C] - f0;
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = ((n[0][a] * d0 + n[1][a] * d1) + n[2][a] * d2) / det;
}

// m_k: det times the gradient of corner k's hat function
__device__ __forceinline__ void tfg_corner(const float n[3][3], int k, float m[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = k == 0 ? -((n[0][a] + n[1][a]) + n[2][a]) : k == 1 ? n[0][a] : k == 2 ? n[1][a] : n[2][a];
}

// grid (T C / 256, B): one lane per (tet, channel), the lanes of a tet next to each other; 12 contiguous bytes per lane
__global__ __launch_bounds__(kTfgBlock) void k_tfg_fwd(const float *__restrict__ field, const float *__restrict__ pos,
                                                       const int32_t *__restrict__ tet_idx, float *out, float *vol, int V, int T, int C,
                                                       int idx_batch)
{
    const long long e = (long long)blockIdx.x * kTfgBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)T * C) return;
    const int t = (int)(e / C), c = (int)(e - (long long)t * C);
    int vi[4];
    float n[3][3], det, g[3] = {0.0f, 0.0f, 0.0f};
    const bool live = tet_frame(pos + (size_t)b * V * 3, tet_idx, (idx_batch > 1 ? (size_t)b * T : 0) + t, V, vi, n, det);
    if (out) {                                                        // (without it: the volumes alone)
        if (live) tfg_grad(field + (size_t)b * V * C + c, C, vi, n, det, g);
        float *o = out + (((size_t)b * T + t) * C + c) * 3;
        o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
    }
    if (vol && c == 0) vol[(size_t)b * T + t] = live ? det / 6.0f : 0.0f;
}

// What arrives on the gradients of a tet.  Explicit: the rows of grad_out [B,T,C,3] and grad_vol [B,T].  Energies: formed from
// the saved sums, out[c,0] = S0_c / W and out[c,1] = S1_c / W with w = vol, S0 = sum w |g|^2, S1 = sum w (|g| - target)^2:
//   d / d g_c = (w / W) (2 go0 + 2 go1 (|g| - target) / |g|) g_c       (the second term 0 where |g| = 0)
//   d / d w   = (go0 (|g|^2 - out0) + go1 ((|g| - target)^2 - out1)) / W, summed over the channels
struct TfgExplicit {
    const float *gout, *gvol;                                        // of the shape
    int C;
    __device__ __forceinline__ void on_grad(int t, int c, const float *, float, float G[3], float &gv) const
    {
        const float *r = gout + ((size_t)t * C + c) * 3;
        G[0] = r[0]; G[1] = r[1]; G[2] = r[2];
    }
    __device__ __forceinline__ float on_vol(int t) const { return gvol ? gvol[t] : 0.0f; }
};
struct TfgEnergies {
    const double *stats;                                             // of the shape: kTfeStats doubles
    const float *go;                                                 // of the shape: [C,2]
    float target, inv_w;
    __device__ __forceinline__ void on_grad(int, int c, const float g[3], float det, float G[3], float &gv) const
    {
        const float go0 = go[2 * c], go1 = go[2 * c + 1];
        const float s2 = dot3(g, g), s = sqrtf(s2), d = s - target;
        const float coef = (det / 6.0f) * inv_w * (2.0f * go0 + (s > 0.0f ? 2.0f * go1 * d / s : 0.0f));
        G[0] = coef * g[0]; G[1] = coef * g[1]; G[2] = coef * g[2];
        gv += (go0 * (s2 - (float)stats[1 + c]) + go1 * (d * d - (float)stats[1 + kTfeMaxC + c])) * inv_w;
    }
    __device__ __forceinline__ float on_vol(int) const { return 0.0f; }
};

__device__ __forceinline__ TfgExplicit tfg_upstream(const float *gout, const float *gvol, int b, int T, int C)
{
    return TfgExplicit{gout + (size_t)b * T * C * 3, gvol ? gvol + (size_t)b * T : nullptr, C};
}
__device__ __forceinline__ TfgEnergies tfg_upstream(const double *stats, const float *go, float target, int b, int C)
{
    const double W = stats[(size_t)b * kTfeStats];
    return TfgEnergies{stats + (size_t)b * kTfeStats, go + (size_t)b * C * 2, target, W > 0.0 ? (float)(1.0 / W) : 0.0f};
}

// grid (V C / 256, B): one lane per (vertex, channel) walks the vertex's incidences
template <typename Up>
__device__ __forceinline__ void tfg_bwd_field(const Up up, const float *__restrict__ field, const float *__restrict__ pos,
                                              const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                              const int32_t *__restrict__ slots, float *gfield, int b, int V, int T, int C, int idx_batch)
{
    const long long e = (long long)blockIdx.x * kTfgBlock + threadIdx.x;
    if (e >= (long long)V * C) return;
    const int v = (int)(e / C), c = (int)(e - (long long)v * C);
    const size_t row = (idx_batch > 1 ? (size_t)b * V : 0) + v, tbase = idx_batch > 1 ? (size_t)b * T : 0;
    const int i0 = offsets[row], i1 = offsets[row + 1];
    const float *p = pos + (size_t)b * V * 3, *f = field + (size_t)b * V * C + c;
    float acc = 0.0f;
    for (int i = i0; i < i1; ++i) {
        const int s = slots[i], t = s >> 2, k = s & 3;
        if ((unsigned)t >= (unsigned)T) continue;
        int vi[4];
        float n[3][3], det, g[3], G[3], m[3], gv = 0.0f;
        if (!tet_frame(p, tet_idx, tbase + t, V, vi, n, det)) continue;
        tfg_grad(f, C, vi, n, det, g);
        up.on_grad(t, c, g, det, G, gv);
        tfg_corner(n, k, m);
        acc = acc + dot3(m, G) / det;
    }
    gfield[((size_t)b * V + v) * C + c] = acc;
}

// grid (V / 256, B): one lane per vertex walks its incidences and, per incidence, the channels
template <typename Up>
__device__ __forceinline__ void tfg_bwd_pos(const Up up, const float *__restrict__ field, const float *__restrict__ pos,
                                            const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                            const int32_t *__restrict__ slots, float *gpos, int b, int V, int T, int C, int idx_batch)
{
    const int v = blockIdx.x * kTfgBlock + threadIdx.x;
    if (v >= V) return;
    const size_t row = (idx_batch > 1 ? (size_t)b * V : 0) + v, tbase = idx_batch > 1 ? (size_t)b * T : 0;
    const int i0 = offsets[row], i1 = offsets[row + 1];
    const float *p = pos + (size_t)b * V * 3, *f = field + (size_t)b * V * C;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int i = i0; i < i1; ++i) {
        const int s = slots[i], t = s >> 2, k = s & 3;
        if ((unsigned)t >= (unsigned)T) continue;
        int vi[4];
        float n[3][3], det, m[3];
        if (!tet_frame(p, tet_idx, tbase + t, V, vi, n, det)) continue;
        tfg_corner(n, k, m);
        float r[3] = {0.0f, 0.0f, 0.0f}, gv = up.on_vol(t);
        for (int c = 0; c < C; ++c) {
            float g[3], G[3];
            tfg_grad(f + c, C, vi, n, det, g);
            up.on_grad(t, c, g, det, G, gv);
            const float a = dot3(m, G) / det;
#pragma unroll
            for (int x = 0; x < 3; ++x) r[x] = r[x] - a * g[x];
        }
#pragma unroll
        for (int x = 0; x < 3; ++x) acc[x] = acc[x] + (r[x] + gv * m[x] / 6.0f);
    }
    float *o = gpos + ((size_t)b * V + v) * 3;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
}

__global__ __launch_bounds__(kTfgBlock) void k_tfg_bwd_field(const float *__restrict__ gout, const float *__restrict__ gvol,
                                                             const float *__restrict__ field, const float *__restrict__ pos,
                                                             const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                                             const int32_t *__restrict__ slots, float *gfield, int V, int T, int C,
                                                             int idx_batch)
{
    const int b = blockIdx.y;
    tfg_bwd_field(tfg_upstream(gout, gvol, b, T, C), field, pos, tet_idx, offsets, slots, gfield, b, V, T, C, idx_batch);
}
__global__ __launch_bounds__(kTfgBlock) void k_tfg_bwd_pos(const float *__restrict__ gout, const float *__restrict__ gvol,
                                                           const float *__restrict__ field, const float *__restrict__ pos,
                                                           const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ slots, float *gpos, int V, int T, int C, int idx_batch)
{
    const int b = blockIdx.y;
    tfg_bwd_pos(tfg_upstream(gout, gvol, b, T, C), field, pos, tet_idx, offsets, slots, gpos, b, V, T, C, idx_batch);
}
__global__ __launch_bounds__(kTfgBlock) void k_tfe_bwd_field(const double *__restrict__ stats, const float *__restrict__ go, float target,
                                                             const float *__restrict__ field, const float *__restrict__ pos,
                                                             const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                                             const int32_t *__restrict__ slots, float *gfield, int V, int T, int C,
                                                             int idx_batch)
{
    const int b = blockIdx.y;
    tfg_bwd_field(tfg_upstream(stats, go, target, b, C), field, pos, tet_idx, offsets, slots, gfield, b, V, T, C, idx_batch);
}
__global__ __launch_bounds__(kTfgBlock) void k_tfe_bwd_pos(const double *__restrict__ stats, const float *__restrict__ go, float target,
                                                           const float *__restrict__ field, const float *__restrict__ pos,
                                                           const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ slots, float *gpos, int V, int T, int C, int idx_batch)
{
    const int b = blockIdx.y;
    tfg_bwd_pos(tfg_upstream(stats, go, target, b, C), field, pos, tet_idx, offsets, slots, gpos, b, V, T, C, idx_batch);
}

// grid (kTfeParts, B): per workgroup the sums (W, S0_c, S1_c) over its tets, in doubles
__global__ __launch_bounds__(kTfgBlock) void k_tfe_pass(const float *__restrict__ field, const float *__restrict__ pos,
                                                        const int32_t *__restrict__ tet_idx, double *part, float target, int V, int T,
                                                        int C, int idx_batch)
{
    __shared__ double sh[kTfgBlock / 64][kTfeStats];
    const int b = blockIdx.y;
    const float *p = pos + (size_t)b * V * 3, *f = field + (size_t)b * V * C;
    const size_t tbase = idx_batch > 1 ? (size_t)b * T : 0;
    double acc[kTfeStats];
#pragma unroll
    for (int k = 0; k < kTfeStats; ++k) acc[k] = 0.0;
    for (int t = blockIdx.x * kTfgBlock + threadIdx.x; t < T; t += kTfeParts * kTfgBlock) {
        int vi[4];
        float n[3][3], det;
        if (!tet_frame(p, tet_idx, tbase + t, V, vi, n, det)) continue;
        const double w = (double)(det / 6.0f);
        acc[0] += w;
#pragma unroll
        for (int c = 0; c < kTfeMaxC; ++c)
            if (c < C) {
                float g[3];
                tfg_grad(f + c, C, vi, n, det, g);
                const float s2 = dot3(g, g), d = sqrtf(s2) - target;
                acc[1 + c] += w * (double)s2;
                acc[1 + kTfeMaxC + c] += w * (double)(d * d);
            }
    }
#pragma unroll
    for (int k = 0; k < kTfeStats; ++k) acc[k] = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < kTfeStats; ++k) sh[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < kTfeStats) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kTfgBlock / 64; ++w) s += sh[w][threadIdx.x];
        part[((size_t)b * kTfeParts + blockIdx.x) * kTfeStats + threadIdx.x] = s;
    }
}

// grid (B), one wave: lane l holds the partial of workgroup l
__global__ __launch_bounds__(64) void k_tfe_final(const double *__restrict__ part, double *stats, float *out, int C)
{
    const int b = blockIdx.x;
    const double *src = part + ((size_t)b * kTfeParts + threadIdx.x) * kTfeStats;
    double v[kTfeStats];
#pragma unroll
    for (int k = 0; k < kTfeStats; ++k) v[k] = wave_sum(src[k]);
    if (threadIdx.x != 0) return;
    const double W = v[0];
    double *st = stats + (size_t)b * kTfeStats;
    st[0] = W;
#pragma unroll
    for (int k = 1; k < kTfeStats; ++k) st[k] = W > 0.0 ? v[k] / W : 0.0;
#pragma unroll
    for (int c = 0; c < kTfeMaxC; ++c)
        if (c < C) {
            out[((size_t)b * C + c) * 2] = (float)st[1 + c];
            out[((size_t)b * C + c) * 2 + 1] = (float)st[1 + kTfeMaxC + c];
        }
}
static_assert(kTfeParts == 64, "k_tfe_final reads one partial per lane of a wave");

// grid (V C / 256, B): one lane per (vertex, channel)
__global__ __launch_bounds__(kTfgBlock) void k_ttv_fwd(const float *__restrict__ val, const float *__restrict__ weights,
                                                       const int32_t *__restrict__ offsets, const int32_t *__restrict__ slots, float *out,
                                                       float *wsum, float fill, int V, int T, int C, int idx_batch)
{
    const long long e = (long long)blockIdx.x * kTfgBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)V * C) return;
    const int v = (int)(e / C), c = (int)(e - (long long)v * C);
    const size_t row = (idx_batch > 1 ? (size_t)b * V : 0) + v;
    const int i0 = offsets[row], i1 = offsets[row + 1];
    const float *x = val + (size_t)b * T * C + c, *w = weights ? weights + (size_t)b * T : nullptr;
    float num = 0.0f, den = 0.0f;
    for (int i = i0; i < i1; ++i) {
        const int t = slots[i] >> 2;
        if ((unsigned)t >= (unsigned)T) continue;
        const float wt = w ? w[t] : 1.0f;
        num = __fadd_rn(num, __fmul_rn(wt, x[(size_t)t * C]));
        den = __fadd_rn(den, wt);
    }
    out[((size_t)b * V + v) * C + c] = den > 0.0f ? __fdiv_rn(num, den) : fill;
    if (c == 0) wsum[(size_t)b * V + v] = den;
}

// grid (T C / 256, B): one lane per (tet, channel) gathers its four corners
__global__ __launch_bounds__(kTfgBlock) void k_ttv_bwd(const float *__restrict__ gout, const float *__restrict__ wsum,
                                                       const float *__restrict__ weights, const int32_t *__restrict__ tet_idx, float *gval,
                                                       int V, int T, int C, int idx_batch)
{
    const long long e = (long long)blockIdx.x * kTfgBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (long long)T * C) return;
    const int t = (int)(e / C), c = (int)(e - (long long)t * C);
    const int4 q = *reinterpret_cast<const int4 *>(tet_idx + ((idx_batch > 1 ? (size_t)b * T : 0) + t) * 4);
    const int vi[4] = {q.x, q.y, q.z, q.w};
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((unsigned)vi[k] >= (unsigned)V) continue;
        const float W = wsum[(size_t)b * V + vi[k]];
        if (W > 0.0f) acc = __fadd_rn(acc, __fdiv_rn(gout[((size_t)b * V + vi[k]) * C + c], W));
    }
    gval[((size_t)b * T + t) * C + c] = __fmul_rn(weights ? weights[(size_t)b * T + t] : 1.0f, acc);
}

// the workspace of the energies: the partial sums of the pass
struct TfeLayout {
    size_t bytes;
    double *part;
};
TfeLayout tfe_layout(size_t B, void *ws)
{
    TfeLayout L{};
    Arena A(ws);
    L.part = A.take<double>(B * kTfeParts * kTfeStats);
    L.bytes = A.end();
    return L;
}

int tfg_check(int B, int V, int T, int C, int idx_batch, const char *what)
{
    if (B < 0 || V < 0 || T < 0) return set_error(DEFTET_EINVAL, "%s: negative size", what);
    if (C < 1) return set_error(DEFTET_EINVAL, "%s: at least one channel expected (got %d)", what, C);
    if (B > 65535) return set_error(DEFTET_ELIMIT, "%s: more than 65535 shapes", what);
    if (idx_batch != 1 && idx_batch != B) return set_error(DEFTET_EINVAL, "%s: tet list batch must be 1 or n_batch (got %d)", what, idx_batch);
    if ((long long)B * V >= 0x7FFFFFFFll || (long long)B * T * 4 >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: B V or 4 B T does not fit 31 bits", what);
    if (((long long)T * C + kTfgBlock - 1) / kTfgBlock >= 0x7FFFFFFFll || ((long long)V * C + kTfgBlock - 1) / kTfgBlock >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: T C or V C exceeds what one grid covers", what);
    return DEFTET_OK;
}

}  // namespace
}  // namespace deftet

using namespace deftet;

extern "C" {

int deftet_tet_field_gradient_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, float *out, float *vol, int n_batch,
                                      int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, C = n_channel;
    DEFTET_TRY(tfg_check(B, V, T, C, idx_batch, "tet_field_gradient"));
    if (B == 0 || T == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(tet_idx && (out || vol) && (((field || !out) && pos) || V == 0), "tet_field_gradient: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_field_gradient: tet_idx must be 16-byte aligned");
    const int lanes = out ? C : 1;                                    // per tet
    DEFTET_LAUNCH(k_tfg_fwd, dim3(blocks_for((long long)T * lanes, kTfgBlock), (unsigned)B), dim3(kTfgBlock), as_stream(stream), field, pos, tet_idx,
                  out, vol, V, T, lanes, idx_batch);
    return DEFTET_OK;
}

int deftet_tet_field_gradient_bwd_f32(const float *grad_out, const float *grad_vol, const float *field, const float *pos,
                                      const int32_t *tet_idx, const int32_t *offsets, const int32_t *slots, float *grad_field,
                                      float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, C = n_channel;
    DEFTET_TRY(tfg_check(B, V, T, C, idx_batch, "tet_field_gradient_bwd"));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(field && pos && offsets && (T == 0 || (tet_idx && slots && grad_out)), "tet_field_gradient_bwd: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_field_gradient_bwd: tet_idx must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (grad_field)
        DEFTET_LAUNCH(k_tfg_bwd_field, dim3(blocks_for((long long)V * C, kTfgBlock), (unsigned)B), dim3(kTfgBlock), st, grad_out, grad_vol, field, pos,
                      tet_idx, offsets, slots, grad_field, V, T, C, idx_batch);
    if (grad_pos)
        DEFTET_LAUNCH(k_tfg_bwd_pos, dim3(blocks_for(V, kTfgBlock), (unsigned)B), dim3(kTfgBlock), st, grad_out, grad_vol, field, pos, tet_idx, offsets,
                      slots, grad_pos, V, T, C, idx_batch);
    return DEFTET_OK;
}

size_t deftet_tet_field_energies_workspace_bytes(int n_batch)
{
    return n_batch < 0 ? 0 : tfe_layout((size_t)n_batch, nullptr).bytes;
}

int deftet_tet_field_energies_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, float *out, double *stats, float target,
                                      int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, C = n_channel;
    if (C < 1 || C > kTfeMaxC)
        return set_error(DEFTET_EINVAL, "tet_field_energies: between 1 and %d channels expected (got %d)", kTfeMaxC, C);
    DEFTET_TRY(tfg_check(B, V, T, C, idx_batch, "tet_field_energies"));
    const TfeLayout L = tfe_layout((size_t)B, workspace);
    if (B == 0) return DEFTET_OK;
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    DEFTET_CHECK_ARG(out && stats && (T == 0 || tet_idx) && ((field && pos) || V == 0 || T == 0), "tet_field_energies: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_field_energies: tet_idx must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    DEFTET_LAUNCH(k_tfe_pass, dim3(kTfeParts, (unsigned)B), dim3(kTfgBlock), st, field, pos, tet_idx, L.part, target, V, T, C, idx_batch);
    DEFTET_LAUNCH(k_tfe_final, dim3((unsigned)B), dim3(64), st, (const double *)L.part, stats, out, C);
    return DEFTET_OK;
}

int deftet_tet_field_energies_bwd_f32(const double *stats, const float *grad_out, float target, const float *field, const float *pos,
                                      const int32_t *tet_idx, const int32_t *offsets, const int32_t *slots, float *grad_field,
                                      float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, C = n_channel;
    if (C < 1 || C > kTfeMaxC)
        return set_error(DEFTET_EINVAL, "tet_field_energies_bwd: between 1 and %d channels expected (got %d)", kTfeMaxC, C);
    DEFTET_TRY(tfg_check(B, V, T, C, idx_batch, "tet_field_energies_bwd"));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(stats && grad_out && field && pos && offsets && (T == 0 || (tet_idx && slots)), "tet_field_energies_bwd: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_field_energies_bwd: tet_idx must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (grad_field)
        DEFTET_LAUNCH(k_tfe_bwd_field, dim3(blocks_for((long long)V * C, kTfgBlock), (unsigned)B), dim3(kTfgBlock), st, stats, grad_out, target, field,
                      pos, tet_idx, offsets, slots, grad_field, V, T, C, idx_batch);
    if (grad_pos)
        DEFTET_LAUNCH(k_tfe_bwd_pos, dim3(blocks_for(V, kTfgBlock), (unsigned)B), dim3(kTfgBlock), st, stats, grad_out, target, field, pos, tet_idx,
                      offsets, slots, grad_pos, V, T, C, idx_batch);
    return DEFTET_OK;
}

int deftet_tet_to_vertex_fwd_f32(const float *values, const float *weights, const int32_t *offsets, const int32_t *slots, float *out,
                                 float *weight_sum, float fill, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel,
                                 void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, C = n_channel;
    DEFTET_TRY(tfg_check(B, V, T, C, idx_batch, "tet_to_vertex"));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(offsets && out && weight_sum && (T == 0 || (values && slots)), "tet_to_vertex: null pointer");
    DEFTET_LAUNCH(k_ttv_fwd, dim3(blocks_for((long long)V * C, kTfgBlock), (unsigned)B), dim3(kTfgBlock), as_stream(stream), values, weights, offsets,
                  slots, out, weight_sum, fill, V, T, C, idx_batch);
    return DEFTET_OK;
}

int deftet_tet_to_vertex_bwd_f32(const float *grad_out, const float *weight_sum, const float *weights, const int32_t *tet_idx,
                                 float *grad_values, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, C = n_channel;
    DEFTET_TRY(tfg_check(B, V, T, C, idx_batch, "tet_to_vertex_bwd"));
    if (B == 0 || T == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(tet_idx && grad_values && ((grad_out && weight_sum) || V == 0), "tet_to_vertex_bwd: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_to_vertex_bwd: tet_idx must be 16-byte aligned");
    DEFTET_LAUNCH(k_ttv_bwd, dim3(blocks_for((long long)T * C, kTfgBlock), (unsigned)B), dim3(kTfgBlock), as_stream(stream), grad_out, weight_sum,
                  weights, tet_idx, grad_values, V, T, C, idx_batch);
    return DEFTET_OK;
}

}  // extern "C"
