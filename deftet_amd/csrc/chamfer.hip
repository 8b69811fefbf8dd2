// chamfer.hip — the chamfer term of the surface loss for CDNA4 / gfx950:
// layers/DefTet/deftet.py:174-177 composed (utils/mesh_utils.py:290-299, :360-374): K area-uniform samples per predicted
// face, each measured against its nearest ground-truth point (operator A10).  As torch expressions these are ~45 small
// launches per step (forward and backward); here: one to place the samples, one for the distances, one for the gradient.
#pragma clang fp contract(off)
#include "common.hpp"

namespace deftet {
namespace surf {

constexpr float kChamferEps = 1e-10f;   // inside the square root (utils/mesh_utils.py:14)

// samples f32 [B, F*K, 3]: sample j of face f in row f*K + j = wa*a + wb*b + wc*c with s = sqrt(r0), wa = 1 - s,
// wb = s (1 - r1), wc = s r1 (square-root warp of two uniform numbers r f32 [2, B, F, K])
__global__ __launch_bounds__(256) void k_face_samples(const float *__restrict__ tri, const float *__restrict__ r, float *samples, int K,
                                                      long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float *t = tri + (i / K) * 9;
    const float s = sqrtf(r[i]), r1 = r[total + i];
    const float wa = 1.0f - s, wb = s * (1.0f - r1), wc = s * r1;
#pragma unroll
    for (int k = 0; k < 3; ++k) samples[i * 3 + k] = (wa * t[k] + wb * t[3 + k]) + wc * t[6 + k];
}

// d f32 [B,N] = sqrt(|sample - gt[idx]|^2 + eps) for the first n_valid[b] rows of shape b, 0 beyond
__global__ __launch_bounds__(256) void k_chamfer_fwd(const float *__restrict__ samples, const float *__restrict__ gt,
                                                     const int *__restrict__ idx, const int *__restrict__ n_valid, float *d, int N, int M)
{
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const size_t i = (size_t)b * N + j;
    float v = 0.f;
    if (j < n_valid[b]) {
        const float *sp = samples + i * 3, *g = gt + ((size_t)b * M + idx[i]) * 3;
        const float dx = sp[0] - g[0], dy = sp[1] - g[1], dz = sp[2] - g[2];
        v = sqrtf(((dx * dx + dy * dy) + dz * dz) + kChamferEps);
    }
    d[i] = v;
}

// grad_tri f32 [B,F,3,3]: one lane per face adds up its K samples' gradients (no atomics); gscale f32 [B] = dL/d(sum of d)
__global__ __launch_bounds__(256) void k_chamfer_bwd(const float *__restrict__ samples, const float *__restrict__ gt,
                                                     const int *__restrict__ idx, const int *__restrict__ n_valid,
                                                     const float *__restrict__ d, const float *__restrict__ r,
                                                     const float *__restrict__ gscale, float *grad_tri, int F, int K, int M, long long total)
{
    const int b = blockIdx.y;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f};
    const int N = F * K;
    const float gs = gscale[b];
    for (int j = 0; j < K; ++j) {
        const int row = f * K + j;
        if (row >= n_valid[b]) break;
        const size_t i = (size_t)b * N + row;
        const float *sp = samples + i * 3, *g = gt + ((size_t)b * M + idx[i]) * 3;
        const float s = sqrtf(r[i]), r1 = r[total + i];
        const float wa = 1.0f - s, wb = s * (1.0f - r1), wc = s * r1;
        const float w = gs / d[i];                                     // d(sqrt(q + eps))/d(sample) = (sample - near) / d
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gk = w * (sp[k] - g[k]);
            ga[k] += wa * gk; gb[k] += wb * gk; gc[k] += wc * gk;
        }
    }
    float *o = grad_tri + ((size_t)b * F + f) * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = ga[k]; o[3 + k] = gb[k]; o[6 + k] = gc[k]; }
}

}  // namespace surf
}  // namespace deftet

using namespace deftet;
using namespace deftet::surf;

extern "C" int deftet_face_samples_f32(const float *tri, const float *r, float *samples, int B, int F, int K, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && F >= 0 && K >= 1, "bad size");
    const long long total = (long long)B * F * K;
    if (total == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(tri && r && samples, "null pointer");
    DEFTET_CHECK_ARG(total * 3 < (1LL << 40), "too many samples");
    DEFTET_LAUNCH(k_face_samples, dim3(blocks_for(total, 256)), dim3(256), as_stream(stream_), tri, r, samples, K, total);
    return DEFTET_OK;
}

extern "C" int deftet_chamfer_fwd_f32(const float *samples, const float *gt, const int32_t *idx, const int32_t *n_valid, float *d, int B,
                                      int N, int M, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && N >= 0 && M >= 1 && B <= 65535, "bad size");
    if (B == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(samples && gt && idx && n_valid && d, "null pointer");
    DEFTET_LAUNCH(k_chamfer_fwd, dim3(blocks_for(N, 256), B), dim3(256), as_stream(stream_), samples, gt, idx, n_valid, d, N, M);
    return DEFTET_OK;
}

extern "C" int deftet_chamfer_bwd_f32(const float *samples, const float *gt, const int32_t *idx, const int32_t *n_valid, const float *d,
                                      const float *r, const float *gscale, float *grad_tri, int B, int F, int K, int M, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && F >= 0 && K >= 1 && M >= 1 && B <= 65535, "bad size");
    if (B == 0 || F == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(samples && gt && idx && n_valid && d && r && gscale && grad_tri, "null pointer");
    DEFTET_LAUNCH(k_chamfer_bwd, dim3(blocks_for(F, 256), B), dim3(256), as_stream(stream_), samples, gt, idx, n_valid, d, r, gscale, grad_tri, F, K,
                  M, (long long)B * F * K);
    return DEFTET_OK;
}
