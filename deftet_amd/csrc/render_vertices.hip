// render_vertices.hip — everything between the image optimiser's per-vertex parameters and the rasterizer's dense per-face
// buffers (3_model/deftet.py:427-468, 3_model/cameraop.py:19-33, 5_rendereq/deftetrneder.py:78-95):
//   project   z, xy, act per vertex from positions, features and a camera        k_project_fwd / k_project_bwd
//   gather    face_z / face_xy / face_feat per face corner through face_idx      k_face_gather_fwd
//   reduce    per-vertex sum of the rasterizer's per-corner gradients            k_face_gather_bwd
// The reduce is the 3-corner twin of vertex_ops.hip's k_gather_bwd: the face list is turned ONCE into a CSR of (face, corner)
// incidences per vertex (vtx::incidence_csr, shared with deftet_tet_vertex_csr_i32) and every component is summed in ascending
// slot order — no atomics, the same bits whatever the launch shape.
#include "common.hpp"

namespace deftet {
namespace rv {

// The camera of one view in fp64, and cam = R (p - c) with every row summed left to right — the operations and the order of
// `perspective`, evaluated in fp64 and rounded once per output.  Why not an fp32 chain: near the image centre cam.x and cam.y are
// differences of terms ~|p - c|, and an fp32 chain leaves them (and the gradients, which cancel the same way) with 3e-5..5e-5
// relative error on entries above 1e-3 of the maximum — outside the 1e-5 element-relative bound the outputs are held to.
struct Camera {
    double R[9], c[3], p[3];
    __device__ Camera(const float *rot, const float *camPos, const float *proj, int b)
    {
        for (int i = 0; i < 9; ++i) R[i] = rot[(size_t)b * 9 + i];
        for (int i = 0; i < 3; ++i) { c[i] = camPos[(size_t)b * 3 + i]; p[i] = proj[i]; }
    }
    __device__ void to_camera(const float *pos, double cam[3]) const
    {
        const double d0 = pos[0] - c[0], d1 = pos[1] - c[1], d2 = pos[2] - c[2];
        for (int i = 0; i < 3; ++i) cam[i] = (d0 * R[3 * i] + d1 * R[3 * i + 1]) + d2 * R[3 * i + 2];
    }
};

// One lane per (view, vertex): z = cam.z; xy = (cam.x px, cam.y py) / (cam.z pz) * mult; act = sigmoid(feat), behind cam.z as
// channel 0 when depthChannel.  Shared positions / features (batch 1) are read by every view.
__global__ __launch_bounds__(256) void k_project_fwd(const float *__restrict__ pos, const float *__restrict__ feat,
                                                     const float *__restrict__ rot, const float *__restrict__ camPos,
                                                     const float *__restrict__ proj, float mult, int depthChannel, float *z, float *xy,
                                                     float *act, int V, int D, int posBatch, int featBatch)
{
    const int b = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const Camera cam(rot, camPos, proj, b);
    double c[3];
    cam.to_camera(pos + ((posBatch > 1 ? (size_t)b * V : 0) + v) * 3, c);
    const double den = c[2] * cam.p[2];
    const size_t row = (size_t)b * V + v;
    z[row] = (float)c[2];
    xy[row * 2] = (float)((c[0] * cam.p[0]) / den * (double)mult);
    xy[row * 2 + 1] = (float)((c[1] * cam.p[1]) / den * (double)mult);
    const int Do = D + (depthChannel ? 1 : 0);
    float *a = act + row * Do;
    if (depthChannel) *a++ = (float)c[2];
    const float *f = feat + ((featBatch > 1 ? (size_t)b * V : 0) + v) * D;
    for (int k = 0; k < D; ++k) a[k] = (float)(1.0 / (1.0 + exp(-(double)f[k])));
}

// d pos of one (view, vertex), recomputed from the position (the saved fp32 outputs would carry their rounding into the
// cancelling sums): d xy.x / d cam.x = px mult / (cam.z pz), d xy / d cam.z = -xy / cam.z; cam.z itself gets a gradient through the
// depth channel alone (the rasterizer gives none to face_z).  Then R^T, left to right.
__device__ __forceinline__ void project_bwd_one(const float *gxy, const float *gact, const float *pos, const Camera &cam, double mult,
                                                int depthChannel, int Do, size_t row, double g[3])
{
    double c[3];
    cam.to_camera(pos, c);
    const double den = c[2] * cam.p[2];
    const double gx = gxy ? (double)gxy[row * 2] : 0.0, gy = gxy ? (double)gxy[row * 2 + 1] : 0.0;
    const double sx = cam.p[0] * mult / den, sy = cam.p[1] * mult / den;
    const double gcx = gx * sx, gcy = gy * sy;
    double gcz = -((gcx * c[0] + gcy * c[1]) / c[2]);
    if (depthChannel && gact) gcz += (double)gact[row * Do];
    for (int j = 0; j < 3; ++j) g[j] = (cam.R[j] * gcx + cam.R[3 + j] * gcy) + cam.R[6 + j] * gcz;
}

// d sigmoid(x) / dx = e / (1 + e)^2 with e = exp(-|x|): no 1 - a of a rounded a
__device__ __forceinline__ double dsigmoid(float x)
{
    const double e = exp(-fabs((double)x));
    return e / ((1.0 + e) * (1.0 + e));
}

// One lane per (view, vertex).  A per-view input writes its own row; a shared one (batch 1) is summed over the views in
// ascending b by the lanes of view 0 (the lanes of the other views then have nothing to do for it).
__global__ __launch_bounds__(256) void k_project_bwd(const float *__restrict__ gxy, const float *__restrict__ gact,
                                                     const float *__restrict__ pos, const float *__restrict__ feat,
                                                     const float *__restrict__ rot, const float *__restrict__ camPos,
                                                     const float *__restrict__ proj, float mult, int depthChannel, float *gradPos,
                                                     float *gradFeat, int B, int V, int D, int posBatch, int featBatch)
{
    const int b = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int o = depthChannel ? 1 : 0, Do = D + o;
    if (gradPos) {
        if (posBatch > 1) {
            double g[3];
            const size_t row = (size_t)b * V + v;
            project_bwd_one(gxy, gact, pos + row * 3, Camera(rot, camPos, proj, b), mult, depthChannel, Do, row, g);
            gradPos[row * 3] = (float)g[0]; gradPos[row * 3 + 1] = (float)g[1]; gradPos[row * 3 + 2] = (float)g[2];
        } else if (b == 0) {
            double s[3] = {0.0, 0.0, 0.0};
            for (int bb = 0; bb < B; ++bb) {
                double g[3];
                project_bwd_one(gxy, gact, pos + (size_t)v * 3, Camera(rot, camPos, proj, bb), mult, depthChannel, Do, (size_t)bb * V + v, g);
                s[0] += g[0]; s[1] += g[1]; s[2] += g[2];
            }
            gradPos[(size_t)v * 3] = (float)s[0]; gradPos[(size_t)v * 3 + 1] = (float)s[1]; gradPos[(size_t)v * 3 + 2] = (float)s[2];
        }
    }
    if (gradFeat) {
        if (featBatch > 1) {
            const size_t row = (size_t)b * V + v;
            for (int k = 0; k < D; ++k)
                gradFeat[row * D + k] = gact ? (float)((double)gact[row * Do + o + k] * dsigmoid(feat[row * D + k])) : 0.f;
        } else if (b == 0) {
            for (int k = 0; k < D; ++k) {
                const double ds = dsigmoid(feat[(size_t)v * D + k]);
                double s = 0.0;
                for (int bb = 0; bb < B && gact; ++bb) s += (double)gact[((size_t)bb * V + v) * Do + o + k] * ds;
                gradFeat[(size_t)v * D + k] = (float)s;
            }
        }
    }
}

// One launch for the three per-face arrays; every lane owns one output element (a z, an xy pair or one feature of one corner),
// so consecutive lanes store consecutive addresses.  Per view the element space is [0,3F) z, [3F,6F) xy pairs, [6F,6F+3F*Do)
// features; the lanes of one corner read the same index (a broadcast) and neighbouring floats of one vertex row.
__global__ __launch_bounds__(256) void k_face_gather_fwd(const float *__restrict__ z, const float *__restrict__ xy,
                                                         const float *__restrict__ act, const int64_t *__restrict__ idx, float *faceZ,
                                                         float *faceXy, float *faceFeat, int V, long long n3, int Do, int *bad)
{
    const int b = blockIdx.y;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3 * (2 + Do)) return;
    long long j;                                             // corner 3 f + k
    int seg, ch = 0;
    if (e < n3) { seg = 0; j = e; }
    else if (e < 2 * n3) { seg = 1; j = e - n3; }
    else { seg = 2; j = (e - 2 * n3) / Do; ch = (int)((e - 2 * n3) - j * Do); }
    const long long vi = idx[j];
    const bool ok = vi >= 0 && vi < V;                       // torch indexing raises; here: NaN + flag, as k_gather_fwd
    if (!ok && bad) *bad = 1;
    const size_t src = (size_t)b * V + (ok ? vi : 0), dst = (size_t)b * n3 + j;
    if (seg == 0) faceZ[dst] = ok ? z[src] : quiet_nan();
    else if (seg == 1) {
        float2 val = make_float2(quiet_nan(), quiet_nan());
        if (ok) val = *reinterpret_cast<const float2 *>(xy + src * 2);
        *reinterpret_cast<float2 *>(faceXy + dst * 2) = val;
    } else faceFeat[dst * Do + ch] = ok ? act[src * Do + ch] : quiet_nan();
}

// One lane per (view, vertex, component): components 0,1 are xy, 2.. the Do feature channels, so the lanes of a vertex read
// neighbouring floats of the same corner rows.  The order contract fixes the additions — one fp32 accumulator per component,
// incidences added one after the other in slot order — not the loads: four incidences are in flight per lane (slot -> row is a
// chain of two loads; a Kuhn interior vertex has 36 incidences).  Any degree takes the same loop.  A null gradient is zeros.
__global__ __launch_bounds__(256) void k_face_gather_bwd(const float *__restrict__ gFaceXy, const float *__restrict__ gFaceFeat,
                                                         const int *__restrict__ offsets, const int *__restrict__ slots, float *gXy,
                                                         float *gAct, int V, long long n3, int Do)
{
    const int b = blockIdx.y;
    const int C = 2 + Do;
    // every XCD (workgroup i runs on XCD i % 8) takes a contiguous eighth of the vertex range: speed only (k_gather_bwd)
    const long long per = gridDim.x >> 3, wg = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    const long long gid = wg * blockDim.x + threadIdx.x;
    if (gid >= (long long)V * C) return;
    const int v = (int)(gid / C), c = (int)(gid - (long long)v * C);
    const float *src = c < 2 ? gFaceXy : gFaceFeat;
    const int stride = c < 2 ? 2 : Do, ch = c < 2 ? c : c - 2;
    float acc = 0.f;
    if (src) {
        src += (size_t)b * n3 * stride + ch;
        const int s1 = offsets[v + 1];
        int i = offsets[v];
        for (; i + 3 < s1; i += 4) {
            const int t0 = slots[i], t1 = slots[i + 1], t2 = slots[i + 2], t3 = slots[i + 3];
            const float r0 = src[(size_t)t0 * stride], r1 = src[(size_t)t1 * stride], r2 = src[(size_t)t2 * stride],
                        r3 = src[(size_t)t3 * stride];
            acc += r0; acc += r1; acc += r2; acc += r3;
        }
        for (; i < s1; ++i) acc += src[(size_t)slots[i] * stride];
    }
    const size_t row = (size_t)b * V + v;
    if (c < 2) gXy[row * 2 + c] = acc;
    else gAct[row * Do + ch] = acc;
}

}  // namespace rv
}  // namespace deftet

using namespace deftet;

extern "C" size_t deftet_face_vertex_csr_workspace_bytes(int V, int F) { return vtx::incidence_csr_workspace_bytes(1, V, F, 3); }

extern "C" int deftet_face_vertex_csr_i32(const int64_t *face_idx, int32_t *offsets, int32_t *slots, int32_t *bad_flag, int V, int F,
                                          void *workspace, size_t workspace_bytes, void *stream_)
{
    return vtx::incidence_csr(face_idx, offsets, slots, bad_flag, 1, V, F, 3, workspace, workspace_bytes, as_stream(stream_));
}

static int check_project_sizes(int B, int V, int D, int pos_batch, int feat_batch)
{
    DEFTET_CHECK_ARG(B >= 0 && V >= 0 && D >= 1, "n_batch / n_vertex negative or n_feat < 1");
    DEFTET_CHECK_ARG(B <= 65535, "n_batch=%d exceeds 65535", B);
    DEFTET_CHECK_ARG(pos_batch == 1 || pos_batch == B, "pos batch must be 1 or n_batch (got %d)", pos_batch);
    DEFTET_CHECK_ARG(feat_batch == 1 || feat_batch == B, "feat batch must be 1 or n_batch (got %d)", feat_batch);
    return DEFTET_OK;
}

extern "C" int deftet_project_vertices_fwd_f32(const float *pos, const float *feat, const float *rot, const float *cam_pos,
                                               const float *proj, float multiplier, int depth_channel, float *z, float *xy, float *act,
                                               int B, int V, int D, int pos_batch, int feat_batch, void *stream_)
{
    DEFTET_TRY(check_project_sizes(B, V, D, pos_batch, feat_batch));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(pos && feat && rot && cam_pos && proj && z && xy && act, "null pointer");
    DEFTET_LAUNCH(rv::k_project_fwd, dim3(blocks_for(V, 256), B), dim3(256), as_stream(stream_), pos, feat, rot, cam_pos, proj, multiplier,
                  depth_channel ? 1 : 0, z, xy, act, V, D, pos_batch, feat_batch);
    return DEFTET_OK;
}

extern "C" int deftet_project_vertices_bwd_f32(const float *g_xy, const float *g_act, const float *pos, const float *feat, const float *rot,
                                               const float *cam_pos, const float *proj, float multiplier, int depth_channel,
                                               float *grad_pos, float *grad_feat, int B, int V, int D, int pos_batch, int feat_batch,
                                               void *stream_)
{
    DEFTET_TRY(check_project_sizes(B, V, D, pos_batch, feat_batch));
    if (B == 0 || V == 0 || (!grad_pos && !grad_feat)) return DEFTET_OK;
    DEFTET_CHECK_ARG(pos && feat && rot && cam_pos && proj, "null pointer");
    DEFTET_LAUNCH(rv::k_project_bwd, dim3(blocks_for(V, 256), B), dim3(256), as_stream(stream_), g_xy, g_act, pos, feat, rot, cam_pos, proj,
                  multiplier, depth_channel ? 1 : 0, grad_pos, grad_feat, B, V, D, pos_batch, feat_batch);
    return DEFTET_OK;
}

static int check_gather_sizes(int B, int V, int F, int Do)
{
    DEFTET_CHECK_ARG(B >= 0 && V >= 0 && F >= 0 && Do >= 1, "negative size or no feature channel");
    DEFTET_CHECK_ARG(B <= 65535, "n_batch=%d exceeds 65535", B);
    DEFTET_CHECK_ARG(((long long)3 * F * (2 + Do) + 255) / 256 < 0x7FFFFFFFLL && ((long long)V * (2 + Do) + 255) / 256 + 8 < 0x7FFFFFFFLL &&
                         (long long)3 * F < 0x7FFFFFFFLL,
                     "face list too large");
    return DEFTET_OK;
}

extern "C" int deftet_face_gather_fwd_f32(const float *z, const float *xy, const float *act, const int64_t *face_idx, float *face_z,
                                          float *face_xy, float *face_feat, int32_t *bad_flag, int B, int V, int F, int Do, void *stream_)
{
    DEFTET_TRY(check_gather_sizes(B, V, F, Do));
    if (B == 0 || F == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(face_idx && face_z && face_xy && face_feat && (V == 0 || (z && xy && act)), "null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)xy & 7) == 0 && ((uintptr_t)face_xy & 7) == 0, "xy/face_xy must be 8-byte aligned");
    const long long n3 = (long long)3 * F;
    DEFTET_LAUNCH(rv::k_face_gather_fwd, dim3(blocks_for(n3 * (2 + Do), 256), B), dim3(256), as_stream(stream_), z, xy, act,
                  face_idx, face_z, face_xy, face_feat, V, n3, Do, bad_flag);
    return DEFTET_OK;
}

extern "C" int deftet_face_gather_bwd_f32(const float *grad_face_xy, const float *grad_face_feat, const int32_t *offsets,
                                          const int32_t *slots, float *g_xy, float *g_act, int B, int V, int F, int Do, void *stream_)
{
    DEFTET_TRY(check_gather_sizes(B, V, F, Do));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(offsets && g_xy && g_act && (F == 0 || slots), "null pointer");
    const unsigned wgs = (unsigned)align_up(blocks_for((long long)V * (2 + Do), 256), 8);
    DEFTET_LAUNCH(rv::k_face_gather_bwd, dim3(wgs, B), dim3(256), as_stream(stream_), grad_face_xy, grad_face_feat, offsets, slots, g_xy,
                  g_act, V, (long long)3 * F, Do);
    return DEFTET_OK;
}
