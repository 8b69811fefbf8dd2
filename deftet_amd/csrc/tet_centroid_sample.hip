// tet_centroid_sample.hip — the input of the occupancy decoder straight from the vertices:
//   occ_feature = cat(sample_f(mean(gather(pos, tets), 2)[:, chosen], volumes), centroids^T)      layers/pc_model.py:276-306
// computed from (vertice_pos, tet list, chosen tets, volumes) without anything of size O(T 4 3): one forward launch for the whole
// volume list, one launch for the gradient on the centroids, one for the gradient on the vertices.  The volumes' gradient is
// pointvoxel.hip's (deftet_voxel_cells_f32 + deftet_voxel_sample_bwd_vol_f32 on the centroids this forward writes).
// No float atomics; every sum has one order:
//   centroid      ((a + b) + c) + d, then * 0.25f, every step rounded, per coordinate, corners 0,1,2,3
//   value         pointvoxel.hpp's: u = clamp((cent + 0.5) r, 0, r - 1), eight rounded products added in corner order 000 .. 111
//   to centroids  per volume the channel sum from 0 in ascending order (pos_grad_of_volume), the volumes' results added in list
//                 order, the position row of grad_out last
//   to vertices   gpos[b,v] = 0.25f * sum over the incidences (4 t + corner, ascending) of v, over the slots that chose t in
//                 ascending slot, of gcent[b,slot]: one accumulator from 0, one product at the end
#include "cell_gather.hpp"                      // the sort plumbing
#include "pointvoxel.hpp"                       // the trilinear arithmetic

namespace deftet {
namespace {

constexpr int kTcsMaxVol = 8;                                       // volumes per call (the encoder hands four)
constexpr int kTcsMaxChunk = 64;                                    // (volume, channel range) rows of the forward's table

// the volume list and the table a forward workgroup finds its (volume, channel range) in, both by value in the kernel arguments
struct TcsVolumes {
    const float *vol[kTcsMaxVol];
    int C[kTcsMaxVol], R[kTcsMaxVol], c_off[kTcsMaxVol];
    int n;
};
struct TcsChunks {
    int c0[kTcsMaxChunk], c1[kTcsMaxChunk];
    unsigned char vol[kTcsMaxChunk];
};

// the centroid of slot j of shape b; false (and NaNs) for a tet index outside [0,T) or a vertex index outside [0,V)
__device__ __forceinline__ bool centroid_of(const float *__restrict__ pos, const int32_t *__restrict__ tet_idx,
                                            const int32_t *__restrict__ select, int first, int b, int j, int V, int T, int idx_batch,
                                            float cent[3])
{
    cent[0] = cent[1] = cent[2] = quiet_nan();
    const int t = select ? select[j] : first + j;
    if (t < 0 || t >= T) return false;
    const int4 vi = *reinterpret_cast<const int4 *>(tet_idx + ((idx_batch > 1 ? (size_t)b * T : 0) + t) * 4);
    if ((unsigned)vi.x >= (unsigned)V || (unsigned)vi.y >= (unsigned)V || (unsigned)vi.z >= (unsigned)V || (unsigned)vi.w >= (unsigned)V)
        return false;
    const float *p = pos + (size_t)b * V * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        cent[k] = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(p[(size_t)vi.x * 3 + k], p[(size_t)vi.y * 3 + k]), p[(size_t)vi.z * 3 + k]),
                                      p[(size_t)vi.w * 3 + k]), 0.25f);
    return true;
}

// grid (slots / 256, table rows, B): a workgroup is uniform in (volume, channel range), its lanes are consecutive slots
__global__ __launch_bounds__(kPvBlock) void k_tcs_fwd(TcsVolumes vv, TcsChunks ch, const float *__restrict__ pos,
                                                      const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ select, int first,
                                                      float *out, float *centroids, int32_t *bad, int V, int T, int K, int idx_batch,
                                                      int C_feat, int C_total)
{
    const int j = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.z;
    if (j >= K) return;
    float cent[3];
    const bool ok = centroid_of(pos, tet_idx, select, first, b, j, V, T, idx_batch, cent);
    if (blockIdx.y == 0) {                                           // the first row of the table also writes what no volume owns
        if (!ok && bad) *bad = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            centroids[((size_t)b * K + j) * 3 + k] = cent[k];
            if (C_total > C_feat) out[((size_t)b * C_total + C_feat + k) * K + j] = cent[k];
        }
    }
    const int k = ch.vol[blockIdx.y], c0 = ch.c0[blockIdx.y], c1 = ch.c1[blockIdx.y];
    if (c0 >= c1) return;
    const int C = vv.C[k], R = vv.R[k];
    float *o = out + ((size_t)b * C_total + vv.c_off[k]) * K + j;
    if (!ok) {
        for (int c = c0; c < c1; ++c) o[(size_t)c * K] = quiet_nan();
        return;
    }
    float raw[3], u[3];
    load_u(cent, 0, 0, 0, 1, R, raw, u);                             // the rounded centroid as a point set of one
    Corners cn;
    corners_of(u, R, false, cn);
    const size_t R3 = (size_t)R * R * R;
    const float *f = vv.vol[k] + ((size_t)b * C + c0) * R3;
    for (int c = c0; c < c1; ++c, f += R3) o[(size_t)c * K] = sample_corners(f, cn);
}

// grid (slots / 64, B), block (64, volumes): wave y sums volume y's channels for 64 consecutive slots; wave 0 then adds the
// volumes' results in list order and the position row last.  A NaN centroid (a slot the forward refused) gets 0.
__global__ __launch_bounds__(64 * kTcsMaxVol) void k_tcs_bwd_pos(TcsVolumes vv, const float *__restrict__ centroids,
                                                                 const float *__restrict__ gout, float *gcent, int K, int C_feat,
                                                                 int C_total)
{
    __shared__ float part[kTcsMaxVol][3][64];
    const int j = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    const int k = __builtin_amdgcn_readfirstlane((int)threadIdx.y);      // a wave is one row of the block: uniform, so the list is read by scalar loads
    const bool in = j < K;
    if (in && k < vv.n) {
        float raw[3], u[3], res[3];
        load_u(centroids, 0, b, j, K, vv.R[k], raw, u);
        pos_grad_of_volume(vv.vol[k], gout, raw, u, b, j, vv.C[k], vv.R[k], K, vv.c_off[k], C_total, 0, res);
#pragma unroll
        for (int a = 0; a < 3; ++a) part[k][a][threadIdx.x] = res[a];
    }
    __syncthreads();
    if (k != 0 || !in) return;
    const float *c = centroids + ((size_t)b * K + j) * 3;
    const bool good = c[0] == c[0] && c[1] == c[1] && c[2] == c[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float g = vv.n > 0 ? part[0][a][threadIdx.x] : 0.0f;
        for (int q = 1; q < vv.n; ++q) g = g + part[q][a][threadIdx.x];
        if (C_total > C_feat) g += gout[((size_t)b * C_total + C_feat + a) * K + j];
        gcent[((size_t)b * K + j) * 3 + a] = good ? g : 0.0f;
    }
}

// the chosen tet of every slot as a sort key; an index outside [0,T) takes the sentinel T and lands in no tet's segment
__global__ __launch_bounds__(kPvBlock) void k_tcs_keys(const int32_t *__restrict__ select, unsigned *keys, int K, int T)
{
    const int j = blockIdx.x * kPvBlock + threadIdx.x;
    if (j >= K) return;
    const int t = select[j];
    keys[j] = t >= 0 && t < T ? (unsigned)t : (unsigned)T;
}

// one thread per (shape, vertex): its incidences in CSR order, per incidence the slots of that tet in ascending slot (seg / perm
// from the stable sort of the keys above; without a selection the one slot t - first), one accumulator, one product at the end
__global__ __launch_bounds__(kPvBlock) void k_tcs_bwd_vertices(const float *__restrict__ gcent, const int32_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ slots, const int32_t *__restrict__ seg,
                                                               const int32_t *__restrict__ perm, int first, float *gpos, int V, int K,
                                                               int idx_batch, int accumulate)
{
    const int v = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (v >= V) return;
    const size_t row = (idx_batch > 1 ? (size_t)b * V : 0) + v;
    const int i0 = offsets[row], i1 = offsets[row + 1];
    const float *g = gcent + (size_t)b * K * 3;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (int i = i0; i < i1; ++i) {
        const int t = slots[i] >> 2;
        if (seg) {
            const int q1 = seg[t + 1];
            for (int q = seg[t]; q < q1; ++q) {
                const float *p = g + (size_t)perm[q] * 3;
                ax = __fadd_rn(ax, p[0]);
                ay = __fadd_rn(ay, p[1]);
                az = __fadd_rn(az, p[2]);
            }
        } else {
            const int j = t - first;
            if (j >= 0 && j < K) {
                const float *p = g + (size_t)j * 3;
                ax = __fadd_rn(ax, p[0]);
                ay = __fadd_rn(ay, p[1]);
                az = __fadd_rn(az, p[2]);
            }
        }
    }
    float *o = gpos + ((size_t)b * V + v) * 3;
    const float rx = __fmul_rn(0.25f, ax), ry = __fmul_rn(0.25f, ay), rz = __fmul_rn(0.25f, az);
    o[0] = accumulate ? __fadd_rn(o[0], rx) : rx;
    o[1] = accumulate ? __fadd_rn(o[1], ry) : ry;
    o[2] = accumulate ? __fadd_rn(o[2], rz) : rz;
}

// the workspace of the backward to the vertices: the sort of the K chosen tets, the slots in tet order and the table seg[T + 1]
struct TcsLayout {
    size_t bytes;
    SortBufs s;
    int32_t *perm, *seg;
};
TcsLayout tcs_layout(size_t T, size_t K, void *ws)
{
    TcsLayout L{};
    Arena A(ws);
    take_sort(A, K, L.s);
    L.perm = A.take<int32_t>(K);
    L.seg = A.take<int32_t>(T + 1);
    L.bytes = A.end();
    return L;
}

int check_volumes(const float *const *vols, const int *channels, const int *resolutions, int n_vol, int B, bool need_ptr,
                  TcsVolumes &vv, int &C_feat, const char *what)
{
    if (n_vol < 0 || n_vol > kTcsMaxVol) return set_error(DEFTET_EINVAL, "%s: between 0 and %d volumes expected (got %d)", what, kTcsMaxVol, n_vol);
    if (n_vol > 0 && (!channels || !resolutions || !vols)) return set_error(DEFTET_EINVAL, "%s: null volume list", what);
    vv.n = n_vol;
    long long c_off = 0;
    for (int k = 0; k < n_vol; ++k) {
        const long long C = channels[k], R = resolutions[k];
        if (C < 0 || R < 1) return set_error(DEFTET_EINVAL, "%s: volume %d has a negative channel count or a resolution below 1", what, k);
        if (R * R * R * (long long)(B > 0 ? B : 1) >= 0x7FFFFFFFll) return set_error(DEFTET_ELIMIT, "%s: B R^3 does not fit 31 bits", what);
        if (need_ptr && C > 0 && !vols[k]) return set_error(DEFTET_EINVAL, "%s: null volume pointer", what);
        vv.vol[k] = vols[k];
        vv.C[k] = (int)C;
        vv.R[k] = (int)R;
        vv.c_off[k] = (int)c_off;
        c_off += C;
        if (c_off >= 0x7FFFFFFFll) return set_error(DEFTET_ELIMIT, "%s: too many channels", what);
    }
    C_feat = (int)c_off;
    return DEFTET_OK;
}

int check_mesh(int B, int V, int T, int K, int idx_batch, const int32_t *select, int first, const char *what)
{
    if (B < 0 || V < 0 || T < 0 || K < 0) return set_error(DEFTET_EINVAL, "%s: negative size", what);
    if (B > 65535) return set_error(DEFTET_ELIMIT, "%s: more than 65535 shapes", what);
    if (idx_batch != 1 && idx_batch != B) return set_error(DEFTET_EINVAL, "%s: tet list batch must be 1 or n_batch (got %d)", what, idx_batch);
    if (!select && (first < 0 || (long long)first + K > T))
        return set_error(DEFTET_EINVAL, "%s: the range first + n_slot = %lld exceeds the %d tets", what, (long long)first + K, T);
    if ((long long)B * V >= 0x7FFFFFFFll || (long long)B * K >= 0x7FFFFFFFll || (long long)idx_batch * T * 4 >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: B V, B K or 4 T does not fit 31 bits", what);
    return DEFTET_OK;
}

}  // namespace
}  // namespace deftet

using namespace deftet;

extern "C" {

size_t deftet_tet_centroid_sample_workspace_bytes(int n_batch, int n_tet, int n_slot)
{
    if (n_batch < 0 || n_tet < 0 || n_slot < 0) return 0;
    return tcs_layout((size_t)n_tet, (size_t)n_slot, nullptr).bytes;    // (the selection is shared by the batch: no factor n_batch)
}

int deftet_tet_centroid_sample_fwd_f32(const float *const *vols, const int *channels, const int *resolutions, int n_vol, const float *pos,
                                       const int32_t *tet_idx, const int32_t *select, int first, float *out, float *centroids,
                                       int32_t *bad_flag, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_slot, int append_pos,
                                       void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, K = n_slot;
    TcsVolumes vv{};
    int C_feat = 0;
    DEFTET_TRY(check_volumes(vols, channels, resolutions, n_vol, B, B > 0 && K > 0, vv, C_feat, "tet_centroid_sample"));
    DEFTET_TRY(check_mesh(B, V, T, K, idx_batch, select, first, "tet_centroid_sample"));
    if (B == 0 || K == 0) return DEFTET_OK;
    const int C_total = C_feat + (append_pos ? 3 : 0);
    DEFTET_CHECK_ARG(pos && tet_idx && centroids && (out || C_total == 0), "tet_centroid_sample: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_centroid_sample: tet_idx must be 16-byte aligned");
    const unsigned gK = blocks_for(K, kPvBlock);
    // channels per table row: a few thousand workgroups, and no more rows than the table holds
    int c_per = C_feat > 0 ? channels_per_thread(C_feat, (long long)gK * B) : 1;
    const int c_min = (C_feat + (kTcsMaxChunk - kTcsMaxVol) - 1) / (kTcsMaxChunk - kTcsMaxVol);
    if (c_per < c_min) c_per = c_min;
    TcsChunks ch{};
    int rows = 0;
    for (int k = 0; k < n_vol; ++k)
        for (int c0 = 0; c0 < vv.C[k]; c0 += c_per, ++rows) {
            ch.vol[rows] = (unsigned char)k;
            ch.c0[rows] = c0;
            ch.c1[rows] = c0 + c_per < vv.C[k] ? c0 + c_per : vv.C[k];
        }
    if (rows == 0) rows = 1;                                         // no channel at all: one empty row writes the centroids
    DEFTET_LAUNCH(k_tcs_fwd, dim3(gK, (unsigned)rows, (unsigned)B), dim3(kPvBlock), as_stream(stream), vv, ch, pos, tet_idx, select, first,
                  out, centroids, bad_flag, V, T, K, idx_batch, C_feat, C_total);
    return DEFTET_OK;
}

int deftet_tet_centroid_sample_bwd_pos_f32(const float *const *vols, const int *channels, const int *resolutions, int n_vol,
                                           const float *centroids, const float *grad_out, float *grad_cent, int n_batch, int n_slot,
                                           int append_pos, void *stream)
{
    const int B = n_batch, K = n_slot;
    TcsVolumes vv{};
    int C_feat = 0;
    DEFTET_TRY(check_volumes(vols, channels, resolutions, n_vol, B, B > 0 && K > 0, vv, C_feat, "tet_centroid_sample_bwd_pos"));
    DEFTET_CHECK_ARG(B >= 0 && K >= 0, "tet_centroid_sample_bwd_pos: negative size");
    if (B > 65535 || (long long)B * K >= 0x7FFFFFFFll) return set_error(DEFTET_ELIMIT, "tet_centroid_sample_bwd_pos: more than 65535 shapes or B K past 31 bits");
    if (B == 0 || K == 0) return DEFTET_OK;
    const int C_total = C_feat + (append_pos ? 3 : 0);
    DEFTET_CHECK_ARG(centroids && grad_cent && (grad_out || C_total == 0), "tet_centroid_sample_bwd_pos: null pointer");
    DEFTET_LAUNCH(k_tcs_bwd_pos, dim3(blocks_for(K, 64), (unsigned)B), dim3(64, (unsigned)(n_vol > 0 ? n_vol : 1)), as_stream(stream), vv,
                  centroids, grad_out, grad_cent, K, C_feat, C_total);
    return DEFTET_OK;
}

int deftet_tet_centroid_sample_bwd_vertices_f32(const float *grad_cent, const int32_t *offsets, const int32_t *slots, const int32_t *select,
                                                int first, float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_slot,
                                                int accumulate, void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet, K = n_slot;
    DEFTET_TRY(check_mesh(B, V, T, K, idx_batch, select, first, "tet_centroid_sample_bwd_vertices"));
    const bool sorted = select != nullptr && K > 0;
    const TcsLayout L = tcs_layout((size_t)T, (size_t)K, workspace);
    if (sorted) DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    if (B == 0 || V == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(offsets && grad_pos && (T == 0 || slots) && (K == 0 || grad_cent), "tet_centroid_sample_bwd_vertices: null pointer");
    hipStream_t st = as_stream(stream);
    if (sorted) {
        DEFTET_LAUNCH(k_tcs_keys, dim3(blocks_for(K, kPvBlock)), dim3(kPvBlock), st, select, L.s.keys, K, T);
        DEFTET_TRY(sort_and_segment(L.s, L.perm, L.seg, (size_t)K, (unsigned)T, st));
    }
    // without a selection and without slots (K = 0) the walk finds no slot and writes the zeros itself
    DEFTET_LAUNCH(k_tcs_bwd_vertices, dim3(blocks_for(V, kPvBlock), (unsigned)B), dim3(kPvBlock), st, grad_cent, offsets,
                  slots, sorted ? (const int32_t *)L.seg : (const int32_t *)nullptr, sorted ? (const int32_t *)L.perm : (const int32_t *)nullptr,
                  first, grad_pos, V, K, idx_batch, accumulate);
    return DEFTET_OK;
}

}  // extern "C"
