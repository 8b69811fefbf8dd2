// pointvoxel.hip — the two point-voxel operators that join the point-cloud encoder to the tet grid:
//   average voxelization (layers/pv_module/functional/src/voxelization/vox.cu) forward and backward, and
//   trilinear sampling of voxel volumes at points (pc_model.py:182-194 sample_f; functional/devoxelization.py;
//   src/interpolate/trilinear_devox.cu) forward, backward to the volumes and backward to the positions.
// No float atomics anywhere: both scatters are turned into gathers by a stable sort of the points by voxel / by cell
// (prims.hpp), so every sum has one fixed order and two runs give the same bits.
//
// Orders of summation (the contracts of include/deftet_hip.h):
//   voxelization   out[b,c,s] = 0 + feat[i0] * inv + feat[i1] * inv + ...   over the points of voxel s in ascending i, every
//                  product rounded before it is added (what the reference kernel computes with its threads one after another)
//   sampling       ((w000 f000 + w001 f001) + w010 f010) + ... + w111 f111, z fastest, w = (wx * wy) * wz
//   to the volumes per (channel, cell) eight corner sums over the cell's points in ascending p (the sort is stable; a long segment
//                  by 64 lanes and a fixed butterfly, see cell_gather.hpp), then per voxel the partials of corner 000 .. 111
//   to positions   channels in ascending order, one volume after the other (the caller's list order)
#include "cell_gather.hpp"                      // the sort by cell, the corner partials and their workspace: shared with image_sample.hip
#include "pointvoxel.hpp"                       // load_u, corners_of, pos_grad_of_volume: shared with tet_centroid_sample.hip

namespace deftet {
namespace {

// ---------------------------------------------------------------------------- average voxelization
__global__ __launch_bounds__(kPvBlock) void k_vox_keys(const int32_t *__restrict__ coords, int32_t *ind, unsigned *keys, int N, int R,
                                                       unsigned n_keys)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (p >= N) return;
    const int x = coords[((size_t)b * 3 + 0) * N + p], y = coords[((size_t)b * 3 + 1) * N + p], z = coords[((size_t)b * 3 + 2) * N + p];
    const bool ok = x >= 0 && x < R && y >= 0 && y < R && z >= 0 && z < R;
    const int i = ok ? (x * R + y) * R + z : -1;
    ind[(size_t)b * N + p] = i;
    keys[(size_t)b * N + p] = ok ? (unsigned)b * (unsigned)(R * R * R) + (unsigned)i : n_keys;
}

__global__ __launch_bounds__(kPvBlock) void k_vox_fwd(const float *__restrict__ feat, const int32_t *__restrict__ perm,
                                                      const int32_t *__restrict__ seg, float *out, int32_t *cnt, int C, int N, int R3,
                                                      int c_per)
{
    const int s = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.z;
    if (s >= R3) return;
    const int j0 = seg[(size_t)b * R3 + s], j1 = seg[(size_t)b * R3 + s + 1];
    if (blockIdx.y == 0) cnt[(size_t)b * R3 + s] = j1 - j0;
    const float inv = j1 > j0 ? 1.0f / (float)(j1 - j0) : 0.0f;
    const int c0 = blockIdx.y * c_per, c1 = min(C, c0 + c_per);
    for (int c = c0; c < c1; ++c) {
        const float *f = feat + ((size_t)b * C + c) * N - (size_t)b * N;       // perm holds b N + p
        float acc = 0.0f;
        for (int j = j0; j < j1; ++j) acc = __fadd_rn(acc, __fmul_rn(f[perm[j]], inv));
        out[((size_t)b * C + c) * R3 + s] = acc;
    }
}

__global__ __launch_bounds__(kPvBlock) void k_vox_bwd(const float *__restrict__ gy, const int32_t *__restrict__ ind,
                                                      const int32_t *__restrict__ cnt, float *gx, int C, int N, int R3, int c_per)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.z;
    if (p >= N) return;
    const int i = ind[(size_t)b * N + p];
    const bool ok = i >= 0 && i < R3;
    const int n = ok ? cnt[(size_t)b * R3 + i] : 0;
    const float inv = n > 0 ? 1.0f / (float)n : 0.0f;
    const int c0 = blockIdx.y * c_per, c1 = min(C, c0 + c_per);
    for (int c = c0; c < c1; ++c)
        gx[((size_t)b * C + c) * N + p] = n > 0 ? __fmul_rn(gy[((size_t)b * C + c) * R3 + i], inv) : 0.0f;
}

// ---------------------------------------------------------------------------- trilinear sampling, forward
__global__ __launch_bounds__(kPvBlock) void k_vs_fwd(const float *__restrict__ vol, const float *__restrict__ pos, float *out, int32_t *inds,
                                                     float *wgts, int C, int R, int N, int c_off, int C_total, int mode, int legacy,
                                                     int c_per)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.z;
    if (p >= N) return;
    float raw[3], u[3];
    load_u(pos, mode, b, p, N, R, raw, u);
    Corners cn;
    corners_of(u, R, legacy != 0, cn);
    if (inds && blockIdx.y == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            inds[((size_t)b * 8 + k) * N + p] = cn.idx[k];
            wgts[((size_t)b * 8 + k) * N + p] = cn.w[k];
        }
    }
    const size_t R3 = (size_t)R * R * R;
    const int c0 = blockIdx.y * c_per, c1 = min(C, c0 + c_per);
    for (int c = c0; c < c1; ++c) {
        const float *f = vol + ((size_t)b * C + c) * R3;
        out[((size_t)b * C_total + c_off + c) * N + p] = sample_corners(f, cn);
    }
}

// ---------------------------------------------------------------------------- backward to the volumes
__global__ __launch_bounds__(kPvBlock) void k_cell_keys(const float *__restrict__ pos, int mode, unsigned *keys, int N, int R)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (p >= N) return;
    float raw[3], u[3];
    load_u(pos, mode, b, p, N, R, raw, u);
    const int x = (int)floorf(u[0]), y = (int)floorf(u[1]), z = (int)floorf(u[2]);
    keys[(size_t)b * N + p] = (unsigned)b * (unsigned)(R * R * R) + (unsigned)((x * R + y) * R + z);
}
// the eight weights of the points in sorted order, corner-major: wsorted[k][j]
__global__ __launch_bounds__(kPvBlock) void k_cell_weights(const float *__restrict__ pos, int mode, const int32_t *__restrict__ perm,
                                                           float *wsorted, int B, int N, int R)
{
    const size_t BN = (size_t)B * N, j = (size_t)blockIdx.x * kPvBlock + threadIdx.x;
    if (j >= BN) return;
    const int g = perm[j], b = g / N, p = g - b * N;
    float raw[3], u[3];
    load_u(pos, mode, b, p, N, R, raw, u);
    Corners cn;
    corners_of(u, R, false, cn);
#pragma unroll
    for (int k = 0; k < 8; ++k) wsorted[(size_t)k * BN + j] = cn.w[k];
}
// the legacy pair: the cell is inds[:,0,:]; a first index outside the volume drops the point (sentinel key)
__global__ __launch_bounds__(kPvBlock) void k_inds_keys(const int32_t *__restrict__ inds, unsigned *keys, int N, int R3, unsigned n_keys)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (p >= N) return;
    const int i = inds[(size_t)b * 8 * N + p];
    keys[(size_t)b * N + p] = i >= 0 && i < R3 ? (unsigned)b * (unsigned)R3 + (unsigned)i : n_keys;
}
__global__ __launch_bounds__(kPvBlock) void k_inds_gather(const int32_t *__restrict__ inds, const float *__restrict__ wgts,
                                                          const int32_t *__restrict__ perm, float *wsorted, int32_t *isorted, int B, int N)
{
    const size_t BN = (size_t)B * N, j = (size_t)blockIdx.x * kPvBlock + threadIdx.x;
    if (j >= BN) return;
    const int g = perm[j], b = g / N, p = g - b * N;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        wsorted[(size_t)k * BN + j] = wgts[((size_t)b * 8 + k) * N + p];
        isorted[(size_t)k * BN + j] = inds[((size_t)b * 8 + k) * N + p];
    }
}

// The two stages of cell_gather.hpp with eight corners.  KeepNominal (the legacy pair): a term counts only where the recorded
// index IS the voxel the corner nominally lands in — the reference's hi index falls back on lo where d == 0, and there its
// weight is exactly 0, so the terms left out are zeros.
// k_vs_vol_from_partials: voxel v adds the up to eight partials that meet in it, corner 000 .. 111 in that order, from 0.
constexpr size_t kPvPartialBudget = (size_t)64 << 20;               // scratch for the partials: the channels are chunked to fit it
// the one layout the four entries with a workspace carve: the sort's arrays, the voxelization's perm / seg, and over them the partials
inline CellWs layout(int B, int N, int R, void *ws)
{
    return cell_layout<8>((size_t)B * N, (size_t)B * R * R * R, kPvPartialBudget, true, true, ws);
}

struct KeepNominal {
    const int32_t *isorted;
    size_t BN;
    int R;
    // the voxel corner k of `cell` nominally lands in, -1 outside the volume
    __device__ void corners(int cell, int vk[8]) const
    {
        const int cx = cell / (R * R), cy = (cell / R) % R, cz = cell % R;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int x = cx + (k >> 2), y = cy + ((k >> 1) & 1), z = cz + (k & 1);
            vk[k] = x < R && y < R && z < R ? (x * R + y) * R + z : -1;
        }
    }
    __device__ bool operator()(int k, int j, const int vk[8]) const { return isorted[(size_t)k * BN + j] == vk[k]; }
};

__global__ __launch_bounds__(kPvBlock) void k_vs_vol_from_partials(const float *__restrict__ part, float *gvol, int C, int R, int c_first,
                                                                   int c_chunk, int c_count)
{
    const int R3 = R * R * R, b = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * kPvBlock + threadIdx.x;
    if (t >= (size_t)c_count * R3) return;
    const int cl = (int)(t / R3), v = (int)(t - (size_t)cl * R3);
    const int vx = v / (R * R), vy = (v / R) % R, vz = v % R;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cx = vx - (k >> 2), cy = vy - ((k >> 1) & 1), cz = vz - (k & 1);
        if (cx < 0 || cy < 0 || cz < 0) continue;
        acc = __fadd_rn(acc, part[(((size_t)b * c_chunk + cl) * 8 + k) * R3 + (size_t)((cx * R + cy) * R + cz)]);
    }
    gvol[((size_t)b * C + c_first + cl) * R3 + v] = acc;
}

// ---------------------------------------------------------------------------- backward to the positions
__global__ __launch_bounds__(kPvBlock) void k_vs_bwd_pos(const float *__restrict__ vol, const float *__restrict__ pos,
                                                         const float *__restrict__ gout, float *gpos, int C, int R, int N, int c_off,
                                                         int C_total, int mode, int accumulate)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (p >= N) return;
    float raw[3], u[3];
    load_u(pos, mode, b, p, N, R, raw, u);
    float res[3];
    pos_grad_of_volume(vol, gout, raw, u, b, p, C, R, N, c_off, C_total, mode, res);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float *dst = mode == 0 ? gpos + ((size_t)b * N + p) * 3 + j : gpos + ((size_t)b * 3 + j) * N + p;
        *dst = accumulate ? *dst + res[j] : res[j];
    }
}

inline int check_sizes(int B, int C, int N, int R, const char *what)
{
    if (B < 0 || C < 0 || N < 0 || R < 1) return set_error(DEFTET_EINVAL, "%s: negative size or resolution below 1", what);
    if (B > 65535) return set_error(DEFTET_ELIMIT, "%s: more than 65535 shapes", what);
    if ((long long)R * R * R * (long long)(B > 0 ? B : 1) >= 0x7FFFFFFFll || (long long)B * N >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: B R^3 or B N does not fit 31 bits", what);
    if ((long long)C * R * R * R / kPvBlock >= 0x7FFFFFFFll) return set_error(DEFTET_ELIMIT, "%s: C R^3 too large", what);
    return DEFTET_OK;
}

}  // namespace
}  // namespace deftet

using namespace deftet;

extern "C" {

size_t deftet_pointvoxel_workspace_bytes(int n_batch, int n_point, int resolution)
{
    if (n_batch < 0 || n_point < 0 || resolution < 0) return 0;
    return layout(n_batch, n_point, resolution, nullptr).bytes;
}

int deftet_avg_voxelize_fwd_f32(const float *feat, const int32_t *coords, float *out, int32_t *ind, int32_t *cnt, int n_batch,
                                int n_channel, int n_point, int resolution, void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, C, N, R, "avg_voxelize"));
    const size_t R3 = (size_t)R * R * R;
    hipStream_t st = as_stream(stream);
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(cnt && (out || C == 0), "avg_voxelize: null output");
    if (N == 0 || C == 0) {
        if (C > 0) DEFTET_HIP(hipMemsetAsync(out, 0, (size_t)B * C * R3 * sizeof(float), st));
        if (N == 0) {
            DEFTET_HIP(hipMemsetAsync(cnt, 0, (size_t)B * R3 * sizeof(int32_t), st));
            return DEFTET_OK;
        }
    }
    DEFTET_CHECK_ARG(coords && ind && (feat || C == 0), "avg_voxelize: null pointer");
    const size_t n = (size_t)B * N;
    const unsigned n_keys = (unsigned)((size_t)B * R3);
    const CellWs L = layout(B, N, R, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    const unsigned gN = blocks_for(N, kPvBlock);
    DEFTET_LAUNCH(k_vox_keys, dim3(gN, B), dim3(kPvBlock), st, coords, ind, L.s.keys, N, R, n_keys);
    DEFTET_TRY(sort_and_segment(L.s, L.perm, L.seg, n, n_keys, st));
    const unsigned gS = blocks_for(R3, kPvBlock);
    const int c_per = C > 0 ? channels_per_thread(C, (long long)gS * B) : 1;
    const unsigned gC = C > 0 ? blocks_for(C, c_per) : 1u;
    if (gC > 65535u) return set_error(DEFTET_ELIMIT, "avg_voxelize: too many channel chunks");
    DEFTET_LAUNCH(k_vox_fwd, dim3(gS, gC, B), dim3(kPvBlock), st, feat, (const int32_t *)L.perm, (const int32_t *)L.seg, out, cnt, C, N, (int)R3,
                  c_per);
    return DEFTET_OK;
}

int deftet_avg_voxelize_bwd_f32(const float *grad_y, const int32_t *ind, const int32_t *cnt, float *grad_x, int n_batch, int n_channel,
                                int n_point, int resolution, void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, C, N, R, "avg_voxelize_bwd"));
    if (B == 0 || C == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(grad_y && ind && cnt && grad_x, "avg_voxelize_bwd: null pointer");
    const unsigned gN = blocks_for(N, kPvBlock);
    const int c_per = channels_per_thread(C, (long long)gN * B);
    const unsigned gC = blocks_for(C, c_per);
    if (gC > 65535u) return set_error(DEFTET_ELIMIT, "avg_voxelize_bwd: too many channel chunks");
    DEFTET_LAUNCH(k_vox_bwd, dim3(gN, gC, B), dim3(kPvBlock), as_stream(stream), grad_y, ind, cnt, grad_x, C, N, R * R * R, c_per);
    return DEFTET_OK;
}

int deftet_voxel_sample_fwd_f32(const float *vol, const float *pos, float *out, int32_t *inds, float *wgts, int n_batch, int n_channel,
                                int resolution, int n_point, int channel_offset, int n_channel_total, int pos_mode, int legacy,
                                void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, C, N, R, "voxel_sample"));
    DEFTET_CHECK_ARG(channel_offset >= 0 && n_channel_total >= channel_offset + C, "voxel_sample: channel offset + channels exceed the destination");
    DEFTET_CHECK_ARG(pos_mode == 0 || pos_mode == 1, "voxel_sample: pos_mode 0 (pos [B,N,3]) or 1 (coords [B,3,N])");
    DEFTET_CHECK_ARG((inds == nullptr) == (wgts == nullptr), "voxel_sample: inds and wgts come together");
    if (B == 0 || N == 0 || (C == 0 && !inds)) return DEFTET_OK;
    DEFTET_CHECK_ARG(pos && (C == 0 || (vol && out)), "voxel_sample: null pointer");
    const unsigned gN = blocks_for(N, kPvBlock);
    const int c_per = C > 0 ? channels_per_thread(C, (long long)gN * B) : 1;
    const unsigned gC = C > 0 ? blocks_for(C, c_per) : 1u;
    if (gC > 65535u) return set_error(DEFTET_ELIMIT, "voxel_sample: too many channel chunks");
    DEFTET_LAUNCH(k_vs_fwd, dim3(gN, gC, B), dim3(kPvBlock), as_stream(stream), vol, pos, out, inds, wgts, C, R, N, channel_offset,
                  n_channel_total, pos_mode, legacy, c_per);
    return DEFTET_OK;
}

int deftet_voxel_cells_f32(const float *pos, int pos_mode, int32_t *perm, int32_t *seg, float *wsorted, int n_batch, int n_point,
                           int resolution, void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, 0, N, R, "voxel_cells"));
    DEFTET_CHECK_ARG(pos_mode == 0 || pos_mode == 1, "voxel_cells: pos_mode 0 or 1");
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(seg, "voxel_cells: null pointer");
    hipStream_t st = as_stream(stream);
    const unsigned n_keys = (unsigned)((size_t)B * R * R * R);
    if (N == 0) {
        DEFTET_HIP(hipMemsetAsync(seg, 0, ((size_t)n_keys + 1) * sizeof(int32_t), st));
        return DEFTET_OK;
    }
    DEFTET_CHECK_ARG(pos && perm && wsorted, "voxel_cells: null pointer");
    const size_t n = (size_t)B * N;
    const CellWs L = layout(B, N, R, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    DEFTET_LAUNCH(k_cell_keys, dim3(blocks_for(N, kPvBlock), B), dim3(kPvBlock), st, pos, pos_mode, L.s.keys, N, R);
    DEFTET_TRY(sort_and_segment(L.s, perm, seg, n, n_keys, st));
    DEFTET_LAUNCH(k_cell_weights, dim3(blocks_for(n, kPvBlock)), dim3(kPvBlock), st, pos, pos_mode, (const int32_t *)perm,
                  wsorted, B, N, R);
    return DEFTET_OK;
}

int deftet_voxel_cells_from_inds_i32(const int32_t *inds, const float *wgts, int32_t *perm, int32_t *seg, float *wsorted,
                                     int32_t *isorted, int n_batch, int n_point, int resolution, void *workspace, size_t workspace_bytes,
                                     void *stream)
{
    const int B = n_batch, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, 0, N, R, "voxel_cells_from_inds"));
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(seg, "voxel_cells_from_inds: null pointer");
    hipStream_t st = as_stream(stream);
    const int R3 = R * R * R;
    const unsigned n_keys = (unsigned)((size_t)B * R3);
    if (N == 0) {
        DEFTET_HIP(hipMemsetAsync(seg, 0, ((size_t)n_keys + 1) * sizeof(int32_t), st));
        return DEFTET_OK;
    }
    DEFTET_CHECK_ARG(inds && wgts && perm && wsorted && isorted, "voxel_cells_from_inds: null pointer");
    const size_t n = (size_t)B * N;
    const CellWs L = layout(B, N, R, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    DEFTET_LAUNCH(k_inds_keys, dim3(blocks_for(N, kPvBlock), B), dim3(kPvBlock), st, inds, L.s.keys, N, R3, n_keys);
    DEFTET_TRY(sort_and_segment(L.s, perm, seg, n, n_keys, st));
    DEFTET_LAUNCH(k_inds_gather, dim3(blocks_for(n, kPvBlock)), dim3(kPvBlock), st, inds, wgts, (const int32_t *)perm, wsorted,
                  isorted, B, N);
    return DEFTET_OK;
}

int deftet_voxel_sample_bwd_vol_f32(const float *grad_out, const int32_t *perm, const int32_t *seg, const float *wsorted,
                                    const int32_t *isorted, float *grad_vol, int n_batch, int n_channel, int resolution, int n_point,
                                    int channel_offset, int n_channel_total, void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, C, N, R, "voxel_sample_bwd_vol"));
    DEFTET_CHECK_ARG(channel_offset >= 0 && n_channel_total >= channel_offset + C, "voxel_sample_bwd_vol: channel offset + channels exceed the source");
    if (B == 0 || C == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(seg && grad_vol && (N == 0 || (grad_out && perm && wsorted)), "voxel_sample_bwd_vol: null pointer");
    const CellWs L = layout(B, N, R, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    const int R3 = R * R * R;
    hipStream_t st = as_stream(stream);
    auto gather = [&](const float *part, int c0, int c_chunk, int cc) -> int {
        DEFTET_LAUNCH(k_vs_vol_from_partials, dim3(blocks_for((size_t)cc * R3, kPvBlock), (unsigned)B), dim3(kPvBlock), st, part,
                      grad_vol, C, R, c0, c_chunk, cc);
        return DEFTET_OK;
    };
    if (isorted)
        return cell_gather_bwd<8>(L, KeepNominal{isorted, (size_t)B * N, R}, grad_out, perm, seg, wsorted, B, R3, N, C, channel_offset,
                                  n_channel_total, st, gather);
    return cell_gather_bwd<8>(L, KeepEvery{}, grad_out, perm, seg, wsorted, B, R3, N, C, channel_offset, n_channel_total, st, gather);
}

int deftet_voxel_sample_bwd_pos_f32(const float *vol, const float *pos, const float *grad_out, float *grad_pos, int n_batch, int n_channel,
                                    int resolution, int n_point, int channel_offset, int n_channel_total, int pos_mode, int accumulate,
                                    void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, R = resolution;
    DEFTET_TRY(check_sizes(B, C, N, R, "voxel_sample_bwd_pos"));
    DEFTET_CHECK_ARG(channel_offset >= 0 && n_channel_total >= channel_offset + C, "voxel_sample_bwd_pos: channel offset + channels exceed the source");
    DEFTET_CHECK_ARG(pos_mode == 0 || pos_mode == 1, "voxel_sample_bwd_pos: pos_mode 0 or 1");
    if (B == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(pos && grad_pos && (C == 0 || (vol && grad_out)), "voxel_sample_bwd_pos: null pointer");
    DEFTET_LAUNCH(k_vs_bwd_pos, dim3(blocks_for(N, kPvBlock), B), dim3(kPvBlock), as_stream(stream), vol, pos, grad_out,
                  grad_pos, C, R, N, channel_offset, n_channel_total, pos_mode, accumulate);
    return DEFTET_OK;
}

}  // extern "C"
