// image_sample.hip — pixel-aligned image features for the single-image branch: feature maps f32 [B,C_k,H_k,W_k]
// read bilinearly at projected points uv f32 [B,N,2] (grid_sample's convention, layers/disn.py:257-305) and written side by side
// with the global feature rows and the appended rows into ONE result f32 [B, G + sum C_k + A, N]; the gradients to the maps, to
// uv and to the global features.  The 2-D twin of pointvoxel.hip: no float atomics anywhere, the scatter into the maps is a gather
// over a stable sort of the points by cell (cell_gather.hpp), so every sum has one fixed order and two runs give the same bits.
//
// Orders of summation (the contracts of include/deftet_hip.h):
//   sampling      ((w00 f00 + w01 f01) + w10 f10) + w11 f11, x fastest, w = (x factor) * (y factor); a corner outside the map adds 0
//   to the maps   per (channel, cell) four corner sums over the cell's points in ascending p (the sort is stable; a segment longer
//                 than 32 points by 64 lanes and a fixed butterfly, see cell_gather.hpp), then per texel the partials of corner
//                 (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) in that order, from 0
//   to uv         channels ascending from 0, one map after the other (the caller's list order: the first launch writes, later add)
//   to global     per row lane l adds n = l, l + 64, ... from 0, then a fixed butterfly over the 64 lanes (offsets 32 .. 1)
#include "image_sample.hpp"                     // pixel_of, tap_of, sample_tap, slope_tap: one statement for forward and backward

namespace deftet {
namespace {

constexpr size_t kIsPartialBudget = (size_t)32 << 20;                // scratch for the corner partials: the channels are chunked to fit it
// the one layout both entries with a workspace carve: the sort's arrays, then the partials
inline CellWs layout(int B, int N, int H, int W, void *ws)
{
    return cell_layout<4>((size_t)B * N, (size_t)B * cells_of(H, W), kIsPartialBudget, false, false, ws);
}

// ---------------------------------------------------------------------------- forward
__global__ __launch_bounds__(kPvBlock) void k_is_fwd(const float *__restrict__ map, const float *__restrict__ uv, float *out, int C, int H,
                                                     int W, int N, int c_off, int C_total, int border, int align, int c_per)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.z;
    if (p >= N) return;
    Tap t;
    tap_of(uv[((size_t)b * N + p) * 2], uv[((size_t)b * N + p) * 2 + 1], H, W, border, align, t);
    const size_t HW = (size_t)H * W;
    const int c0 = blockIdx.y * c_per, c1 = min(C, c0 + c_per);
    for (int c = c0; c < c1; ++c) out[((size_t)b * C_total + c_off + c) * N + p] = sample_tap(map + ((size_t)b * C + c) * HW, t);
}

// rows [0,G): global_features[b,g] for every point; rows [C_total - A, C_total): append[b,p,a] transposed
__global__ __launch_bounds__(kPvBlock) void k_is_rows(const float *__restrict__ glob, const float *__restrict__ app, float *out, int G, int A,
                                                      int N, int C_total, int r_per)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.z;
    if (p >= N) return;
    const int r0 = blockIdx.y * r_per, r1 = min(G + A, r0 + r_per);
    for (int r = r0; r < r1; ++r) {
        if (r < G) out[((size_t)b * C_total + r) * N + p] = glob[(size_t)b * G + r];
        else out[((size_t)b * C_total + (C_total - A) + (r - G)) * N + p] = app[((size_t)b * N + p) * A + (r - G)];
    }
}

// ---------------------------------------------------------------------------- backward to the maps
__global__ __launch_bounds__(kPvBlock) void k_is_keys(const float *__restrict__ uv, unsigned *keys, int N, int H, int W, int border, int align,
                                                      unsigned n_keys)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (p >= N) return;
    Tap t;
    tap_of(uv[((size_t)b * N + p) * 2], uv[((size_t)b * N + p) * 2 + 1], H, W, border, align, t);
    keys[(size_t)b * N + p] = t.out ? n_keys : (unsigned)b * (unsigned)cells_of(H, W) + (unsigned)cell_of(t, W);
}
// the four weights of the points in sorted order, corner-major: wsorted[k][j] (a fully-outside point: zeros, behind every segment)
__global__ __launch_bounds__(kPvBlock) void k_is_weights(const float *__restrict__ uv, const int32_t *__restrict__ perm, float *wsorted, int B,
                                                         int N, int H, int W, int border, int align)
{
    const size_t BN = (size_t)B * N, j = (size_t)blockIdx.x * kPvBlock + threadIdx.x;
    if (j >= BN) return;
    const int g = perm[j];
    Tap t;
    tap_of(uv[(size_t)g * 2], uv[(size_t)g * 2 + 1], H, W, border, align, t);
#pragma unroll
    for (int k = 0; k < 4; ++k) wsorted[(size_t)k * BN + j] = t.out ? 0.0f : t.w[k];
}

// The two stages of cell_gather.hpp with four corners, every term kept; a long segment is the usual case here: the vertices along
// a viewing ray project to one pixel.
// k_is_map_from_partials: texel (y,x) adds the up to four partials that meet in it, corner order, from 0.  A corner partial that
// lands outside the map is never read.
__global__ __launch_bounds__(kPvBlock) void k_is_map_from_partials(const float *__restrict__ part, float *gmap, int C, int H, int W, int c_first,
                                                                   int c_chunk, int c_count)
{
    const int HW = H * W, n_cells = cells_of(H, W), b = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * kPvBlock + threadIdx.x;
    if (t >= (size_t)c_count * HW) return;
    const int cl = (int)(t / HW), v = (int)(t - (size_t)cl * HW), y = v / W, x = v - y * W;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                   // corner k of the cell whose lo corner is (y - ky, x - kx) >= (-1, -1)
        const int cy = y - (k >> 1) + 1, cx = x - (k & 1) + 1;
        acc = __fadd_rn(acc, part[(((size_t)b * c_chunk + cl) * 4 + k) * n_cells + (size_t)(cy * (W + 1) + cx)]);
    }
    gmap[((size_t)b * C + c_first + cl) * HW + v] = acc;
}

// ---------------------------------------------------------------------------- backward to uv
__global__ __launch_bounds__(kPvBlock) void k_is_bwd_uv(const float *__restrict__ map, const float *__restrict__ uv,
                                                        const float *__restrict__ gout, float *guv, int C, int H, int W, int N, int c_off,
                                                        int C_total, int border, int align, int accumulate)
{
    const int p = blockIdx.x * kPvBlock + threadIdx.x, b = blockIdx.y;
    if (p >= N) return;
    Tap t;
    tap_of(uv[((size_t)b * N + p) * 2], uv[((size_t)b * N + p) * 2 + 1], H, W, border, align, t);
    const size_t HW = (size_t)H * W;
    float gx = 0.0f, gy = 0.0f;
    if (!t.out) {
        for (int c = 0; c < C; ++c) {
            const float go = gout[((size_t)b * C_total + c_off + c) * N + p];
            float ddx, ddy;
            slope_tap(map + ((size_t)b * C + c) * HW, t, ddx, ddy);
            gx += go * ddx;
            gy += go * ddy;
        }
    }
    const float sx = align ? 0.5f * (float)(W - 1) : 0.5f * (float)W, sy = align ? 0.5f * (float)(H - 1) : 0.5f * (float)H;
    const float rx = t.out || t.hx ? 0.0f : sx * gx, ry = t.out || t.hy ? 0.0f : sy * gy;
    float *dst = guv + ((size_t)b * N + p) * 2;
    dst[0] = accumulate ? dst[0] + rx : rx;
    dst[1] = accumulate ? dst[1] + ry : ry;
}

// ---------------------------------------------------------------------------- backward to the global features
// one wave per row (b, g) of grad_out's first G rows
__global__ __launch_bounds__(kPvBlock) void k_is_rowsum(const float *__restrict__ gout, float *gglob, int n_rows, int G, int N, int C_total)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * (kPvBlock / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                      // wave-uniform
    const int b = row / G, g = row - b * G;
    const float *src = gout + ((size_t)b * C_total + g) * N;
    float s = 0.0f;
    for (int n = lane; n < N; n += 64) s = __fadd_rn(s, src[n]);
#pragma unroll  // wave_sum's order (wave.hpp); written out, a call changes this kernel's instruction stream
    for (int off = 32; off >= 1; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
    if (lane == 0) gglob[row] = s;
}

inline int check_sizes(int B, int C, int N, int H, int W, const char *what)
{
    if (B < 0 || C < 0 || N < 0 || H < 1 || W < 1) return set_error(DEFTET_EINVAL, "%s: negative size or a map side below 1", what);
    if (B > 65535) return set_error(DEFTET_ELIMIT, "%s: more than 65535 shapes", what);
    if (((long long)H + 1) * ((long long)W + 1) * (long long)(B > 0 ? B : 1) >= 0x7FFFFFFFll || (long long)B * N >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: B (H + 1) (W + 1) or B N does not fit 31 bits", what);
    if ((long long)C * H * W / kPvBlock >= 0x7FFFFFFFll) return set_error(DEFTET_ELIMIT, "%s: C H W too large", what);
    return DEFTET_OK;
}
inline bool flags_ok(int border, int align) { return (border == 0 || border == 1) && (align == 0 || align == 1); }

}  // namespace
}  // namespace deftet

using namespace deftet;

extern "C" {

size_t deftet_image_sample_workspace_bytes(int n_batch, int n_point, int height, int width)
{
    if (n_batch < 0 || n_point < 0 || height < 1 || width < 1) return 0;
    return layout(n_batch, n_point, height, width, nullptr).bytes;
}

int deftet_image_sample_fwd_f32(const float *map, const float *uv, const float *global_features, const float *append, float *out,
                                int n_batch, int n_channel, int height, int width, int n_point, int n_global, int n_append,
                                int channel_offset, int n_channel_total, int border, int align_corners, void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, H = height, W = width, G = global_features ? n_global : 0, A = append ? n_append : 0;
    DEFTET_TRY(check_sizes(B, C, N, H, W, "image_sample"));
    DEFTET_CHECK_ARG(n_global >= 0 && n_append >= 0, "image_sample: negative row count");
    DEFTET_CHECK_ARG(channel_offset >= 0 && (long long)n_channel_total >= (long long)channel_offset + C,
                     "image_sample: channel offset + channels exceed the destination");
    DEFTET_CHECK_ARG((long long)n_channel_total >= (long long)G + A && (C == 0 || (channel_offset >= G && channel_offset + C <= n_channel_total - A)),
                     "image_sample: the map's rows overlap the global or the appended rows");
    DEFTET_CHECK_ARG(flags_ok(border, align_corners), "image_sample: border and align_corners are 0 or 1");
    if (B == 0 || N == 0 || (C == 0 && G + A == 0)) return DEFTET_OK;
    DEFTET_CHECK_ARG(out && (C == 0 || (map && uv)), "image_sample: null pointer");
    hipStream_t st = as_stream(stream);
    const unsigned gN = blocks_for(N, kPvBlock);
    if (C > 0) {
        const int c_per = channels_per_thread(C, (long long)gN * B);
        const unsigned gC = blocks_for(C, c_per);
        if (gC > 65535u) return set_error(DEFTET_ELIMIT, "image_sample: too many channel chunks");
        DEFTET_LAUNCH(k_is_fwd, dim3(gN, gC, B), dim3(kPvBlock), st, map, uv, out, C, H, W, N, channel_offset, n_channel_total, border,
                      align_corners, c_per);
    }
    if (G + A > 0) {
        const int r_per = channels_per_thread(G + A, (long long)gN * B);
        const unsigned gR = blocks_for(G + A, r_per);
        if (gR > 65535u) return set_error(DEFTET_ELIMIT, "image_sample: too many row chunks");
        DEFTET_LAUNCH(k_is_rows, dim3(gN, gR, B), dim3(kPvBlock), st, global_features, append, out, G, A, N, n_channel_total, r_per);
    }
    return DEFTET_OK;
}

int deftet_image_cells_f32(const float *uv, int32_t *perm, int32_t *seg, float *wsorted, int n_batch, int n_point, int height, int width,
                           int border, int align_corners, void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, N = n_point, H = height, W = width;
    DEFTET_TRY(check_sizes(B, 0, N, H, W, "image_cells"));
    DEFTET_CHECK_ARG(flags_ok(border, align_corners), "image_cells: border and align_corners are 0 or 1");
    const CellWs L = layout(B, N, H, W, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(seg, "image_cells: null pointer");
    hipStream_t st = as_stream(stream);
    const unsigned n_keys = (unsigned)((size_t)B * cells_of(H, W));
    if (N == 0) {
        DEFTET_HIP(hipMemsetAsync(seg, 0, ((size_t)n_keys + 1) * sizeof(int32_t), st));
        return DEFTET_OK;
    }
    DEFTET_CHECK_ARG(uv && perm && wsorted, "image_cells: null pointer");
    const size_t n = (size_t)B * N;
    DEFTET_LAUNCH(k_is_keys, dim3(blocks_for(N, kPvBlock), B), dim3(kPvBlock), st, uv, L.s.keys, N, H, W, border, align_corners,
                  n_keys);
    DEFTET_TRY(sort_and_segment(L.s, perm, seg, n, n_keys, st));
    DEFTET_LAUNCH(k_is_weights, dim3(blocks_for(n, kPvBlock)), dim3(kPvBlock), st, uv, (const int32_t *)perm, wsorted, B, N, H,
                  W, border, align_corners);
    return DEFTET_OK;
}

int deftet_image_sample_bwd_map_f32(const float *grad_out, const int32_t *perm, const int32_t *seg, const float *wsorted, float *grad_map,
                                    int n_batch, int n_channel, int height, int width, int n_point, int channel_offset, int n_channel_total,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, H = height, W = width;
    DEFTET_TRY(check_sizes(B, C, N, H, W, "image_sample_bwd_map"));
    DEFTET_CHECK_ARG(channel_offset >= 0 && (long long)n_channel_total >= (long long)channel_offset + C,
                     "image_sample_bwd_map: channel offset + channels exceed the source");
    const CellWs L = layout(B, N, H, W, workspace);
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    if (B == 0 || C == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(seg && grad_map && (N == 0 || (grad_out && perm && wsorted)), "image_sample_bwd_map: null pointer");
    const size_t HW = (size_t)H * W;
    hipStream_t st = as_stream(stream);
    return cell_gather_bwd<4>(L, KeepEvery{}, grad_out, perm, seg, wsorted, B, cells_of(H, W), N, C, channel_offset, n_channel_total, st,
                              [&](const float *part, int c0, int c_chunk, int cc) -> int {
                                  DEFTET_LAUNCH(k_is_map_from_partials, dim3(blocks_for((size_t)cc * HW, kPvBlock), (unsigned)B),
                                                dim3(kPvBlock), st, part, grad_map, C, H, W, c0, c_chunk, cc);
                                  return DEFTET_OK;
                              });
}

int deftet_image_sample_bwd_uv_f32(const float *map, const float *uv, const float *grad_out, float *grad_uv, int n_batch, int n_channel,
                                   int height, int width, int n_point, int channel_offset, int n_channel_total, int border,
                                   int align_corners, int accumulate, void *stream)
{
    const int B = n_batch, C = n_channel, N = n_point, H = height, W = width;
    DEFTET_TRY(check_sizes(B, C, N, H, W, "image_sample_bwd_uv"));
    DEFTET_CHECK_ARG(channel_offset >= 0 && (long long)n_channel_total >= (long long)channel_offset + C,
                     "image_sample_bwd_uv: channel offset + channels exceed the source");
    DEFTET_CHECK_ARG(flags_ok(border, align_corners), "image_sample_bwd_uv: border and align_corners are 0 or 1");
    if (B == 0 || N == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(uv && grad_uv && (C == 0 || (map && grad_out)), "image_sample_bwd_uv: null pointer");
    DEFTET_LAUNCH(k_is_bwd_uv, dim3(blocks_for(N, kPvBlock), B), dim3(kPvBlock), as_stream(stream), map, uv, grad_out, grad_uv,
                  C, H, W, N, channel_offset, n_channel_total, border, align_corners, accumulate);
    return DEFTET_OK;
}

int deftet_image_sample_bwd_global_f32(const float *grad_out, float *grad_global, int n_batch, int n_global, int n_point, int n_channel_total,
                                       void *stream)
{
    const int B = n_batch, G = n_global, N = n_point;
    DEFTET_CHECK_ARG(B >= 0 && G >= 0 && N >= 0 && n_channel_total >= G, "image_sample_bwd_global: negative size or more global rows than rows");
    if ((long long)B * G >= 0x7FFFFFFFll) return set_error(DEFTET_ELIMIT, "image_sample_bwd_global: B G does not fit 31 bits");
    if (B == 0 || G == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(grad_global && (N == 0 || grad_out), "image_sample_bwd_global: null pointer");
    const int rows = B * G, per = kPvBlock / 64;
    DEFTET_LAUNCH(k_is_rowsum, dim3(blocks_for(rows, per)), dim3(kPvBlock), as_stream(stream), grad_out, grad_global, rows, G, N,
                  n_channel_total);
    return DEFTET_OK;
}

}  // extern "C"
