// cell_gather.hpp — the scatter of a point's gradient into the grid cells it read, as an atomic-free gather: the
// points are sorted by cell (stable), the weights stored corner-major in sorted order, per (channel, cell) the corner partials
// summed in ONE fixed order, then per voxel / texel the partials that meet in it gathered.  pointvoxel.hip (eight corners; through
// it tet_centroid_sample) and image_sample.hip (four corners) are the two users of all of it: the partials kernel, the chunked
// driver and the workspace layout.  tet_centroid_sample.hip and tet_field_sample.hip use the sort plumbing alone.  Everything sits
// in an anonymous namespace: each translation unit gets its own copy (the kernels included).
#pragma once
#include "prims.hpp"

namespace deftet {
namespace {

constexpr int kPvBlock = 256;
constexpr int kCellShort = 32;                  // a longer segment is summed by the whole wave

// ---------------------------------------------------------------------------- sort plumbing
// seg[s] = the first sorted position whose key is >= s, s in [0, n_keys]: voxel / cell s owns [seg[s], seg[s + 1])
__global__ __launch_bounds__(kPvBlock) void k_pv_segments(const unsigned *__restrict__ sorted, unsigned n, unsigned n_keys, int32_t *seg)
{
    const unsigned s = blockIdx.x * kPvBlock + threadIdx.x;
    if (s > n_keys) return;
    unsigned a = 0u, b = n;
    while (a < b) {
        const unsigned m = a + (b - a) / 2u;
        if (sorted[m] < s) a = m + 1u;
        else b = m;
    }
    seg[s] = (int32_t)a;
}

inline int key_bits(unsigned n_keys)
{
    int bits = 1;
    while (bits < 32 && (n_keys >> bits) != 0u) ++bits;             // the sentinel n_keys itself must be representable
    return bits;
}

struct SortBufs {
    unsigned *keys, *sorted;
    void *tmp;
    size_t tmp_bytes;
};
// the three arrays of a sort of n keys, taken from A in this order
inline void take_sort(Arena &A, size_t n, SortBufs &s)
{
    s.keys = A.take<unsigned>(n);
    s.sorted = A.take<unsigned>(n);
    s.tmp_bytes = prims::radix_sort_temp_bytes<unsigned, unsigned>(n);
    s.tmp = A.take<char>(s.tmp_bytes);
}
// keys (already written) -> perm (the point ids b N + p in key order, stable) and seg
inline int sort_and_segment(const SortBufs &s, int32_t *perm, int32_t *seg, size_t n, unsigned n_keys, hipStream_t st)
{
    DEFTET_TRY(prims::radix_sort_from<unsigned, unsigned>(prims::PtrLoad<unsigned>{s.keys}, s.sorted, prims::IotaLoad{}, (unsigned *)perm,
                                                          n, key_bits(n_keys), s.tmp, s.tmp_bytes, st));
    DEFTET_LAUNCH(k_pv_segments, dim3(blocks_for(n_keys + 1, kPvBlock)), dim3(kPvBlock), st, (const unsigned *)s.sorted, (unsigned)n,
                  n_keys, seg);
    return DEFTET_OK;
}

// channels per thread so that the grid has a few thousand workgroups; the sums do not depend on it
inline int channels_per_thread(int C, long long groups_per_channel_chunk)
{
    const long long want = 4096;
    long long chunks = (want + groups_per_channel_chunk - 1) / groups_per_channel_chunk;
    chunks = chunks < 1 ? 1 : (chunks > C ? C : chunks);
    return (int)((C + chunks - 1) / chunks);
}

// ---------------------------------------------------------------------------- the workspace
// The one layout every entry of the two operators carves (over a null base: its size): the sort's arrays of n points, with
// `own_perm_seg` a perm [n] and a seg [n_keys + 1] behind them (avg_voxelize keeps its own inside the workspace), and the corner
// partials of a chunk of channels: `budget` bytes, or one channel (n_keys cells of NC floats) if that is larger.  The sort and the
// partials belong to separate entries on one stream and are never live together: with `overlay` they share the bytes.
struct CellWs {
    SortBufs s;
    int32_t *perm, *seg;
    float *part;
    size_t part_bytes, bytes;
};
template <int NC>
inline CellWs cell_layout(size_t n, size_t n_keys, size_t budget, bool own_perm_seg, bool overlay, void *ws)
{
    Arena A(ws);
    CellWs w{};
    take_sort(A, n, w.s);
    if (own_perm_seg) {
        w.perm = A.take<int32_t>(n);
        w.seg = A.take<int32_t>(n_keys + 1);
    }
    const size_t sort_end = A.end(), one = n_keys * NC * sizeof(float);
    if (overlay) A.off = 0;
    w.part_bytes = one > budget ? one : budget;
    w.part = A.take<float>(w.part_bytes / sizeof(float));
    w.bytes = sort_end > A.end() ? sort_end : A.end();
    return w;
}

// ---------------------------------------------------------------------------- backward to the grid, two stages
// Two stages, so that every gout element is read once.
// k_cell_partials: per (channel, cell) the NC corner sums part[b][c][k][cell] = sum over the cell's points, in sorted (= ascending
// point) order, of wsorted[k][j] * gout[b,c,perm[j]].  A thread owns a cell; a segment of up to kCellShort points it walks itself
// (the fine volumes: ~1.4 points per cell, most cells empty).  A longer segment (the coarse volumes: ~90 points per cell; the
// vertices along a viewing ray that project to one pixel) is summed by the whole wave: lane l adds the points j0 + l, j0 + l + 64,
// ... in that order, then the 64 lane sums are added by a fixed butterfly (offsets 32, 16, ... 1).  THE DETERMINISM CONTRACT: the
// order depends on the segment's length only, never on the launch or on timing.
// Keep decides at compile time which corner terms count: KeepEvery here, KeepNominal in pointvoxel.hip (the legacy inds / wgts).
// The operator's own second kernel gathers, per voxel / texel, the partials that meet in it, in corner order, from 0.
// Gathers both: the only stores are the thread's own cell and the thread's own voxel / texel.
struct KeepEvery {
    __device__ void corners(int, int *) const {}
    __device__ bool operator()(int, int, const int *) const { return true; }
};

template <int NC, class Keep>
__device__ __forceinline__ void add_point(float acc[NC], const float *__restrict__ wsorted, size_t BN, int j, float gv, const Keep &keep,
                                          const int vk[NC])
{
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        if (!keep(k, j, vk)) continue;
        acc[k] = __fadd_rn(acc[k], __fmul_rn(wsorted[(size_t)k * BN + j], gv));
    }
}

template <int NC, class Keep>
__global__ __launch_bounds__(kPvBlock) void k_cell_partials(const float *__restrict__ gout, const int32_t *__restrict__ perm,
                                                            const int32_t *__restrict__ seg, const float *__restrict__ wsorted, float *part,
                                                            Keep keep, int B, int n_cells, int N, int c_first, int C_total, int c_chunk)
{
    const int b = blockIdx.z, cl = blockIdx.y, lane = threadIdx.x & 63;
    const int cell = blockIdx.x * kPvBlock + threadIdx.x;           // (no early return: the wave's shuffles below need every lane)
    const bool in = cell < n_cells;
    const size_t BN = (size_t)B * N;
    const int j0 = in ? seg[(size_t)b * n_cells + cell] : 0, j1 = in ? seg[(size_t)b * n_cells + cell + 1] : 0;
    const float *g = gout + ((size_t)b * C_total + c_first + cl) * N - (size_t)b * N;      // perm holds b N + p
    float acc[NC] = {};
    int vk[NC];
    keep.corners(in ? cell : 0, vk);
    const bool is_long = j1 - j0 > kCellShort;
    if (!is_long)
        for (int j = j0; j < j1; ++j) add_point<NC>(acc, wsorted, BN, j, g[perm[j]], keep, vk);
    unsigned long long longs = __ballot(is_long);                   // wave-uniform: every lane runs the loop below alike
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1ull;
        const int a0 = __shfl(j0, src), a1 = __shfl(j1, src);
        int wk[NC];
        keep.corners(__shfl(cell, src), wk);
        float s[NC] = {};
        for (int j = a0 + lane; j < a1; j += 64) add_point<NC>(s, wsorted, BN, j, g[perm[j]], keep, wk);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
#pragma unroll  // wave_sum's order (wave.hpp); written out, a call changes this kernel's instruction stream
            for (int off = 32; off >= 1; off >>= 1) s[k] = __fadd_rn(s[k], __shfl_xor(s[k], off));
            if (lane == src) acc[k] = s[k];
        }
    }
    if (in) {
#pragma unroll
        for (int k = 0; k < NC; ++k) part[(((size_t)b * c_chunk + cl) * NC + k) * n_cells + cell] = acc[k];
    }
}

// The channels [c_off, c_off + C) of gout in chunks that fit the layout's partials (at most 65,535: the grid's y), one chunk after
// the other on the stream, so the scratch is reused: the partials of the chunk, then from_partials(part, c0, c_chunk, cc), which
// launches the operator's gather for the channels [c0, c0 + cc) of its grid.  n_cells: the cells of one shape.
template <int NC, class Keep, class Gather>
inline int cell_gather_bwd(const CellWs &L, Keep keep, const float *gout, const int32_t *perm, const int32_t *seg, const float *wsorted, int B,
                           int n_cells, int N, int C, int c_off, int C_total, hipStream_t st, Gather from_partials)
{
    size_t fit = L.part_bytes / ((size_t)B * n_cells * NC * sizeof(float));                 // >= 1 by the layout
    if (fit > 65535) fit = 65535;
    const int c_chunk = (int)fit < C ? (int)fit : C;
    const unsigned gCell = blocks_for(n_cells, kPvBlock);
    for (int c0 = 0; c0 < C; c0 += c_chunk) {
        const int cc = C - c0 < c_chunk ? C - c0 : c_chunk;
        DEFTET_LAUNCH((k_cell_partials<NC, Keep>), dim3(gCell, (unsigned)cc, (unsigned)B), dim3(kPvBlock), st, gout, perm, seg, wsorted, L.part,
                      keep, B, n_cells, N, c_off + c0, C_total, c_chunk);
        DEFTET_TRY(from_partials((const float *)L.part, c0, c_chunk, cc));
    }
    return DEFTET_OK;
}

}  // namespace
}  // namespace deftet
