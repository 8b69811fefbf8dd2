// surface_batch.hpp — what the per-shape surface operators layers.DefTet.forward calls (SURVEY.md section 8 rows A8, A9, A10:
// face_adjacency.hip, tri_distance.hip, nearest_neighbor.hip) share for CDNA4 / gfx950:
//
//   1. the batch of shapes in one launch: workspace slices (kBatchShapes, ShapeCounts, SHAPE, group_shapes), the per-shape
//      exclusive scan k_scan_excl, the counting-sort rank run_atomic_rank, the batch width kNNBatch of the wave-uniform tables;
//   2. the mechanics of the two far passes (k_nn_far_*, k_tri_far_*): the packed (distance bits, index) best-answer word with
//      its exchange between the waves of a block, and the distance to the slab of a cell layer.
//
// Only the mechanics are shared.  The certified margins (1.00003f, 0.9997f, abs_slack, R = sqrt(U) * 1.00001) differ per
// operator on purpose and stay at the call sites, as do the grids (NNGrid, TGrid: any struct with o, cs, slack will do for
// slab_dist) and what a lane evaluates (FarLane, TriLane).  The wave-wide x-range reduction of k_nn_far_rows and
// k_tri_far_rows also stays written out in both: as a shared function it compiled to other instructions in either kernel.
//
// All three reference kernels are "one thread per query, loop over every primitive from global memory".  Here the primitive
// stream is wave-uniform: it is read once per wave through the scalar cache (s_load) and broadcast as SGPR operands, one query
// per lane, so the vector memory pipe only carries the queries and the results.  The arithmetic follows the reference
// operation by operation in fp32 with FMA contraction off (the argmin / neighbour indices are decided by exact fp32
// comparisons), double-typed literals promoted as C++ does.
#pragma once
#include "common.hpp"
#include "wave.hpp"

namespace deftet {
namespace surf {

using u64 = unsigned long long;
using u32 = unsigned int;

// --- batching across shapes ----------------------------------------------------------------------------
// The grid-accelerated operators keep every per-shape scratch array in a workspace SLICE of `slice` bytes; slice s starts
// s * slice bytes after slice 0.  A batched launch covers kBatchShapes shapes with its y (or z) grid dimension: the
// kernels get the pointers of slice 0 and rebase them with SHAPE(ptr), their inputs / outputs with their own strides.
// The per-shape element counts travel by value.  (One launch sequence for a batch instead of one per shape: at ~40
// launches per shape and operator the command processor was what bounded a training step's surface terms.)
constexpr int kBatchShapes = 8;
struct ShapeCounts { int n[kBatchShapes]; };
#define SHAPE(ptr) (ptr) = reinterpret_cast<decltype(ptr)>(reinterpret_cast<uintptr_t>(ptr) + (size_t)sb * slice)
static int group_shapes(int B) { return B < 1 ? 1 : (B < kBatchShapes ? B : kBatchShapes); }      // the largest launch group of B shapes

// exclusive prefix sums of n ints per shape, one launch: workgroup (j, shape) scans tile j (kScanThreads * kScanPer
// elements) after adding up everything before its tile itself — the arrays are a few hundred thousand ints, so the
// redundant reads (L2 hits) cost less than a carry chain through one workgroup (94 us per call in round 2) or a second
// launch.  out[n] receives the total when with_total.
constexpr int kScanThreads = 1024, kScanPer = 16, kScanTile = kScanThreads * kScanPer;
static inline unsigned scan_tiles(long long n) { return (unsigned)((n + kScanTile - 1) / kScanTile > 0 ? (n + kScanTile - 1) / kScanTile : 1); }
static __global__ __launch_bounds__(kScanThreads) void k_scan_excl(const int *in, int *out, int n, size_t slice, int with_total)
{
    __shared__ int wsum[kScanThreads / 64];
    const int sb = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    SHAPE(in); SHAPE(out);
    const int base = blockIdx.x * kScanTile;
    // carry: the sum of in[0, base) (base is a multiple of the tile, the arrays are 256-byte aligned)
    int carry = 0;
    for (int i = tid * 4; i < base; i += kScanThreads * 4) {
        const int4 q = *reinterpret_cast<const int4 *>(in + i);
        carry += (q.x + q.y) + (q.z + q.w);
    }
    carry = wave_sum(carry);
    if (lane == 0) wsum[w] = carry;
    __syncthreads();
    carry = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) carry += wsum[k];
    __syncthreads();
    int v[kScanPer], sum = 0;
    const int i0 = base + tid * kScanPer;
    if (i0 + kScanPer <= n) {                                       // 16-byte loads
#pragma unroll
        for (int k = 0; k < kScanPer; k += 4) {
            const int4 q = *reinterpret_cast<const int4 *>(in + i0 + k);
            v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
    }
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) sum += v[k];
    const int incl = wave_incl_sum(sum, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int run = carry + incl - sum, tot = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) { if (k < w) run += wsum[k]; tot += wsum[k]; }
    if (i0 + kScanPer <= n) {
#pragma unroll
        for (int k = 0; k < kScanPer; k += 4) {
            int4 q;
            q.x = run; q.y = q.x + v[k]; q.z = q.y + v[k + 1]; q.w = q.z + v[k + 2];
            run = q.w + v[k + 3];
            *reinterpret_cast<int4 *>(out + i0 + k) = q;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) { if (i0 + k < n) out[i0 + k] = run; run += v[k]; }
    }
    if (with_total && tid == 0 && blockIdx.x == gridDim.x - 1) out[n] = carry + tot;
}

// rank = atomicAdd(&counter[key], 1) for every lane with key >= 0, with ONE atomic per run of consecutive lanes that share
// a key: point clouds sampled face by face put ~20 consecutive points into the same cell, and returning atomics on a
// handful of addresses were what the binning kernels spent their time on (k_tri_point_keys 76 us, k_nn_bin 42 us per
// 8 x 97 k points).  Must be called by all lanes of the wave (key < 0: no count).
__device__ __forceinline__ int run_atomic_rank(int *counter, int key)
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1);
    const bool head = key >= 0 && (lane == 0 || prev != key);
    const unsigned long long heads = __ballot(head || key < 0);     // a lane without a key also ends the run before it
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);   // lanes 0..lane
    const int start = 63 - __clzll((long long)(heads & upto));
    const unsigned long long above = heads & ~upto;
    const int end = above ? __ffsll((long long)above) - 1 : 64;
    int base = 0;
    if (head) base = atomicAdd(&counter[key], end - start);
    base = __shfl(base, start);
    return key >= 0 ? base + (lane - start) : 0;
}

// --- the far passes ------------------------------------------------------------------------------------
// records of a wave-uniform table (representatives, row starts, coarse cells) are read this many at a time
constexpr int kNNBatch = 8;

// A lane's best answer as ONE word (distance bits, index): the distances are non-negative, so min over the words is the
// lexicographic (distance, index) minimum = the reference's first strict minimum of an ascending scan.
__device__ __forceinline__ u64 pack_best(float d, int idx) { return ((u64)(unsigned)__float_as_int(d) << 32) | (unsigned)idx; }
__device__ __forceinline__ void unpack_best(u64 v, float &d, int &idx) { d = __int_as_float((int)(v >> 32)); idx = (int)(unsigned)v; }
// every one of the W waves of the block leaves with the block's best answer so far
template <int W>
__device__ __forceinline__ void share_best(u64 (*s_pack)[64], int part, int lane, float &d, int &idx)
{
    s_pack[part][lane] = pack_best(d, idx);
    __syncthreads();
    u64 v = s_pack[0][lane];
#pragma unroll
    for (int w = 1; w < W; ++w) v = min(v, s_pack[w][lane]);
    unpack_best(v, d, idx);
    __syncthreads();
}

// distance from x to the slab of cell layer c on axis k of grid g (0 inside; a flat axis is one unbounded slab)
template <class Grid>
__device__ __forceinline__ float slab_dist(const Grid &g, int k, int c, float x)
{
    if (!(g.cs[k] < INFINITY)) return 0.f;
    const float l = g.o[k] + (float)c * g.cs[k] - g.slack[k], h = g.o[k] + (float)(c + 1) * g.cs[k] + g.slack[k];
    return fmaxf(fmaxf(l - x, x - h), 0.f);
}

}  // namespace surf
}  // namespace deftet
