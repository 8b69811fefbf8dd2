// grid_setup.hpp — what every spatially binned operator shares when it builds its uniform grid: the cell function and the
// reduction of a bounding box (plus a few running sums) over the elements of a shape.
//
//   1. a 256-thread statistics kernel accumulates a BoxStats per thread over a strided loop and ends with block_store():
//      one record of 2 D + S floats per block — lo[0..D), hi[0..D), sum[0..S);
//   2. a 64-lane grid kernel (or the head of the next kernel) reduces the records — load() + wave_reduce() with one record
//      per lane, load_reduce() for any other number — and derives origin, inverse cell size and cell count;
//   3. elements and queries are mapped to cells with grid_cell().
//
// Only these steps are shared.  What a grid kernel makes of the reduced box — the flat-axis threshold, the cell size of a flat
// axis, the slack — differs per operator on purpose and feeds the certified bounds of DESIGN.md ("Grid set-up" lists the
// differences); it stays with the operator.
//
// ORDER OF THE SUMS.  The sums decide cell counts, so their order is part of the result: a thread's own strided sum, the wave
// butterfly in wave.hpp's order (wave_sum), then waves 0, 1, 2, 3 one after the other.  min / max do not depend on the order.
#pragma once
#include "common.hpp"

namespace deftet {

// Cell of x on an axis with origin o, inverse cell size inv and G cells: floor, clamped to [0, G - 1].  fmaxf / fminf return
// their other operand when one is NaN, so a NaN coordinate lands in cell 0 instead of an undefined conversion; inv == 0 (a
// flat axis) puts everything into cell 0.  Monotone non-decreasing in x, which the certified boxes of the callers rely on.
// (point_in_tet.hip keeps a variant of its own, v_med3 and truncation: one instruction less in kernels that are tuned to the
// register, with the monotonicity argument written out beside it.)
__device__ __forceinline__ int grid_cell(float x, float o, float inv, int G)
{
    float f = floorf((x - o) * inv);
    f = fminf(fmaxf(f, 0.f), (float)(G - 1));
    return (int)f;
}

template <int D, int S>
struct BoxStats {
    static constexpr int kWords = 2 * D + S;
    float lo[D], hi[D], sum[S > 0 ? S : 1];

    __device__ __forceinline__ BoxStats()
    {
#pragma unroll
        for (int k = 0; k < D; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
#pragma unroll
        for (int s = 0; s < S; ++s) sum[s] = 0.f;
    }
    // (the caller decides which elements count: a NaN coordinate is dropped by fminf / fmaxf, an infinite one is not)
    __device__ __forceinline__ void add_point(const float *p) { add_box(p, p); }
    __device__ __forceinline__ void add_box(const float *l, const float *h)
    {
#pragma unroll
        for (int k = 0; k < D; ++k) { lo[k] = fminf(lo[k], l[k]); hi[k] = fmaxf(hi[k], h[k]); }
    }
    __device__ __forceinline__ void add_sum(int s, float v) { sum[s] += v; }

    // every lane ends up with the wave's box and sums (wave.hpp's order, written out: calls change the statistics kernels' streams)
    __device__ __forceinline__ void wave_reduce()
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                lo[k] = fminf(lo[k], __shfl_xor(lo[k], off));
                hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off));
            }
#pragma unroll
            for (int s = 0; s < S; ++s) sum[s] += __shfl_xor(sum[s], off);
        }
    }
    // the whole 256-thread block -> one record; a block-wide call (it holds the barrier)
    __device__ __forceinline__ void block_store(float (*sh)[kWords], float *rec)
    {
        wave_reduce();
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) { sh[w][k] = lo[k]; sh[w][D + k] = hi[k]; }
#pragma unroll
            for (int s = 0; s < S; ++s) sh[w][2 * D + s] = sum[s];
        }
        __syncthreads();
        if (threadIdx.x < kWords) {
            const int k = threadIdx.x;
            float v = sh[0][k];
            for (int i = 1; i < 4; ++i) v = k < D ? fminf(v, sh[i][k]) : k < 2 * D ? fmaxf(v, sh[i][k]) : v + sh[i][k];
            rec[k] = v;
        }
    }
    __device__ __forceinline__ void load(const float *__restrict__ rec)
    {
#pragma unroll
        for (int k = 0; k < D; ++k) { lo[k] = rec[k]; hi[k] = rec[D + k]; }
#pragma unroll
        for (int s = 0; s < S; ++s) sum[s] = rec[2 * D + s];
    }
    // n records by one wave, lane by lane in a fixed order, then the butterfly
    __device__ __forceinline__ void load_reduce(const float *__restrict__ part, int n)
    {
        for (int i = (int)(threadIdx.x & 63); i < n; i += 64) {
            add_box(part + i * kWords, part + i * kWords + D);
#pragma unroll
            for (int s = 0; s < S; ++s) sum[s] += part[i * kWords + 2 * D + s];
        }
        wave_reduce();
    }
};

}  // namespace deftet
