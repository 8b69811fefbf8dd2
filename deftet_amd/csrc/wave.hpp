// wave.hpp — the cross-lane layer over one 64-lane wave (gfx950), stated once.  THE ORDERS HERE ARE PART OF RESULTS: every sum
// that promises "the same bits on every run" rests on them.
//   * wave_reduce / wave_sum / wave_min / wave_max: the xor butterfly over offsets 32, 16, ..., 1 — lane l takes op(mine, value
//     of lane l ^ off); these ops commute bit for bit, so every lane ends with the same bits;
//   * wave_incl: the __shfl_up inclusive scan over offsets 1, 2, ..., 32 — lane l >= off takes op(mine, value of lane l - off);
//   * wave_scan_add / wave_scan_max / wave_pk_max: the DPP scan — row_shr 1, 2, 4, 8, then row_bcast15 and row_bcast31.
// Many sites keep their loop written out, because a call compiles their kernel to another instruction stream; each names the
// function here whose order it follows ("Wave primitives", lists them).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace deftet {

typedef unsigned long long lanemask_t;                      // one bit per lane: __ballot's value, an SGPR pair

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T x, Op op)       // result in every lane
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = op(x, __shfl_xor(x, off));
    return x;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T x) { return wave_reduce(x, [](T a, T b) { return a + b; }); }
template <typename T>
__device__ __forceinline__ T wave_min(T x) { return wave_reduce(x, [](T a, T b) { return min(a, b); }); }
template <typename T>
__device__ __forceinline__ T wave_max(T x) { return wave_reduce(x, [](T a, T b) { return max(a, b); }); }
__device__ __forceinline__ float wave_min(float x) { return wave_reduce(x, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max(float x) { return wave_reduce(x, [](float a, float b) { return fmaxf(a, b); }); }

template <typename T, typename Op>
__device__ __forceinline__ T wave_incl(T v, Op op, int lane)   // lane = threadIdx.x & 63
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v = op(v, t);
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_incl_sum(T v, int lane) { return wave_incl(v, [](T a, T b) { return a + b; }, lane); }

// Data-parallel-primitive moves: full-rate VALU, where ds_bpermute shuffles go through the LDS pipe.  The control words:
//   row_shr:n   0x110 + n   lane l reads lane l - n of its own 16-lane row
//   wave_shr:1  0x138       lane l reads lane l - 1, across the rows too
//   row_bcast15 0x142       lane 15 of each row to the next row; row mask 0xa writes rows 1 and 3 only
//   row_bcast31 0x143       lane 31 to rows 2 and 3; row mask 0xc writes those two only
// A scan is row_shr 1, 2, 4, 8 (inclusive inside each row), row_bcast15 under 0xa (the two halves), row_bcast31 under 0xc (the
// wave).  A lane without a source or in a masked row receives 0 either way: with BOUND_CTRL the move reads 0 for it, without
// it the lane keeps `old` = 0.  The encodings differ and the compiler folds them into their consumers differently: raster.hip
// moves without bound_ctrl, point_in_tet.hip with it, each as measured there — so the choice is a template argument.
template <int CTRL, int ROW_MASK, bool BOUND_CTRL>
__device__ __forceinline__ int dpp_move(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xf, BOUND_CTRL); }
template <int CTRL, int ROW_MASK, bool BOUND_CTRL>
__device__ __forceinline__ float dpp_move(float x) { return __int_as_float(dpp_move<CTRL, ROW_MASK, BOUND_CTRL>(__float_as_int(x))); }
template <int N, bool BOUND_CTRL, typename T>
__device__ __forceinline__ T row_shr(T x) { return dpp_move<0x110 + N, 0xf, BOUND_CTRL>(x); }   // N = 1 .. 15
template <bool BOUND_CTRL, int ROW_MASK = 0xa, typename T>
__device__ __forceinline__ T row_bcast15(T x) { return dpp_move<0x142, ROW_MASK, BOUND_CTRL>(x); }
template <bool BOUND_CTRL, int ROW_MASK = 0xc, typename T>
__device__ __forceinline__ T row_bcast31(T x) { return dpp_move<0x143, ROW_MASK, BOUND_CTRL>(x); }
template <bool BOUND_CTRL, typename T>
__device__ __forceinline__ T wave_shr1(T x) { return dpp_move<0x138, 0xf, BOUND_CTRL>(x); }

__device__ __forceinline__ float lane_below(float x) { return wave_shr1<false>(x); }   // the lane below's value; lane 0 receives 0
__device__ __forceinline__ int lane_below(int x) { return wave_shr1<false>(x); }

__device__ __forceinline__ int wave_scan_add(int x)    // inclusive scans over the 64 lanes
{
    x += row_shr<1, true>(x); x += row_shr<2, true>(x); x += row_shr<4, true>(x); x += row_shr<8, true>(x);
    x += row_bcast15<true>(x); x += row_bcast31<true>(x);
    return x;
}
__device__ __forceinline__ int wave_scan_max(int x)    // x >= 0
{
    x = max(x, row_shr<1, true>(x)); x = max(x, row_shr<2, true>(x)); x = max(x, row_shr<4, true>(x)); x = max(x, row_shr<8, true>(x));
    x = max(x, row_bcast15<true>(x)); x = max(x, row_bcast31<true>(x));
    return x;
}
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b)
{
    const u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(unsigned, r);
}
// max of both 16-bit halves over all lanes (max is idempotent: the row masks of a scan are not needed); wave-uniform
__device__ __forceinline__ unsigned wave_pk_max(unsigned v)
{
    v = pk_max(v, (unsigned)row_shr<1, true>((int)v)); v = pk_max(v, (unsigned)row_shr<2, true>((int)v));
    v = pk_max(v, (unsigned)row_shr<4, true>((int)v)); v = pk_max(v, (unsigned)row_shr<8, true>((int)v));
    v = pk_max(v, (unsigned)row_bcast15<true, 0xf>((int)v)); v = pk_max(v, (unsigned)row_bcast31<true, 0xf>((int)v));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Select with the lane mask in an SGPR pair (VOP3 v_cndmask_b32_e64).  Written as `c ? a : b` on a per-lane bool, hipcc emits
// the VCC form `v_cndmask_b32_e32 ..., vcc` where it can, which gfx950 issues about eight times slower than any other VALU
// instruction (9.4 ns per wave-instruction per SIMD against 1.25 for an FMA and 1.85 for this form: tools/probes/
// valu_rate_probe.hip).  The point-in-tet traversal carries a dozen selects per iteration and 21 of them were a seventh of a
// wave's time in the rasterizer's k_bwd_sorted.  T is int or float, each in its own registers: routed through the other type's
// bit casts, the kernels of raster.hip (float) or of point_in_tet.hip (int) compile to other instructions.
template <typename T>
__device__ __forceinline__ T lane_select(lanemask_t m, T if_set, T if_clear)
{
    static_assert(std::is_same<T, int>::value || std::is_same<T, float>::value, "int or float: one 32-bit register");
    T d;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(d) : "v"(if_clear), "v"(if_set), "s"(m));
    return d;
}
__device__ __forceinline__ unsigned lane_select(lanemask_t m, unsigned if_set, unsigned if_clear)
{
    return (unsigned)lane_select(m, (int)if_set, (int)if_clear);
}

__device__ __forceinline__ int lane_bcast(int v, int k) { return __builtin_amdgcn_readlane(v, k); }   // lane k's value (uniform k) in every lane
__device__ __forceinline__ float lane_bcast(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

}  // namespace deftet
