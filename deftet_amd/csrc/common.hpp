// common.hpp — shared helpers for libdeftet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/deftet_hip.h"

namespace deftet {

// thread-local last-error message (deftet_last_error)
char *err_buf();
int set_error(int code, const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

#define DEFTET_CHECK_ARG(cond, ...)                                  \
    do {                                                              \
        if (!(cond)) return deftet::set_error(DEFTET_EINVAL, __VA_ARGS__); \
    } while (0)

// status propagation: the one way a host function hands a callee's refusal or launch error up (variadic: a template
// argument list may bring its own commas)
#define DEFTET_TRY(...)                                               \
    do {                                                              \
        const int rc_ = (__VA_ARGS__);                                \
        if (rc_ != DEFTET_OK) return rc_;                             \
    } while (0)

#define DEFTET_HIP(call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return deftet::set_error(DEFTET_ELAUNCH, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define DEFTET_LAUNCH_CHECK(name)                                                          \
    do {                                                                                    \
        hipError_t e_ = hipGetLastError();                                                  \
        if (e_ != hipSuccess)                                                               \
            return deftet::set_error(DEFTET_ELAUNCH, "launch of %s failed: %s", name, hipGetErrorString(e_)); \
    } while (0)

// Optional per-kernel timing (deftet_profile_select / deftet_profile_read): when a kernel
// name is selected, every launch of that kernel is bracketed by a pair of hipEvents recorded
// on the launch stream.  Off by default; costs one strcmp-free pointer compare per launch.
bool prof_match(const char *name);
void prof_begin(hipStream_t st);
void prof_end(hipStream_t st);

#define DEFTET_LAUNCH(kern, grid, block, stream, ...)                          \
    do {                                                                       \
        const bool prof_ = deftet::prof_match(#kern);                          \
        if (prof_) deftet::prof_begin(stream);                                 \
        hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);         \
        if (prof_) deftet::prof_end(stream);                                   \
        DEFTET_LAUNCH_CHECK(#kern);                                            \
    } while (0)

// same, with dynamic LDS bytes
#define DEFTET_LAUNCH_SHM(kern, grid, block, shm, stream, ...)                 \
    do {                                                                       \
        const bool prof_ = deftet::prof_match(#kern);                          \
        if (prof_) deftet::prof_begin(stream);                                 \
        hipLaunchKernelGGL(kern, grid, block, shm, stream, __VA_ARGS__);       \
        if (prof_) deftet::prof_end(stream);                                   \
        DEFTET_LAUNCH_CHECK(#kern);                                            \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }   // a: a power of two
// workgroups of `block` items that cover n items (host side: launch arguments)
inline unsigned blocks_for(size_t n, size_t block) { return (unsigned)((n + block - 1) / block); }
// The workspace acceptance rule ("Workspaces"): the caller's buffer is present, `align`-byte aligned and at least
// `need` bytes long.  DEFTET_OK, or DEFTET_EINVAL with the one wording (common.cpp), which names the entry and both byte counts.
int workspace_refused(const char *who, const void *ws, size_t got, size_t need, size_t align);
inline int workspace_ok(const char *who, const void *ws, size_t got, size_t need, size_t align = 256)
{
    return ws && aligned(ws, align) && need <= got ? DEFTET_OK : workspace_refused(who, ws, got, need, align);
}
__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7FC00000); }
__device__ __forceinline__ void cross3(const float *a, const float *b, float *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// XCD-aware placement of a 1-D grid whose size is a MULTIPLE OF 8: workgroups go round-robin to the eight XCDs, so every XCD
// takes one CONTIGUOUS share of the logical blocks and the rows that neighbouring ones share are fetched into one L2.  Speed only.
__device__ __forceinline__ int xcd_logical_block() { return (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3); }
// Keeps the RETURNING form of an atomic whose old value is not used: it is complete at the memory side once it has returned,
// and that return is what the s_waitcnt of the ticket reductions observes before they draw their ticket.
template <typename T>
__device__ __forceinline__ void keep_returning(T old) { asm volatile("" ::"v"(old)); }

// bump allocator over the caller's workspace.  Over a null base it only measures: a layout function runs once that way for the
// *_workspace_bytes value and once over the real pointer for the arrays, so the two cannot disagree ("Workspaces").
struct Arena {
    char *base;
    size_t off, cap;
    Arena(void *p, size_t bytes) : base(static_cast<char *>(p)), off(0), cap(bytes) {}
    explicit Arena(void *p) : Arena(p, ~(size_t)0) {}                 // no capacity of its own: the caller compares end() with what it was given
    size_t end() const { return align_up(off, 256); }                // bytes of the layout so far, whole 256-byte lines
    template <typename T>
    T *take(size_t n) {
        off = align_up(off, 256);
        T *r = reinterpret_cast<T *>(base + off);
        off += n * sizeof(T);
        return r;
    }
    bool ok() const { return off <= cap; }
};

constexpr int kWave = 64;  // CDNA4 wavefront

// Ticket reductions (reduce.hip, tet_ops.hip) finish inside one launch by counting workgroups on device-global counters.
// Two launches may only share a set of counters if they cannot run at the same time: launches on ONE stream are ordered, so
// every (device, stream) pair gets its own slot of counters, at most `n_slots` of them per process; -1 when they are used up
// (the caller then takes its multi-launch form, which needs no counters).
int ticket_slot_for_stream(hipStream_t st, int n_slots);

// vertex_ops.hip: grad_pos[b,v] = sum over the (tet, corner) incidences of vertex v of the rows of a [B,T,4,3] gradient, in the
// incidence CSR's order (k_gather_bwd).  rowMask == nullptr: dense rows.  Otherwise the rows are in the COMPACTED form
// k_bary_bwd_hits<true> writes (point_in_tet.hip): rowMask[b][t / 64] has bit t % 64 set iff tet t has a row, stored at row
// (t & ~63) + popcount(mask below the bit); absent rows are zero and are skipped (x + 0 = x: the same sums, bit for bit).
namespace vtx {
int gather_bwd_rows(const float *rows, const unsigned long long *rowMask, const int32_t *offsets, const int32_t *slots, float *grad_pos,
                    int B, int V, int T, int idx_batch, int accumulate, hipStream_t st);
// vertex_ops.hip: the incidence CSR of an index list int64 [idx_batch,E,corners] over V vertices — offsets int32 [idx_batch*V+1],
// slots int32 [idx_batch*corners*E] holding corners*e + corner in ascending order per vertex; *bad_flag = 1 for an index outside
// [0,V).  corners = 4 is deftet_tet_vertex_csr_i32, corners = 3 is deftet_face_vertex_csr_i32 (render_vertices.hip).
size_t incidence_csr_workspace_bytes(int idx_batch, int V, int E, int corners);
int incidence_csr(const int64_t *idx, int32_t *offsets, int32_t *slots, int32_t *bad_flag, int idx_batch, int V, int E, int corners,
                  void *workspace, size_t workspace_bytes, hipStream_t st);
}

}  // namespace deftet
