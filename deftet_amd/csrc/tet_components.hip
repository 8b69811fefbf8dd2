// tet_components.hip — connected components of the inside tets of every shape over the face-neighbour table, and the occupancy
// clean-up built on them: drop floaters, keep the largest piece, fill enclosed voids (gfx950).
//
// The reference leaves this to trimesh on the host ("use trimesh to fix the surface": utils/tet_utils.py:474,
// utils/mesh_utils.py:259,270, 3_model/utils_tetsv.py:132,229).
//
// Tets t and u of one shape are connected when both are inside and u stands in row t of nbr32 or t in row u.  The label of a
// component is its SMALLEST tet index, so the result does not depend on the schedule.
//
// Union-find with one invariant: parent[x] <= x, and parent[x] == x only for a root.  Every write keeps it — a root r is hooked
// under a smaller root by compare-and-swap (r -> q, q < r), a non-root is shortened to an ancestor by fetch_min — so a parent
// chain strictly descends, ends after at most x steps, and the root of a finished forest is the smallest index of its component
// whatever order the hooks happened in.  Launches:
//
//   k_tc_init     parent[t] = the smallest inside neighbour below t, else t (plain stores; no other lane reads them in this
//                 launch); zeroes the accumulators; counts the neighbour entries outside [-1, T) into `bad`
//   k_tc_hook     union(t, u) for every inside entry u of an inside row t, but for the one k_tc_init linked and for a u > t whose
//                 own row names t (that pair is united from u's side; a one-sided entry is united from the side that has it).
//                 Parent words change under other workgroups here, on any XCD: every access is a relaxed agent-scope atomic
//                 (L2-served, never a CU's L1).  No lane waits for another: a failed compare-and-swap means another lane hooked
//                 that root, and the retry starts from strictly smaller roots.
//   k_tc_flatten  label[t] = root(t) (behind the launch boundary every hook is visible); sizes, the open flag and the component
//                 count are summed per wave over the wave's DISTINCT labels first (ballot), then one integer atomic per
//                 (wave, label): a component that holds most of a shape costs T / 64 adds on its root's word, not T
//   k_tc_finish   sizes / open from the accumulator words
//
// and for the clean-up, with nothing read back: k_tc_fill (inside or an enclosed outside component), k_tc_best (per shape the
// largest surviving component, the smaller label among equals: a 64-bit max of size << 32 | ~label), k_tc_keep.
// Every loop has a trip bound in the code; a chain that breaks the invariant or a loop that runs out is counted in `bad`.
#include "common.hpp"
#include "union_find.hpp"
#include "wave.hpp"

namespace deftet {
namespace tc {

constexpr int kThreads = 256;
constexpr unsigned kOpenBit = 0x80000000u, kSizeMask = 0x7FFFFFFFu;

using uf::find_root;                                                  // union_find.hpp: the invariant, the hook, the shortening
using uf::unite;

__device__ __forceinline__ bool is_in(const unsigned char *in, int t, int invert) { return (in[t] != 0) != (invert != 0); }

__global__ __launch_bounds__(kThreads) void k_tc_init(const unsigned char *__restrict__ inside, int invert, const int4 *__restrict__ nbr,
                                                      int T, int count_bad, int *parent, unsigned *acc, int *count, int *bad)
{
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
    const bool live = t < T;
    int nbad = 0;
    if (live) {
        const unsigned char *in = inside + (size_t)b * T;
        const int4 n4 = nbr[t];
        const int n[4] = {n4.x, n4.y, n4.z, n4.w};
        const bool me = is_in(in, t, invert);
        int p = t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (n[i] < -1 || n[i] >= T) { ++nbad; continue; }          // counted, never followed
            if (me && n[i] >= 0 && n[i] < p && is_in(in, n[i], invert)) p = n[i];
        }
        parent[(size_t)b * T + t] = p;
        acc[(size_t)b * T + t] = 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) count[b] = 0;
    if (count_bad && b == 0) {                                         // the table is shared by the shapes: counted once
        const unsigned long long any = __ballot(nbad > 0);
        if (any) {
            int s = nbad;
            s = wave_sum(s);
            if ((threadIdx.x & 63) == 0) atomicAdd(bad, s);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_tc_hook(const unsigned char *__restrict__ inside, int invert, const int4 *__restrict__ nbr,
                                                      int T, int *parent, int *bad)
{
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const unsigned char *in = inside + (size_t)b * T;
    if (!is_in(in, t, invert)) return;
    int *par = parent + (size_t)b * T;
    const int4 n4 = nbr[t];
    const int n[4] = {n4.x, n4.y, n4.z, n4.w};
    const int trips = 2 * T + 2;
    bool link[4];
    int first = t;                                                     // what k_tc_init made the parent of t: linked already
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = n[i];
        link[i] = u >= 0 && u < T && u != t && is_in(in, u, invert);
        if (link[i] && u < first) first = u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = n[i];
        if (!link[i] || u == first) continue;
        if (u > t) {                                                   // row u names t: the pair is united from u's side
            const int4 m = nbr[u];
            if (m.x == t || m.y == t || m.z == t || m.w == t) continue;
        }
        unite(par, t, u, trips, bad);
    }
}

__global__ __launch_bounds__(kThreads) void k_tc_flatten(const unsigned char *__restrict__ inside, int invert, const int4 *__restrict__ nbr,
                                                         int T, int *parent, int *labels, unsigned *acc, int *count, int *bad)
{
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
    const unsigned char *in = inside + (size_t)b * T;
    const bool me = t < T && is_in(in, t, invert);
    int L = -1;
    bool open = false;
    if (me) {
        L = find_root(parent + (size_t)b * T, t, bad);
        const int4 n4 = nbr[t];
        open = n4.x == -1 || n4.y == -1 || n4.z == -1 || n4.w == -1;
    }
    if (t < T) labels[(size_t)b * T + t] = L;
    // one add per distinct label of the wave (every lane of the wave is here: no lane has returned)
    unsigned *accb = acc + (size_t)b * T;
    unsigned long long todo = __ballot(L >= 0);
    for (int k = 0; k < 64 && todo; ++k) {
        const int leader = __ffsll((long long)todo) - 1;
        const int Lf = __shfl(L, leader);
        const bool mine = L == Lf;                                     // (Lf >= 0: lanes without a label never match)
        const unsigned long long same = __ballot(mine), op = __ballot(mine && open);
        if (lane == leader) {
            atomicAdd(accb + Lf, (unsigned)__popcll(same));
            if (op) atomicOr(accb + Lf, kOpenBit);
        }
        todo &= ~same;
    }
    const unsigned long long roots = __ballot(me && L == t);
    if (lane == 0 && roots) atomicAdd(count + b, (int)__popcll(roots));
}

__global__ __launch_bounds__(kThreads) void k_tc_finish(const unsigned *__restrict__ acc, size_t n, int *sizes, unsigned char *open)
{
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const unsigned a = acc[e];
    if (sizes) sizes[e] = (int)(a & kSizeMask);
    if (open) open[e] = (unsigned char)(a >> 31);
}

// labels / acc: the components of the COMPLEMENT of inside
__global__ __launch_bounds__(kThreads) void k_tc_fill(const unsigned char *__restrict__ inside, const int *__restrict__ labels,
                                                      const unsigned *__restrict__ acc, int T, unsigned char *filled)
{
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const size_t e = (size_t)b * T + t;
    const int L = labels[e];
    bool in = inside[e] != 0;
    if (!in && L >= 0 && L < T) in = !(acc[(size_t)b * T + L] & kOpenBit);
    filled[e] = in ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_tc_best(const int *__restrict__ labels, const unsigned *__restrict__ acc, int T, int min_size,
                                                      unsigned long long *best)
{
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long key = 0ull;
    if (t < T && labels[(size_t)b * T + t] == t) {
        const unsigned size = acc[(size_t)b * T + t] & kSizeMask;
        if (size >= (unsigned)min_size) key = ((unsigned long long)size << 32) | (unsigned long long)(~(unsigned)t);
    }
    key = wave_reduce(key, [](unsigned long long mine, unsigned long long other) { return other > mine ? other : mine; });
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best + b, key);
}

__global__ __launch_bounds__(kThreads) void k_tc_keep(const int *__restrict__ labels, const unsigned *__restrict__ acc,
                                                      const unsigned long long *__restrict__ best, int T, int min_size, int keep_largest,
                                                      unsigned char *keep)
{
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const size_t e = (size_t)b * T + t;
    const int L = labels[e];
    bool k = L >= 0 && L < T;
    if (k && min_size > 0) k = (acc[(size_t)b * T + L] & kSizeMask) >= (unsigned)min_size;
    if (k && keep_largest) {
        const unsigned long long w = best[b];
        k = w != 0ull && (unsigned)L == ~(unsigned)(w & 0xFFFFFFFFull);
    }
    keep[e] = k ? 1 : 0;
}

}  // namespace tc
}  // namespace deftet

using namespace deftet;
using namespace deftet::tc;

namespace {
// parent: the forest; acc: size and open bit per label; labels / mask: the clean-up's own labelling and the filled mask;
// best: the winner of keep_largest per shape; count: the clean-up's component count when the caller does not ask for it
struct Ws {
    int *parent, *labels, *count;
    unsigned *acc;
    unsigned char *mask;
    unsigned long long *best;
    size_t bytes;
};
Ws carve(void *workspace, int B, int T)
{
    Arena A(workspace);
    Ws w{};
    const size_t n = (size_t)B * T;
    w.parent = A.take<int>(n);
    w.acc = A.take<unsigned>(n);
    w.labels = A.take<int>(n);
    w.mask = A.take<unsigned char>(n);
    w.best = A.take<unsigned long long>((size_t)B);
    w.count = A.take<int>((size_t)B);
    w.bytes = A.end();
    return w;
}

int check_shape(const char *who, const void *inside, const void *nbr, int B, int T, const void *bad, void *workspace, size_t wsb, Ws &W)
{
    DEFTET_CHECK_ARG(T >= 1, "%s: n_tet=%d must be positive", who, T);
    DEFTET_CHECK_ARG(B >= 1 && B <= 65535, "%s: n_batch=%d outside 1..65535", who, B);
    DEFTET_CHECK_ARG((long long)B * T < 2147483647LL && T <= 1073741822, "%s: n_batch * n_tet does not fit 31 bits", who);
    DEFTET_CHECK_ARG(inside, "%s: null pointer: inside_bxt", who);
    DEFTET_CHECK_ARG(nbr && ((uintptr_t)nbr & 15) == 0, "%s: null or misaligned pointer: nbr32_tx4", who);
    DEFTET_CHECK_ARG(bad, "%s: null pointer: bad", who);
    W = carve(workspace, B, T);
    DEFTET_TRY(workspace_ok(who, workspace, wsb, W.bytes));
    return DEFTET_OK;
}

// labels / acc / count of the components of (inside != 0) ^ invert
int label(const unsigned char *inside, int invert, const int32_t *nbr, int B, int T, int count_bad, const Ws &W, int *labels, int *count,
          int *bad, hipStream_t st)
{
    const dim3 grid(blocks_for(T, kThreads), B), block(kThreads);
    DEFTET_LAUNCH(k_tc_init, grid, block, st, inside, invert, (const int4 *)nbr, T, count_bad, W.parent, W.acc, count, bad);
    DEFTET_LAUNCH(k_tc_hook, grid, block, st, inside, invert, (const int4 *)nbr, T, W.parent, bad);
    DEFTET_LAUNCH(k_tc_flatten, grid, block, st, inside, invert, (const int4 *)nbr, T, W.parent, labels, W.acc, count, bad);
    return DEFTET_OK;
}

int finish(const Ws &W, int B, int T, int *sizes, unsigned char *open, hipStream_t st)
{
    const size_t n = (size_t)B * T;
    DEFTET_LAUNCH(k_tc_finish, dim3(blocks_for(n, kThreads)), dim3(kThreads), st, (const unsigned *)W.acc, n, sizes, open);
    return DEFTET_OK;
}
}  // namespace

extern "C" size_t deftet_tet_components_workspace_bytes(int B, int T)
{
    return B <= 0 || T <= 0 ? 256 : carve(nullptr, B, T).bytes;
}

extern "C" int deftet_tet_components_u8(const uint8_t *inside_bxt, const int32_t *nbr32_tx4, int B, int T, int32_t *labels, int32_t *sizes,
                                        uint8_t *open, int32_t *count, int32_t *bad, void *workspace, size_t wsb, void *stream_)
{
    Ws W;
    DEFTET_TRY(check_shape("tet_components", inside_bxt, nbr32_tx4, B, T, bad, workspace, wsb, W));
    DEFTET_CHECK_ARG(labels && sizes && open && count, "tet_components: null pointer: labels / sizes / open / count");
    hipStream_t st = as_stream(stream_);
    DEFTET_HIP(hipMemsetAsync(bad, 0, 4, st));
    DEFTET_TRY(label(inside_bxt, 0, nbr32_tx4, B, T, 1, W, labels, count, bad, st));
    return finish(W, B, T, sizes, open, st);
}

extern "C" int deftet_occupancy_cleanup_u8(const uint8_t *inside_bxt, const int32_t *nbr32_tx4, int B, int T, int keep_largest, int min_size,
                                           int fill_voids, uint8_t *keep, int32_t *labels, int32_t *sizes, uint8_t *open, int32_t *count,
                                           int32_t *bad, void *workspace, size_t wsb, void *stream_)
{
    Ws W;
    DEFTET_TRY(check_shape("occupancy_cleanup", inside_bxt, nbr32_tx4, B, T, bad, workspace, wsb, W));
    DEFTET_CHECK_ARG(keep, "occupancy_cleanup: null pointer: keep");
    DEFTET_CHECK_ARG(min_size >= 0, "occupancy_cleanup: min_size=%d is negative", min_size);
    DEFTET_CHECK_ARG((labels != nullptr) == (sizes != nullptr) && (labels != nullptr) == (open != nullptr) &&
                         (labels != nullptr) == (count != nullptr),
                     "occupancy_cleanup: labels, sizes, open and count go together");
    hipStream_t st = as_stream(stream_);
    const dim3 grid(blocks_for(T, kThreads), B), block(kThreads);
    int *lab = labels ? labels : W.labels, *cnt = count ? count : W.count;
    DEFTET_HIP(hipMemsetAsync(bad, 0, 4, st));
    const uint8_t *mask = inside_bxt;
    if (fill_voids) {
        DEFTET_TRY(label(inside_bxt, 1, nbr32_tx4, B, T, 1, W, lab, cnt, bad, st));
        DEFTET_LAUNCH(k_tc_fill, grid, block, st, inside_bxt, (const int *)lab, (const unsigned *)W.acc, T, W.mask);
        mask = W.mask;
    }
    DEFTET_TRY(label(mask, 0, nbr32_tx4, B, T, !fill_voids, W, lab, cnt, bad, st));
    if (keep_largest) {
        DEFTET_HIP(hipMemsetAsync(W.best, 0, (size_t)B * 8, st));
        DEFTET_LAUNCH(k_tc_best, grid, block, st, (const int *)lab, (const unsigned *)W.acc, T, min_size, W.best);
    }
    DEFTET_LAUNCH(k_tc_keep, grid, block, st, (const int *)lab, (const unsigned *)W.acc, (const unsigned long long *)W.best, T, min_size,
                  keep_largest, keep);
    if (labels) return finish(W, B, T, sizes, open, st);
    return DEFTET_OK;
}
