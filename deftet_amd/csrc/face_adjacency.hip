// face_adjacency.hip — the face edge adjacency layers.DefTet.forward calls per shape and the
// normal consistency that reads its table, for CDNA4 / gfx950.
//   A8  deftet_face_edge_adj_f32   layers/DefTet/tet_face_adj_m_idx/tet_face_adj_m_for.cu:15-130
#pragma clang fp contract(off)
#include "common.hpp"
#include "surface_batch.hpp"

namespace deftet {
namespace surf {

// ---------------------------------------------------------------------------- A8 face edge adjacency
__device__ __forceinline__ bool pos_equal(const float *a, const float *b)
{   // equal(), tet_face_adj_m_for.cu:26-35
    float diff = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float d = a[i] - b[i];
        if (d < 0) d = -d;
        diff += d;
    }
    return (double)diff <= 1e-15;
}

__global__ __launch_bounds__(256) void k_face_edge_adj(const float *__restrict__ face, float *__restrict__ adj, int F, int max_nei)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = f < F;
    float fa[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) fa[i] = face[(size_t)(live ? f : 0) * 9 + i];
    int found = live ? 0 : max_nei;
    for (int g = 0; g < F; ++g) {                                   // ascending g, :95
        if (__ballot(found < max_nei) == 0ull) break;               // every lane of the wave is full (:104-106)
        float fb[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) fb[i] = face[(size_t)g * 9 + i];   // wave-uniform -> scalar loads
        // check_share (:38-69) through the 3x3 vertex-equality matrix: equal() is a pure
        // function of its two vertices, so evaluating each pair once gives the same boolean
        bool E[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[i][j] = pos_equal(fa + 3 * i, fb + 3 * j);
        bool share = false;
#pragma unroll
        for (int ia = 0; ia < 3; ++ia)
#pragma unroll
            for (int ib = 0; ib < 3; ++ib) {
                const int ia2 = (ia + 1) % 3, ib2 = (ib + 1) % 3;
                share = share || (E[ia][ib] && E[ia2][ib2]) || (E[ia][ib2] && E[ia2][ib]);   // :60, :63
            }
        if (share && g != f && found < max_nei) {                   // :96, :100-103
            adj[(size_t)f * max_nei + found] = (float)g;
            ++found;
        }
    }
}

// --- A8, hash-based (exact): O(F) instead of O(F^2) --------------------------------------------------
// equal(a,b) (L1 distance <= 1e-15 in fp32) can only hold if, coordinate by coordinate, the two
// floats are bitwise identical or both "tiny" (|x| < 2^-24: one ulp there is still > 1e-15 above
// that magnitude, so distinct non-tiny floats differ by >= 7e-15).  NaN/Inf coordinates never
// compare equal (the difference is NaN).  So a NECESSARY condition for two faces to share an edge
// is equality of a 192-bit edge key built from per-coordinate keys (float bits, or one tag for
// all tiny values, or a unique tag for non-finite ones).  Edge records are chained per slot of a hash table
// on that key (one atomicExch each), and every face runs the EXACT check_share() only on the chain
// entries whose full key equals the key of one of its three edges, keeping the 30 smallest neighbour
// ids in ascending order.  Two launches for a whole batch of surfaces (rounds 1-2 radix-sorted the
// records by the 192-bit key: three 64-bit passes, ~38 launches per surface).
struct VKey { u32 x, y, z; };

__device__ __forceinline__ u32 coord_key(float v, u32 unique, bool &bad)
{
    const u32 b = __float_as_uint(v);
    if ((b & 0x7F800000u) == 0x7F800000u) { bad = true; return unique; }   // NaN / Inf: never equal to anything
    if (fabsf(v) < 5.9604645e-08f) return 0u;                                // tiny (|x| < 2^-24), includes +-0
    return b;
}
__device__ __forceinline__ VKey vertex_key(const float *v, u32 unique)
{
    bool bad = false;
    VKey k{coord_key(v[0], unique, bad), coord_key(v[1], unique, bad), coord_key(v[2], unique, bad)};
    if (bad) { k.x = 0xFFFFFFFFu; k.y = unique; k.z = 0u; }                 // 0xFFFFFFFF is itself a NaN pattern: no finite float has it
    return k;
}
__device__ __forceinline__ bool vkey_less(const VKey &a, const VKey &b)
{
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    return a.z < b.z;
}

// 64-bit hash of an edge key (a <= b in vkey order): the chains of a table slot hold every edge with that key plus
// the few that collide with it; keys are compared in full before check_share() runs.
__device__ __forceinline__ u64 mix64(u64 x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
struct EKey { VKey a, b; };
__device__ __forceinline__ EKey edge_key(const float *fa, int f, int e)
{
    VKey a = vertex_key(fa + 3 * e, (u32)(f * 3 + e)), b = vertex_key(fa + 3 * ((e + 1) % 3), (u32)(f * 3 + (e + 1) % 3));
    if (vkey_less(b, a)) { const VKey t = a; a = b; b = t; }
    return EKey{a, b};
}
__device__ __forceinline__ bool ekey_equal(const EKey &p, const EKey &q)
{
    return p.a.x == q.a.x && p.a.y == q.a.y && p.a.z == q.a.z && p.b.x == q.b.x && p.b.y == q.b.y && p.b.z == q.b.z;
}
__device__ __forceinline__ u32 ekey_slot(const EKey &k, u32 mask)
{
    u64 h = mix64(((u64)k.a.x << 32) | k.a.y);
    h = mix64(h ^ (((u64)k.a.z << 32) | k.b.x));
    h = mix64(h ^ (((u64)k.b.y << 32) | k.b.z));
    return (u32)h & mask;
}

constexpr int kA8Shapes = 32;          // shapes per launch (their face counts travel by value)
struct A8Counts { int n[kA8Shapes]; };

// every edge record r = 3 f + e of shape blockIdx.y is pushed onto the chain of its table slot (one atomicExch)
__global__ __launch_bounds__(256) void k_edge_insert(const float *__restrict__ face, int Fmax, A8Counts cnt, u32 mask, int *head, int *next)
{
    const int b = blockIdx.y, F = cnt.n[b];
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= F * 3) return;
    const int f = r / 3, e = r % 3;
    const EKey k = edge_key(face + ((size_t)b * Fmax + f) * 9, f, e);
    int *hb = head + (size_t)b * (mask + 1), *nb = next + (size_t)b * Fmax * 3;
    nb[r] = atomicExch(&hb[ekey_slot(k, mask)], r);
}

__device__ __forceinline__ bool check_share_exact(const float *fa, const float *fb)
{   // check_share, tet_face_adj_m_for.cu:38-69 (through the 3x3 vertex-equality matrix)
    bool E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E[i][j] = pos_equal(fa + 3 * i, fb + 3 * j);
    bool share = false;
#pragma unroll
    for (int ia = 0; ia < 3; ++ia)
#pragma unroll
        for (int ib = 0; ib < 3; ++ib) {
            const int ia2 = (ia + 1) % 3, ib2 = (ib + 1) % 3;
            share = share || (E[ia][ib] && E[ia2][ib2]) || (E[ia][ib2] && E[ia2][ib]);
        }
    return share;
}

constexpr int kMaxNeiFast = 32;        // the sorted path keeps its candidate list in registers/scratch

// every face walks the chains of its three edges: candidates with an identical 192-bit key get the EXACT check_share(),
// the max_nei smallest neighbour ids are kept in ascending order (the chain order does not matter)
__global__ __launch_bounds__(256) void k_face_neighbors(const float *__restrict__ face, int Fmax, A8Counts cnt, u32 mask,
                                                        const int *__restrict__ head, const int *__restrict__ next,
                                                        float *__restrict__ adj, int max_nei)
{
    const int b = blockIdx.y, F = cnt.n[b];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float *fbase = face + (size_t)b * Fmax * 9;
    const int *hb = head + (size_t)b * (mask + 1), *nxt = next + (size_t)b * Fmax * 3;
    float fa[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) fa[i] = fbase[(size_t)f * 9 + i];
    int nb[kMaxNeiFast];
    int n = 0;
    for (int e = 0; e < 3; ++e) {
        const EKey k = edge_key(fa, f, e);
        for (int rj = hb[ekey_slot(k, mask)]; rj >= 0; rj = nxt[rj]) {
            const int g = rj / 3;
            if (g == f) continue;
            if (n == max_nei && g > nb[n - 1]) continue;             // cannot be among the max_nei smallest
            float fb[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) fb[i] = fbase[(size_t)g * 9 + i];
            if (!ekey_equal(k, edge_key(fb, g, rj % 3))) continue;  // a hash collision, or another key in the same slot
            if (!check_share_exact(fa, fb)) continue;
            // insert g into the ascending list (no duplicates), keep the max_nei smallest
            int pos = 0;
            while (pos < n && nb[pos] < g) ++pos;
            if (pos < n && nb[pos] == g) continue;
            if (n < max_nei) ++n;
            for (int kk = n - 1; kk > pos; --kk) nb[kk] = nb[kk - 1];
            if (pos < n) nb[pos] = g;
        }
    }
    float *ab = adj + ((size_t)b * Fmax + f) * max_nei;
    for (int kk = 0; kk < n; ++kk) ab[kk] = (float)nb[kk];
}

// --- normal consistency on the A8 table (utils/mesh_utils.py:28-39 composed: unit normals, pairs, mean of 1 - cos) ----
// loss_b = mean over the valid entries (i, j = adj[i][k] >= 0) of 1 - <n_i, n_j>,  n = c / sqrt(|c|^2 + 1e-12),
// c = (v1 - v0) x (v2 - v0); 0 when there is no pair.  One workgroup per shape (fixed reduction order: deterministic
// forward); the backward adds the two adjacency directions with float atomics and chains through the normalisation and
// the cross product.  (The torch composition of the same thing gathers a [B, F, 30, 3] tensor and scatters it back in
// the backward: 1.8 ms per call at F = 4,056, B = 8, against ~0.03 ms here.)
constexpr int kNCThreads = 1024;
constexpr float kNormalEps = 1e-12f;

__device__ __forceinline__ void face_cross(const float *t, float *c)
{
    const float e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

__device__ __forceinline__ float block_sum(float v, float *sh)
{
#pragma unroll  // wave_sum's order (wave.hpp); written out, a call changes this kernel's instruction stream
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float tot = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) tot += sh[k];     // fixed order
    return tot;
}

constexpr int kNCLdsFaces = 4096;       // normals of a shape kept in LDS up to this many faces (48 KB)
__global__ __launch_bounds__(kNCThreads) void k_normal_consistency_fwd(const float *__restrict__ tri, const float *__restrict__ adj,
                                                                       const int *__restrict__ n_face, float *loss, float *nrm,
                                                                       float *count, int Fmax, int max_nei)
{
    __shared__ float sh[kNCThreads / 64];
    __shared__ float s_n[kNCLdsFaces * 3];
    const int b = blockIdx.x, F = min(n_face[b], Fmax);
    const float *tb = tri + (size_t)b * Fmax * 9, *ab = adj + (size_t)b * Fmax * max_nei;
    float *nb = nrm + (size_t)b * Fmax * 3;
    const bool lds = F <= kNCLdsFaces;                               // block-uniform
    for (int f = threadIdx.x; f < F; f += kNCThreads) {
        float t[9], c[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = tb[(size_t)f * 9 + k];
        face_cross(t, c);
        const float r = 1.0f / sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + kNormalEps);
        const float n0 = c[0] * r, n1 = c[1] * r, n2 = c[2] * r;
        nb[f * 3] = n0; nb[f * 3 + 1] = n1; nb[f * 3 + 2] = n2;     // kept for the backward
        if (lds) { s_n[f * 3] = n0; s_n[f * 3 + 1] = n1; s_n[f * 3 + 2] = n2; }
    }
    __syncthreads();                                                 // the shape's normals are this workgroup's own writes
    // One (face, neighbour slot) pair per thread and step: the table is read with consecutive addresses, the normals come
    // from LDS, and nothing in a step depends on the previous one, so the unrolled steps overlap.  (One face per thread
    // walking its row — 30 dependent loads behind a branch, four faces after each other — took 65 us for 8 x 4,056
    // faces; the pair loop with the normals gathered from global memory 91 us.)  Surfaces of more than 4,096 faces keep
    // the row walk.
    float s = 0.f, cnt = 0.f;
    if (lds) {
        const int nPair = F * max_nei;
#pragma unroll 4
        for (int i = threadIdx.x; i < nPair; i += kNCThreads) {
            const int f = i / max_nei;
            const float a = ab[i];
            const bool valid = a >= 0.f && a < (float)F;            // (entries outside [0, F) — or NaN — count as "no neighbour")
            const int j = valid ? (int)a : f;
            const float d = s_n[f * 3] * s_n[j * 3] + s_n[f * 3 + 1] * s_n[j * 3 + 1] + s_n[f * 3 + 2] * s_n[j * 3 + 2];
            s += valid ? 1.0f - d : 0.f;
            cnt += valid ? 1.0f : 0.f;
        }
    } else {
        for (int f = threadIdx.x; f < F; f += kNCThreads) {
            const float n0 = nb[f * 3], n1 = nb[f * 3 + 1], n2 = nb[f * 3 + 2];
            for (int k = 0; k < max_nei; ++k) {
                const float a = ab[(size_t)f * max_nei + k];
                if (!(a >= 0.f && a < (float)F)) continue;
                const int j = (int)a;
                s += 1.0f - (n0 * nb[j * 3] + n1 * nb[j * 3 + 1] + n2 * nb[j * 3 + 2]);
                cnt += 1.0f;
            }
        }
    }
    const float S = block_sum(s, sh), C = block_sum(cnt, sh);
    if (threadIdx.x == 0) {
        count[b] = C;
        loss[b] = C > 0.f ? S / C : 0.f;
    }
}

// backward, two launches over (faces, shapes) grids (one workgroup per shape, as the forward still is, ran its ~4 faces x 30
// dependent neighbour loads per thread unhidden: 0.13 ms per 8 shapes):
//  scatter: G_k = d(sum of 1 - <n_i, n_j>)/d n_k = -(sum over row k of n_j) - (sum over the rows i that list k of n_i),
//           formed in acc (zeroed by the caller) with float atomics — the table need not be symmetric (rows are cut at
//           max_nei entries);
//  final:   chain through the normalisation and the cross product, one lane per face.
__global__ __launch_bounds__(256) void k_normal_consistency_bwd_scatter(const float *__restrict__ adj, const int *__restrict__ n_face,
                                                                        const float *__restrict__ nrm, float *acc, int Fmax, int max_nei)
{
    const int b = blockIdx.y, F = min(n_face[b], Fmax);
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float *ab = adj + ((size_t)b * Fmax + f) * max_nei, *nb = nrm + (size_t)b * Fmax * 3;
    float *accb = acc + (size_t)b * Fmax * 3;
    const float n0 = nb[f * 3], n1 = nb[f * 3 + 1], n2 = nb[f * 3 + 2];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < max_nei; ++k) {
        const float a = ab[k];
        if (!(a >= 0.f && a < (float)F)) continue;                  // same validity rule as the forward
        const int j = (int)a;
        s0 += nb[j * 3]; s1 += nb[j * 3 + 1]; s2 += nb[j * 3 + 2];
        unsafeAtomicAdd(&accb[j * 3], -n0); unsafeAtomicAdd(&accb[j * 3 + 1], -n1); unsafeAtomicAdd(&accb[j * 3 + 2], -n2);
    }
    unsafeAtomicAdd(&accb[f * 3], -s0); unsafeAtomicAdd(&accb[f * 3 + 1], -s1); unsafeAtomicAdd(&accb[f * 3 + 2], -s2);
}

__global__ __launch_bounds__(256) void k_normal_consistency_bwd_final(const float *__restrict__ tri, const int *__restrict__ n_face,
                                                                      const float *__restrict__ count, const float *__restrict__ gloss,
                                                                      const float *__restrict__ acc, float *gtri, int Fmax)
{
    const int b = blockIdx.y, F = min(n_face[b], Fmax);
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= Fmax) return;
    const float C = count[b], w = C > 0.f ? gloss[b] / C : 0.f;
    float g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = 0.f;
    if (f < F) {
        const float *tb = tri + ((size_t)b * Fmax + f) * 9, *accf = acc + ((size_t)b * Fmax + f) * 3;
        float t[9], c[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = tb[k];
        face_cross(t, c);
        const float r2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + kNormalEps, r = 1.0f / sqrtf(r2);
        const float G[3] = {accf[0] * w, accf[1] * w, accf[2] * w};
        const float cg = (c[0] * G[0] + c[1] * G[1] + c[2] * G[2]) * r * r * r;          // n = c r:  dL/dc = G r - c (c.G) r^3
        const float dc[3] = {G[0] * r - c[0] * cg, G[1] * r - c[1] * cg, G[2] * r - c[2] * cg};
        const float e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
        // c = e1 x e2:  dL/de1 = e2 x dc,  dL/de2 = dc x e1
        const float d1[3] = {e2[1] * dc[2] - e2[2] * dc[1], e2[2] * dc[0] - e2[0] * dc[2], e2[0] * dc[1] - e2[1] * dc[0]};
        const float d2[3] = {dc[1] * e1[2] - dc[2] * e1[1], dc[2] * e1[0] - dc[0] * e1[2], dc[0] * e1[1] - dc[1] * e1[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) { g[k] = -(d1[k] + d2[k]); g[3 + k] = d1[k]; g[6 + k] = d2[k]; }
    }
    float *gb = gtri + ((size_t)b * Fmax + f) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) gb[k] = g[k];
}

}  // namespace surf
}  // namespace deftet

using namespace deftet;
using namespace deftet::surf;

static u32 a8_table_mask(int F)
{
    u32 n = 64;
    while (n < (u32)(F > 0 ? F : 0) * 6u) n <<= 1;                   // >= 2 slots per edge record
    return n - 1;
}
// the edge hash of every shape: chain heads per table slot, the next record per edge record (three per face)
struct A8Layout {
    size_t bytes;
    int *head, *next;
};
static A8Layout a8_layout(int B, int F_max, void *ws)
{
    A8Layout L{};
    const size_t b = (size_t)(B > 0 ? B : 0);
    Arena A(ws);
    L.head = A.take<int>(b * ((size_t)a8_table_mask(F_max) + 1));
    L.next = A.take<int>(b * (size_t)(F_max > 0 ? F_max : 0) * 3);
    L.bytes = A.end();
    return L;
}
extern "C" size_t deftet_face_edge_adj_workspace_bytes(int F) { return a8_layout(1, F, nullptr).bytes; }
extern "C" size_t deftet_face_edge_adj_ragged_workspace_bytes(int B, int F_max) { return a8_layout(B, F_max, nullptr).bytes; }

// A8 for a batch of surfaces with different face counts: face f32 [B, F_max, 3, 3], adj f32 [B, F_max, max_nei] (pre-filled
// with -1 by the caller), shape b has n_face_host[b] <= F_max faces (HOST integers); neighbour indices are local to the
// shape.  workspace == NULL (or max_nei > 32): the O(F^2) scan per shape; otherwise three launches per 32 shapes.
extern "C" int deftet_face_edge_adj_ragged_f32(const float *face, float *adj, int B, int F_max, const int *n_face_host, int max_nei,
                                               void *workspace, size_t wsb, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && F_max >= 0 && max_nei >= 0 && B <= 65535, "bad size");
    if (F_max >= (1 << 24)) return set_error(DEFTET_ELIMIT, "n_face=%d does not fit a float-encoded index", F_max);
    if (B == 0 || F_max == 0 || max_nei == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(face && adj && n_face_host, "null pointer");
    for (int b = 0; b < B; ++b) DEFTET_CHECK_ARG(n_face_host[b] >= 0 && n_face_host[b] <= F_max, "n_face[%d]=%d outside [0,%d]", b, n_face_host[b], F_max);
    hipStream_t st = as_stream(stream_);
    if (!workspace || max_nei > kMaxNeiFast) {
        for (int b = 0; b < B; ++b)
            if (n_face_host[b] > 0)
                DEFTET_LAUNCH(k_face_edge_adj, dim3(blocks_for(n_face_host[b], 256)), dim3(256), st, face + (size_t)b * F_max * 9,
                              adj + (size_t)b * F_max * max_nei, n_face_host[b], max_nei);
        return DEFTET_OK;
    }
    const A8Layout L = a8_layout(B, F_max, workspace);
    DEFTET_TRY(workspace_ok("deftet_face_edge_adj*", workspace, wsb, L.bytes));
    const u32 mask = a8_table_mask(F_max);
    DEFTET_HIP(hipMemsetAsync(L.head, 0xFF, (size_t)B * (mask + 1) * 4, st));   // -1 = empty chain
    for (int b0 = 0; b0 < B; b0 += kA8Shapes) {
        const int nb = std::min(kA8Shapes, B - b0);
        A8Counts cnt{};
        int fmax = 0;
        for (int i = 0; i < nb; ++i) { cnt.n[i] = n_face_host[b0 + i]; fmax = std::max(fmax, cnt.n[i]); }
        if (fmax == 0) continue;
        const float *fb = face + (size_t)b0 * F_max * 9;
        DEFTET_LAUNCH(k_edge_insert, dim3(blocks_for(fmax * 3, 256), nb), dim3(256), st, fb, F_max, cnt, mask, L.head + (size_t)b0 * (mask + 1),
                      L.next + (size_t)b0 * F_max * 3);
        DEFTET_LAUNCH(k_face_neighbors, dim3(blocks_for(fmax, 256), nb), dim3(256), st, fb, F_max, cnt, mask,
                      (const int *)(L.head + (size_t)b0 * (mask + 1)), (const int *)(L.next + (size_t)b0 * F_max * 3),
                      adj + (size_t)b0 * F_max * max_nei, max_nei);
    }
    return DEFTET_OK;
}

// workspace == NULL (or max_nei > 32): the scalar-stream brute force; otherwise the hash-based path.
extern "C" int deftet_face_edge_adj_f32(const float *face, float *adj, int F, int max_nei, void *workspace, size_t wsb,
                                        void *stream_)
{
    DEFTET_CHECK_ARG(F >= 0 && max_nei >= 0, "negative size");
    return deftet_face_edge_adj_ragged_f32(face, adj, 1, F, &F, max_nei, workspace, wsb, stream_);
}

// Normal consistency of B surfaces on their A8 tables (see k_normal_consistency_fwd).  tri f32 [B,F_max,3,3], adj f32
// [B,F_max,max_nei] (-1 padded, indices local to the shape), n_face int32 [B] ON THE DEVICE; loss f32 [B];
// nrm f32 [B,F_max,3] and count f32 [B] are saved for the backward.  grad_tri f32 [B,F_max,3,3] is fully overwritten
// (zeros for the padding faces); acc f32 [B,F_max,3] is scratch.
extern "C" int deftet_normal_consistency_fwd_f32(const float *tri, const float *adj, const int32_t *n_face, float *loss, float *nrm,
                                                 float *count, int B, int F_max, int max_nei, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && F_max >= 0 && max_nei >= 0, "bad size");
    if (B == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(loss && count && n_face && (F_max == 0 || (tri && nrm)) && (F_max == 0 || max_nei == 0 || adj), "null pointer");
    DEFTET_LAUNCH(k_normal_consistency_fwd, dim3(B), dim3(kNCThreads), as_stream(stream_), tri, adj, n_face, loss, nrm, count, F_max, max_nei);
    return DEFTET_OK;
}

extern "C" int deftet_normal_consistency_bwd_f32(const float *tri, const float *adj, const int32_t *n_face, const float *nrm,
                                                 const float *count, const float *grad_loss, float *grad_tri, float *acc, int B,
                                                 int F_max, int max_nei, void *stream_)
{
    DEFTET_CHECK_ARG(B >= 0 && F_max >= 0 && max_nei >= 0 && B <= 65535, "bad size");
    if (B == 0 || F_max == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(tri && n_face && nrm && count && grad_loss && grad_tri && acc && (max_nei == 0 || adj), "null pointer");
    hipStream_t st = as_stream(stream_);
    DEFTET_HIP(hipMemsetAsync(acc, 0, (size_t)B * F_max * 3 * sizeof(float), st));
    DEFTET_LAUNCH(k_normal_consistency_bwd_scatter, dim3(blocks_for(F_max, 256), B), dim3(256), st, adj, n_face, nrm, acc, F_max, max_nei);
    DEFTET_LAUNCH(k_normal_consistency_bwd_final, dim3(blocks_for(F_max, 256), B), dim3(256), st, tri, n_face, count, grad_loss, (const float *)acc,
                  grad_tri, F_max);
    return DEFTET_OK;
}
