// mesh_components.hip — connected components of a triangle list, their measures, and the mesh clean-up built on them: drop
// floaters and cavity shells, keep the largest piece, compact faces and vertices (gfx950; 420).  The mesh-side
// twin of tet_components.hip; the reference leaves this to trimesh on the host ("use trimesh to fix the surface").
//
// faces int64 [F,3] over V vertices, S >= 1 disjoint shapes on ascending face and vertex ranges.  Faces f and g are connected
// when they share an undirected vertex pair (connectivity 0, "edge": any number of faces may meet on the pair) or a vertex
// (connectivity 1).  The label of a component is its SMALLEST face index (union_find.hpp), so nothing depends on the schedule.
// Every per-component result stands at the label's index and is 0 elsewhere.  Launches of the labelling:
//
//   k_mc_keys        the 3 F incidences i = 3 f + k, local edge (f_k, f_k+1): key min V + max (64 bits), value 2 i + (f_k < f_k+1);
//                    an index outside [0, V) and a face that names a vertex twice are counted and get key 0, which joins nothing
//   radix_sort       stable: a run of equal keys is one edge, its incidences in ascending i
//   k_mc_init        parent[f] = f, the four integer accumulators zeroed
//   k_mc_hook_edge   every incidence of a run with its predecessor (edge mode)
//   k_mc_first / k_mc_hook_vertex   first[v] = the smallest face at v (integer atomicMin), every face with the first of its three
//                    corners (vertex mode)
//   k_mc_flatten     labels[f] = root(f); n_face summed per wave over the wave's distinct labels, one integer atomic each; count per shape
//   k_mc_stats       the run leader classifies the edge — one incidence: boundary; two running the same direction: misoriented;
//                    more than two: non-manifold — and adds 1 at the label of its face (no atomic at all on a closed oriented mesh)
//
// Measures (with verts): area = sum 1/2 |(b-a) x (c-a)|, volume = sum a . (b x c) / 6, every term in double from the widened fp32
// positions.  NO FLOAT ATOMICS: faces are sorted by (label, face) — stable, so a component's run is its faces ascending, led by
// the label itself; the run is cut into chunks of 256 counted FROM THE RUN'S OWN START; a chunk is summed in a fixed binary tree
// over the position inside the chunk (k_mc_chunks: the workgroup that holds the chunk's first face stages 512 terms in LDS, so
// where the chunk lies in the list does not matter); one lane adds a component's chunk sums in ascending order (k_mc_sums).  The
// sum of a component is a function of its own face list and of nothing else: not of the other components, the position in a
// concatenated list, the launch shape or the run.
//
// Clean-up, in this order, nothing read back in between: k_mc_select1 (drop_voids: closed and volume < 0; min_faces; min_area;
// the best size per shape by 64-bit integer max), k_mc_select2 (the smallest label among the best), k_mc_keep (keep flag per
// face; kept faces mark their corners), two scans, k_mc_offsets (the per-shape offsets next to the flags: the one read-back);
// then k_mc_fill_faces / k_mc_fill_verts write the compacted lists.  The gather verts[vertex_map] and its backward are one launch
// each; the map is injective and ascending, so the backward finds a vertex's row by bisection: plain copies, exact zeros elsewhere.
#pragma clang fp contract(off)
#include "common.hpp"
#include "prims.hpp"
#include "union_find.hpp"
#include "wave.hpp"

namespace deftet {
namespace mc {

typedef unsigned long long u64;
typedef unsigned int u32;
constexpr int kThreads = 256;
constexpr int kChunk = 256;                                                // faces per chunk of a component's sums
constexpr int kMaxAttr = 8;
constexpr int kFlagRange = 0, kFlagTwice = 1, kFlagBad = 2, kFlags = 3;    // flags: indices out of range, repeated vertices, union-find
using uf::find_root;
using uf::unite;

struct Layout {
    size_t bytes, n, sortBytes, scanBytes;
    u64 *k0, *k1;            // keys per incidence: unsorted, sorted
    u32 *v0, *v1;            // 2 i + direction: unsorted, sorted
    int *parent, *first;     // the forest [F]; the smallest face at every vertex [V]
    u32 *slab, *order;       // (label, face) sorted
    int *cstart;             // [F] at a label: where its run starts
    double *partA, *partV;   // [F] at a chunk's first position: the chunk's sums
    unsigned char *alive;    // [F] at a label: survives the thresholds
    u64 *best1;              // [S] the best size among the survivors, + 1
    int *best2;              // [S] the smallest label that has it
    int *fpos, *vpos;        // [F+1], [V+1] keep flags / vertex marks, scanned in place
    void *sortTmp, *scanTmp;
};

static Layout make_layout(int V, int F, int S, void *ws)
{
    Layout L{};
    const size_t f = (size_t)(F > 0 ? F : 0), v = (size_t)(V > 0 ? V : 0), s = (size_t)(S > 0 ? S : 0), n = 3 * f;
    L.n = n;
    Arena A(ws);
    L.k0 = A.take<u64>(n);
    L.k1 = A.take<u64>(n);
    L.v0 = A.take<u32>(n);
    L.v1 = A.take<u32>(n);
    L.parent = A.take<int>(f);
    L.first = A.take<int>(v);
    L.slab = A.take<u32>(f);
    L.order = A.take<u32>(f);
    L.cstart = A.take<int>(f);
    L.partA = A.take<double>(f);
    L.partV = A.take<double>(f);
    L.alive = A.take<unsigned char>(f);
    L.best1 = A.take<u64>(s);
    L.best2 = A.take<int>(s);
    L.fpos = A.take<int>(f + 1);
    L.vpos = A.take<int>(v + 1);
    const size_t s64 = prims::radix_sort_temp_bytes<u64, u32>(n), s32 = prims::radix_sort_temp_bytes<u32, u32>(f);
    L.sortBytes = s64 > s32 ? s64 : s32;
    L.sortTmp = A.take<char>(L.sortBytes);
    L.scanBytes = prims::scan_temp_bytes<int>((f > v ? f : v) + 1);
    L.scanTmp = A.take<char>(L.scanBytes);
    L.bytes = A.end();
    return L;
}

// the shape of face f: the last s in [0, S) with off[s] <= f (empty shapes have equal offsets and are passed over)
__device__ __forceinline__ int shape_of(const int *__restrict__ off, int S, int f)
{
    int lo = 0, hi = S;
    for (int k = 0; k < 32 && hi - lo > 1; ++k) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------- labelling
__global__ __launch_bounds__(kThreads) void k_mc_keys(const long long *__restrict__ faces, long long n, int V, u64 *keys, u32 *vals, int *flags)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long f = i / 3;
    const int k = (int)(i - 3 * f);
    const long long a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3];
    u64 key = 0ull;
    if (a < 0 || a >= V) atomicAdd(flags + kFlagRange, 1);                    // every corner is the start of one incidence: counted once
    else if (b < 0 || b >= V) {}                                              // (counted at its own incidence; never followed)
    else if (a == b) atomicAdd(flags + kFlagTwice, 1);
    else key = (u64)(a < b ? a : b) * (u64)V + (u64)(a < b ? b : a);
    keys[i] = key;
    vals[i] = ((u32)i << 1) | (a < b ? 1u : 0u);
}

__global__ __launch_bounds__(kThreads) void k_mc_init(int F, int *parent, int *nface, int *bnd, int *nm, int *mis)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    parent[f] = f;
    nface[f] = 0;
    bnd[f] = 0;
    nm[f] = 0;
    mis[f] = 0;
}

__global__ __launch_bounds__(kThreads) void k_mc_hook_edge(const u64 *__restrict__ key, const u32 *__restrict__ val, long long n, int F,
                                                           int *parent, int *flags)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < 1 || i >= n) return;
    const u64 k = key[i];
    if (k == 0ull || key[i - 1] != k) return;
    const u32 fa = (val[i] >> 1) / 3u, fb = (val[i - 1] >> 1) / 3u;
    if (fa >= (u32)F || fb >= (u32)F || fa == fb) return;
    unite(parent, (int)fa, (int)fb, 2 * F + 2, flags + kFlagBad);
}

__global__ __launch_bounds__(kThreads) void k_mc_first(const long long *__restrict__ faces, long long n, int V, int *first)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long a = faces[i];
    if (a >= 0 && a < V) atomicMin(first + a, (int)(i / 3));
}

__global__ __launch_bounds__(kThreads) void k_mc_hook_vertex(const long long *__restrict__ faces, int F, int V, const int *__restrict__ first,
                                                             int *parent, int *flags)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long a = faces[3 * (long long)f + k];
        if (a < 0 || a >= V) continue;
        const int u = first[a];
        if (u < 0 || u >= F || u == f) continue;
        unite(parent, f, u, 2 * F + 2, flags + kFlagBad);
    }
}

__global__ __launch_bounds__(kThreads) void k_mc_flatten(int F, int *parent, int *labels, int *nface, const int *__restrict__ face_off, int S,
                                                         int *count, int *flags)
{
    const int f = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
    int L = -1;
    if (f < F) {
        L = find_root(parent, f, flags + kFlagBad);
        labels[f] = L;
    }
    // one add per distinct label of the wave (every lane of the wave is here: no lane has returned)
    unsigned long long todo = __ballot(L >= 0);
    for (int k = 0; k < 64 && todo; ++k) {
        const int leader = __ffsll((long long)todo) - 1;
        const int Lf = __shfl(L, leader);
        const unsigned long long same = __ballot(L == Lf);                    // (Lf >= 0: lanes without a label never match)
        if (lane == leader) atomicAdd(nface + Lf, (int)__popcll(same));
        todo &= ~same;
    }
    if (L >= 0 && L == f) atomicAdd(count + shape_of(face_off, S, f), 1);
}

__global__ __launch_bounds__(kThreads) void k_mc_stats(const u64 *__restrict__ key, const u32 *__restrict__ val, long long n, int F,
                                                       const int *__restrict__ labels, int *bnd, int *nm, int *mis)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if (k == 0ull || (i > 0 && key[i - 1] == k)) return;                      // the run leader only
    const bool two = i + 1 < n && key[i + 1] == k, three = two && i + 2 < n && key[i + 2] == k;
    int *to = nullptr;
    if (!two) to = bnd;
    else if (three) to = nm;
    else if (((val[i] ^ val[i + 1]) & 1u) == 0u) to = mis;
    if (!to) return;
    const u32 f = (val[i] >> 1) / 3u;
    if (f >= (u32)F) return;
    const int L = labels[f];
    if (L >= 0 && L < F) atomicAdd(to + L, 1);
}

// ---------------------------------------------------------------------------- measures
__global__ __launch_bounds__(kThreads) void k_mc_starts(const u32 *__restrict__ slab, int F, int *cstart)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= F) return;
    const u32 L = slab[p];
    if (L < (u32)F && (p == 0 || slab[p - 1] != L)) cstart[L] = p;
}

__device__ __forceinline__ void face_terms(const long long *__restrict__ faces, const float *__restrict__ verts, int f, int V, double &area,
                                           double &vol)
{
    area = 0.0;
    vol = 0.0;
    const long long ia = faces[3 * (long long)f], ib = faces[3 * (long long)f + 1], ic = faces[3 * (long long)f + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return;
    double a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)verts[3 * ia + k];
        b[k] = (double)verts[3 * ib + k];
        c[k] = (double)verts[3 * ic + k];
    }
    const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    area = 0.5 * sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double x[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    vol = (a[0] * x[0] + a[1] * x[1] + a[2] * x[2]) / 6.0;
}

// workgroup w owns the chunks whose first face stands at a sorted position in [256 w, 256 w + 256): all of such a chunk lies in
// the 512 positions from 256 w, which the workgroup stages.  Level k of the tree: position j inside the component with
// j mod 2^(k+1) = 0 takes the term at j + 2^k when the component has one (j mod 256 = 0 ends with its chunk's sum).
__global__ __launch_bounds__(kThreads) void k_mc_chunks(const long long *__restrict__ faces, const float *__restrict__ verts,
                                                        const u32 *__restrict__ slab, const u32 *__restrict__ order,
                                                        const int *__restrict__ cstart, int F, int V, double *partA, double *partV)
{
    __shared__ double sa[2 * kChunk], sv[2 * kChunk];
    __shared__ int sj[2 * kChunk];
    const int base = blockIdx.x * kChunk;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = threadIdx.x + h * kChunk, p = base + s;
        int j = -1;
        double a = 0.0, v = 0.0;
        if (p < F) {
            const u32 L = slab[p], f = order[p];
            if (L < (u32)F && f < (u32)F) {
                const int st = cstart[L];
                if (st >= 0 && st <= p) {
                    j = p - st;
                    face_terms(faces, verts, (int)f, V, a, v);
                }
            }
        }
        sj[s] = j;
        sa[s] = a;
        sv[s] = v;
    }
#pragma unroll
    for (int stride = 1; stride < kChunk; stride <<= 1) {
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = threadIdx.x + h * kChunk, j = sj[s];
            if (j >= 0 && (j & (2 * stride - 1)) == 0 && s + stride < 2 * kChunk && sj[s + stride] == j + stride) {
                sa[s] = sa[s] + sa[s + stride];
                sv[s] = sv[s] + sv[s + stride];
            }
        }
    }
    __syncthreads();
    const int s = threadIdx.x, p = base + s;
    if (p < F && sj[s] >= 0 && (sj[s] & (kChunk - 1)) == 0) {
        partA[p] = sa[s];
        partV[p] = sv[s];
    }
}

// the lane at a component's first position adds its chunk sums in ascending order (eight loads in flight, one accumulator)
__global__ __launch_bounds__(kThreads) void k_mc_sums(const u32 *__restrict__ slab, const int *__restrict__ cstart, const int *__restrict__ nface,
                                                      int F, const double *__restrict__ partA, const double *__restrict__ partV, double *area,
                                                      double *volume)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= F) return;
    const u32 L = slab[p];
    if (L >= (u32)F || cstart[L] != p) return;
    const int n = min(max(nface[L], 1), F - p), nch = (n + kChunk - 1) / kChunk;
    double a = partA[p], v = partV[p];
    for (int c0 = 1; c0 < nch; c0 += 8) {
        double xa[8], xv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = min(c0 + k, nch - 1);                               // clamped, unconditional
            xa[k] = partA[p + c * kChunk];
            xv[k] = partV[p + c * kChunk];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c0 + k < nch) {
                a = a + xa[k];
                v = v + xv[k];
            }
    }
    area[L] = a;
    volume[L] = v;
}

// ---------------------------------------------------------------------------- selection and compaction
struct Select {
    int keep_largest, min_faces, drop_voids, by_area;
    double min_area;
};

__device__ __forceinline__ u64 size_key(const Select &o, const int *__restrict__ nface, const double *__restrict__ area, int L)
{
    // area >= +0: the bits of a non-negative double order like the number; + 1 keeps 0 for "nothing survives"
    return o.by_area ? (u64)__double_as_longlong(area[L]) + 1ull : (u64)(unsigned)nface[L];
}

__global__ __launch_bounds__(kThreads) void k_mc_select1(int F, const int *__restrict__ labels, const int *__restrict__ nface,
                                                         const int *__restrict__ bnd, const int *__restrict__ nm, const int *__restrict__ mis,
                                                         const double *__restrict__ area, const double *__restrict__ volume, Select o,
                                                         const int *__restrict__ face_off, int S, unsigned char *alive, u64 *best1)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    bool a = labels[f] == f;
    if (a && o.drop_voids) a = !(bnd[f] == 0 && nm[f] == 0 && mis[f] == 0 && volume[f] < 0.0);
    if (a && o.min_faces > 0) a = nface[f] >= o.min_faces;
    if (a && o.min_area > 0.0) a = !(area[f] < o.min_area);
    alive[f] = a ? 1 : 0;
    if (a && o.keep_largest) atomicMax(best1 + shape_of(face_off, S, f), size_key(o, nface, area, f));
}

__global__ __launch_bounds__(kThreads) void k_mc_select2(int F, const int *__restrict__ labels, const int *__restrict__ nface,
                                                         const double *__restrict__ area, Select o, const int *__restrict__ face_off, int S,
                                                         const unsigned char *__restrict__ alive, const u64 *__restrict__ best1, int *best2)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F || labels[f] != f || !alive[f]) return;
    const int s = shape_of(face_off, S, f);
    if (size_key(o, nface, area, f) == best1[s]) atomicMin(best2 + s, f);
}

__global__ __launch_bounds__(kThreads) void k_mc_keep(const long long *__restrict__ faces, int F, int V, const int *__restrict__ labels,
                                                      const unsigned char *__restrict__ alive, const int *__restrict__ best2,
                                                      const int *__restrict__ face_off, int S, int keep_largest, int *fflag, int *vmark)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f > F) return;
    bool k = false;
    if (f < F) {
        const int L = labels[f];
        k = L >= 0 && L < F && alive[L] != 0;
        if (k && keep_largest) k = best2[shape_of(face_off, S, L)] == L;
        if (k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long a = faces[3 * (long long)f + c];
                if (a >= 0 && a < V) vmark[a] = 1;                            // (the same value from every lane that writes)
            }
    }
    fflag[f] = k ? 1 : 0;                                                     // entry F: the scan's total
}

// counts[kFlags + s] = kept faces before shape s, counts[kFlags + S + 1 + s] = kept vertices before it (s = 0 .. S)
__global__ __launch_bounds__(kThreads) void k_mc_offsets(const int *__restrict__ fpos, const int *__restrict__ vpos,
                                                         const int *__restrict__ face_off, const int *__restrict__ vert_off, int S, int F, int V,
                                                         int *counts)
{
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s > S) return;
    counts[kFlags + s] = fpos[min(max(face_off[s], 0), F)];
    counts[kFlags + S + 1 + s] = vpos[min(max(vert_off[s], 0), V)];
}

__global__ __launch_bounds__(kThreads) void k_mc_fill_faces(const long long *__restrict__ faces, int F, int V, const int *__restrict__ fpos,
                                                            const int *__restrict__ vpos, const int *__restrict__ face_off,
                                                            const int *__restrict__ vert_off, int S, long long Fk, long long *faces_out,
                                                            long long *face_map)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int r = fpos[f];
    if (fpos[f + 1] == r || r < 0 || r >= Fk) return;                         // not kept
    const int s = shape_of(face_off, S, f);
    const int v0 = vpos[min(max(vert_off[s], 0), V)];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long a = faces[3 * (long long)f + c];
        faces_out[3 * (long long)r + c] = a >= 0 && a < V ? (long long)(vpos[a] - v0) : -1;
    }
    face_map[r] = f;
}

__global__ __launch_bounds__(kThreads) void k_mc_fill_verts(int V, const int *__restrict__ vpos, long long Vk, long long *vertex_map)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const int r = vpos[v];
    if (vpos[v + 1] == r || r < 0 || r >= Vk) return;
    vertex_map[r] = v;
}

// ---------------------------------------------------------------------------- gather
__global__ __launch_bounds__(kThreads) void k_mc_gather_fwd(const float *__restrict__ verts, const float *__restrict__ attr, int C,
                                                            const long long *__restrict__ map, int V, int Vk, float *out_verts, float *out_attr)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= Vk) return;
    const long long v = map[r];
    const bool ok = v >= 0 && v < V;
    if (out_verts)
#pragma unroll
        for (int k = 0; k < 3; ++k) out_verts[3 * (size_t)r + k] = ok ? verts[3 * (size_t)v + k] : quiet_nan();
    if (out_attr)
        for (int k = 0; k < C; ++k) out_attr[(size_t)r * C + k] = ok ? attr[(size_t)v * C + k] : quiet_nan();
}

// one lane per OLD vertex: its row of the map by bisection (the map ascends), a copy of that gradient row, or zeros
__global__ __launch_bounds__(kThreads) void k_mc_gather_bwd(const float *__restrict__ g_verts, const float *__restrict__ g_attr, int C,
                                                            const long long *__restrict__ map, int V, int Vk, float *grad_verts, float *grad_attr)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    int lo = 0, hi = Vk;                                                      // first r with map[r] >= v
    for (int k = 0; k < 32 && lo < hi; ++k) {
        const int mid = (lo + hi) >> 1;
        if (map[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    const bool hit = lo < Vk && map[lo] == v;
    if (grad_verts)
#pragma unroll
        for (int k = 0; k < 3; ++k) grad_verts[3 * (size_t)v + k] = hit ? g_verts[3 * (size_t)lo + k] : 0.0f;
    if (grad_attr)
        for (int k = 0; k < C; ++k) grad_attr[(size_t)v * C + k] = hit ? g_attr[(size_t)lo * C + k] : 0.0f;
}

// ---------------------------------------------------------------------------- host side
struct Out {
    int32_t *labels, *nface, *bnd, *nm, *mis, *count;
    double *area, *volume;
};

static int bits_for(u64 top)                                                  // bits that hold every value below `top`
{
    int bits = 1;
    while (bits < 64 && (top - 1) >> bits) ++bits;
    return bits;
}

static int check_mesh(const char *who, const void *faces, int F, int V, const void *face_off, int S, int connectivity, const Out &o,
                      const void *flags, void *workspace, size_t wsb, Layout &L)
{
    DEFTET_CHECK_ARG(F > 0 && V > 0, "%s: n_face=%d, n_vertex=%d must be positive", who, F, V);
    DEFTET_CHECK_ARG(3LL * F < 2147483648LL, "%s: 3 n_face = %lld does not fit 31 bits", who, 3LL * F);
    DEFTET_CHECK_ARG(S >= 1 && S <= 1048576, "%s: n_shape=%d outside 1..1048576", who, S);
    DEFTET_CHECK_ARG(connectivity == 0 || connectivity == 1, "%s: connectivity=%d is neither 0 (edge) nor 1 (vertex)", who, connectivity);
    DEFTET_CHECK_ARG(faces && face_off, "%s: null pointer: faces / face_offsets", who);
    DEFTET_CHECK_ARG(o.labels && o.nface && o.bnd && o.nm && o.mis && o.count && flags, "%s: null pointer: an integer result or the flags", who);
    DEFTET_CHECK_ARG((o.area == nullptr) == (o.volume == nullptr), "%s: area and volume go together", who);
    L = make_layout(V, F, S, workspace);
    DEFTET_TRY(workspace_ok(who, workspace, wsb, L.bytes));
    return DEFTET_OK;
}

// labels, the integer results, count and flags[0..2]; with verts also area and volume
static int label_and_measure(const int64_t *faces, int F, int V, const float *verts, const int32_t *face_off, int S, int connectivity,
                             const Out &o, int32_t *flags, const Layout &L, hipStream_t st)
{
    const long long n = (long long)L.n;
    const dim3 block(kThreads), gridN(blocks_for((size_t)n, kThreads)), gridF(blocks_for(F, kThreads));
    const long long *fc = (const long long *)faces;
    DEFTET_HIP(hipMemsetAsync(flags, 0, kFlags * 4, st));
    DEFTET_HIP(hipMemsetAsync(o.count, 0, (size_t)S * 4, st));
    DEFTET_LAUNCH(k_mc_keys, gridN, block, st, fc, n, V, L.k0, L.v0, (int *)flags);
    DEFTET_TRY((prims::radix_sort<u64, u32>(L.k0, L.k1, L.v0, L.v1, (size_t)n, bits_for((u64)V * (u64)V), L.sortTmp, L.sortBytes, st)));
    DEFTET_LAUNCH(k_mc_init, gridF, block, st, F, L.parent, (int *)o.nface, (int *)o.bnd, (int *)o.nm, (int *)o.mis);
    if (connectivity == 0) {
        DEFTET_LAUNCH(k_mc_hook_edge, gridN, block, st, (const u64 *)L.k1, (const u32 *)L.v1, n, F, L.parent, (int *)flags);
    } else {
        DEFTET_HIP(hipMemsetAsync(L.first, 0x7F, (size_t)V * 4, st));       // 0x7F7F7F7F: above every face index
        DEFTET_LAUNCH(k_mc_first, gridN, block, st, fc, n, V, L.first);
        DEFTET_LAUNCH(k_mc_hook_vertex, gridF, block, st, fc, F, V, (const int *)L.first, L.parent, (int *)flags);
    }
    DEFTET_LAUNCH(k_mc_flatten, gridF, block, st, F, L.parent, (int *)o.labels, (int *)o.nface, (const int *)face_off, S, (int *)o.count,
                  (int *)flags);
    DEFTET_LAUNCH(k_mc_stats, gridN, block, st, (const u64 *)L.k1, (const u32 *)L.v1, n, F, (const int *)o.labels, (int *)o.bnd, (int *)o.nm,
                  (int *)o.mis);
    if (!verts) return DEFTET_OK;
    DEFTET_HIP(hipMemsetAsync(o.area, 0, (size_t)F * 8, st));
    DEFTET_HIP(hipMemsetAsync(o.volume, 0, (size_t)F * 8, st));
    DEFTET_TRY((prims::radix_sort_from<u32, u32>(prims::PtrLoad<u32>{(const u32 *)o.labels}, L.slab, prims::IotaLoad{}, L.order, (size_t)F,
                                                  bits_for((u64)F), L.sortTmp, L.sortBytes, st)));
    DEFTET_HIP(hipMemsetAsync(L.cstart, 0xFF, (size_t)F * 4, st));          // -1: no run starts here
    DEFTET_LAUNCH(k_mc_starts, gridF, block, st, (const u32 *)L.slab, F, L.cstart);
    DEFTET_LAUNCH(k_mc_chunks, dim3(blocks_for(F, kChunk)), dim3(kChunk), st, fc, verts, (const u32 *)L.slab, (const u32 *)L.order,
                  (const int *)L.cstart, F, V, L.partA, L.partV);
    DEFTET_LAUNCH(k_mc_sums, gridF, block, st, (const u32 *)L.slab, (const int *)L.cstart, (const int *)o.nface, F, (const double *)L.partA,
                  (const double *)L.partV, o.area, o.volume);
    return DEFTET_OK;
}

static int check_gather(const char *who, int C, const void *map, int V, int Vk)
{
    DEFTET_CHECK_ARG(V > 0 && Vk > 0 && Vk <= V, "%s: n_vertex=%d must be positive and n_vertex_out=%d in 1..n_vertex", who, V, Vk);
    DEFTET_CHECK_ARG(C >= 0 && C <= kMaxAttr, "%s: n_attr=%d outside 0..8", who, C);
    DEFTET_CHECK_ARG(map, "%s: null pointer: vertex_map", who);
    return DEFTET_OK;
}

}  // namespace mc
}  // namespace deftet

using namespace deftet;
using namespace deftet::mc;

extern "C" size_t deftet_mesh_components_workspace_bytes(int V, int F, int S)
{
    return V <= 0 || F <= 0 || S <= 0 || 3LL * F >= 2147483648LL ? 256 : make_layout(V, F, S, nullptr).bytes;
}

extern "C" int deftet_mesh_components_i64(const int64_t *faces_fx3, int F, int V, const float *verts_vx3, const int32_t *face_offsets, int S,
                                          int connectivity, int32_t *labels, int32_t *n_face, int32_t *boundary_edges,
                                          int32_t *nonmanifold_edges, int32_t *misoriented_edges, double *area, double *volume, int32_t *count,
                                          int32_t *flags, void *workspace, size_t wsb, void *stream_)
{
    const Out o{labels, n_face, boundary_edges, nonmanifold_edges, misoriented_edges, count, area, volume};
    Layout L;
    DEFTET_TRY(check_mesh("mesh_components", faces_fx3, F, V, face_offsets, S, connectivity, o, flags, workspace, wsb, L));
    DEFTET_CHECK_ARG((verts_vx3 == nullptr) == (area == nullptr), "mesh_components: verts goes with area and volume");
    return label_and_measure(faces_fx3, F, V, verts_vx3, face_offsets, S, connectivity, o, flags, L, as_stream(stream_));
}

extern "C" int deftet_mesh_cleanup_count_i64(const int64_t *faces_fx3, int F, int V, const float *verts_vx3, const int32_t *face_offsets,
                                             const int32_t *vertex_offsets, int S, int connectivity, int keep_largest, int min_faces,
                                             double min_area, int drop_voids, int largest_by, int32_t *labels, int32_t *n_face,
                                             int32_t *boundary_edges, int32_t *nonmanifold_edges, int32_t *misoriented_edges, double *area,
                                             double *volume, int32_t *count, int32_t *counts, void *workspace, size_t wsb, void *stream_)
{
    const Out o{labels, n_face, boundary_edges, nonmanifold_edges, misoriented_edges, count, area, volume};
    Layout L;
    DEFTET_TRY(check_mesh("mesh_cleanup", faces_fx3, F, V, face_offsets, S, connectivity, o, counts, workspace, wsb, L));
    DEFTET_CHECK_ARG(vertex_offsets, "mesh_cleanup: null pointer: vertex_offsets");
    DEFTET_CHECK_ARG((verts_vx3 == nullptr) == (area == nullptr), "mesh_cleanup: verts goes with area and volume");
    DEFTET_CHECK_ARG(min_faces >= 0 && min_area >= 0.0, "mesh_cleanup: min_faces=%d or min_area=%g is negative (or not a number)", min_faces, min_area);
    DEFTET_CHECK_ARG(largest_by == 0 || largest_by == 1, "mesh_cleanup: largest_by=%d is neither 0 (faces) nor 1 (area)", largest_by);
    const Select sel{keep_largest ? 1 : 0, min_faces, drop_voids ? 1 : 0, largest_by, min_area};
    DEFTET_CHECK_ARG(verts_vx3 || !(sel.drop_voids || sel.min_area > 0.0 || (sel.keep_largest && sel.by_area)),
                     "mesh_cleanup: drop_voids, min_area and largest_by=area need verts");
    hipStream_t st = as_stream(stream_);
    DEFTET_TRY(label_and_measure(faces_fx3, F, V, verts_vx3, face_offsets, S, connectivity, o, counts, L, st));
    const dim3 block(kThreads), gridF(blocks_for(F, kThreads));
    if (sel.keep_largest) {
        DEFTET_HIP(hipMemsetAsync(L.best1, 0, (size_t)S * 8, st));
        DEFTET_HIP(hipMemsetAsync(L.best2, 0x7F, (size_t)S * 4, st));
    }
    DEFTET_LAUNCH(k_mc_select1, gridF, block, st, F, (const int *)labels, (const int *)n_face, (const int *)boundary_edges,
                  (const int *)nonmanifold_edges, (const int *)misoriented_edges, (const double *)area, (const double *)volume, sel,
                  (const int *)face_offsets, S, L.alive, L.best1);
    if (sel.keep_largest)
        DEFTET_LAUNCH(k_mc_select2, gridF, block, st, F, (const int *)labels, (const int *)n_face, (const double *)area, sel,
                      (const int *)face_offsets, S, (const unsigned char *)L.alive, (const u64 *)L.best1, L.best2);
    DEFTET_HIP(hipMemsetAsync(L.vpos, 0, ((size_t)V + 1) * 4, st));
    DEFTET_LAUNCH(k_mc_keep, dim3(blocks_for((size_t)F + 1, kThreads)), block, st, (const long long *)faces_fx3, F, V, (const int *)labels,
                  (const unsigned char *)L.alive, (const int *)L.best2, (const int *)face_offsets, S, sel.keep_largest, L.fpos, L.vpos);
    DEFTET_TRY((prims::scan<int, prims::Plus, true>(L.fpos, L.fpos, (size_t)F + 1, 0, prims::Plus(), L.scanTmp, L.scanBytes, st)));
    DEFTET_TRY((prims::scan<int, prims::Plus, true>(L.vpos, L.vpos, (size_t)V + 1, 0, prims::Plus(), L.scanTmp, L.scanBytes, st)));
    DEFTET_LAUNCH(k_mc_offsets, dim3(blocks_for((size_t)S + 1, kThreads)), block, st, (const int *)L.fpos, (const int *)L.vpos,
                  (const int *)face_offsets, (const int *)vertex_offsets, S, F, V, (int *)counts);
    return DEFTET_OK;
}

extern "C" int deftet_mesh_cleanup_fill_i64(const int64_t *faces_fx3, int F, int V, const int32_t *face_offsets, const int32_t *vertex_offsets,
                                            int S, long long n_face_out, long long n_vertex_out, int64_t *faces_out, int64_t *vertex_map,
                                            int64_t *face_map, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_CHECK_ARG(F > 0 && V > 0 && 3LL * F < 2147483648LL, "mesh_cleanup: n_face=%d, n_vertex=%d must be positive and 3 n_face fit 31 bits", F, V);
    DEFTET_CHECK_ARG(S >= 1 && S <= 1048576, "mesh_cleanup: n_shape=%d outside 1..1048576", S);
    DEFTET_CHECK_ARG(n_face_out > 0 && n_face_out <= F && n_vertex_out > 0 && n_vertex_out <= V,
                     "mesh_cleanup: n_face_out=%lld outside 1..n_face or n_vertex_out=%lld outside 1..n_vertex", n_face_out, n_vertex_out);
    DEFTET_CHECK_ARG(faces_fx3 && face_offsets && vertex_offsets && faces_out && vertex_map && face_map, "mesh_cleanup: null pointer");
    const Layout L = make_layout(V, F, S, workspace);
    DEFTET_TRY(workspace_ok("mesh_cleanup", workspace, wsb, L.bytes));
    hipStream_t st = as_stream(stream_);
    DEFTET_LAUNCH(k_mc_fill_faces, dim3(blocks_for(F, kThreads)), dim3(kThreads), st, (const long long *)faces_fx3, F, V, (const int *)L.fpos,
                  (const int *)L.vpos, (const int *)face_offsets, (const int *)vertex_offsets, S, n_face_out, (long long *)faces_out,
                  (long long *)face_map);
    DEFTET_LAUNCH(k_mc_fill_verts, dim3(blocks_for(V, kThreads)), dim3(kThreads), st, V, (const int *)L.vpos, n_vertex_out, (long long *)vertex_map);
    return DEFTET_OK;
}

extern "C" int deftet_mesh_gather_fwd_f32(const float *verts_vx3, const float *attr_vxc, int C, const int64_t *vertex_map, int V, int Vk,
                                          float *out_verts, float *out_attr, void *stream_)
{
    DEFTET_TRY(check_gather("mesh_gather", C, vertex_map, V, Vk));
    DEFTET_CHECK_ARG((attr_vxc == nullptr) == (C == 0) && (attr_vxc == nullptr) == (out_attr == nullptr),
                     "mesh_gather: attr, n_attr=%d and out_attr do not go together", C);
    DEFTET_CHECK_ARG(verts_vx3 && out_verts, "mesh_gather: null pointer: verts / out_verts");
    DEFTET_LAUNCH(k_mc_gather_fwd, dim3(blocks_for(Vk, kThreads)), dim3(kThreads), as_stream(stream_), verts_vx3, attr_vxc, C,
                  (const long long *)vertex_map, V, Vk, out_verts, out_attr);
    return DEFTET_OK;
}

extern "C" int deftet_mesh_gather_bwd_f32(const float *grad_out_verts, const float *grad_out_attr, int C, const int64_t *vertex_map, int V,
                                          int Vk, float *grad_verts, float *grad_attr, void *stream_)
{
    DEFTET_TRY(check_gather("mesh_gather_bwd", C, vertex_map, V, Vk));
    DEFTET_CHECK_ARG((grad_out_verts == nullptr) == (grad_verts == nullptr) && (grad_out_attr == nullptr) == (grad_attr == nullptr),
                     "mesh_gather_bwd: every gradient read goes with the gradient written from it");
    DEFTET_CHECK_ARG(grad_verts || grad_attr, "mesh_gather_bwd: null pointer: every output");
    DEFTET_CHECK_ARG(!grad_attr || C > 0, "mesh_gather_bwd: grad_attr without attributes");
    DEFTET_LAUNCH(k_mc_gather_bwd, dim3(blocks_for(V, kThreads)), dim3(kThreads), as_stream(stream_), grad_out_verts, grad_out_attr, C,
                  (const long long *)vertex_map, V, Vk, grad_verts, grad_attr);
    return DEFTET_OK;
}
