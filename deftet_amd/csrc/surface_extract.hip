// surface_extract.hip — triangle surface of a per-tet occupancy: soup rows, per-corner attributes, (tet, local face) index and
// indexed (welded) faces, for a whole batch (gfx950).
//
//   BINARY     utils/tet_utils.py:427-471 (get_face_use_occ): four sparse matmuls + has_adj + boolean-mask indexing per shape
//   THRESHOLD  diff_render/diftet_6_subdiv/3_model/utils_tetsv.py:79-128, 145-225 (get_face_use_occ / _color): scipy float64
//              products and numpy masks on the host
//   fused max  3_model/deftet.py:522-523 (saveobj): occ[t] = max of the four corner weights
//
// Local face i of tet (A,B,C,D) has the corners (i, i^1, i^2): a = [A,B,C,D][i], b = [B,A,D,C][i], c = [C,D,A,B][i].  Rows come in
// ascending (t, i) order per shape.  The neighbour table is indexed by LOCAL FACE: nbr[t][i] = the tet across face i, -1 at the
// grid boundary (deftet_tet_face_neighbours_i64; built once per topology, an int32 copy of 16 bytes per tet feeds the kernels).
//
// Two phases, like every dynamic-size entry of this library.  Count: one lane per tet evaluates face_mask(), four wave ballots
// (one per local face) and their popcounts give the wave's total, the workgroup writes one total; an exclusive scan over the
// B * nblk + 1 totals (prims.hpp) gives every workgroup's first row, and offsets[b] = the first row of shape b.  Fill: a
// workgroup whose total is zero leaves after two loads (the r = 0.3 sphere touches 30 % of the workgroups at res 70); the others
// evaluate face_mask() again, rank their faces with the same ballots, stage the (lane, local face) of every row in LDS in rank
// order, and then walk the workgroup's CONTIGUOUS span of every output with consecutive threads on consecutive words — each
// word finds its source through the staged descriptor, so stores are full lines whatever the row width (36 bytes, 12 C bytes,
// 16 and 24 bytes) and the LDS footprint is 2 KB instead of 36 + 96 KB of staged rows at C = 8.
#include "common.hpp"
#include "prims.hpp"

namespace deftet {
namespace sx {

constexpr int kThreads = 256, kWaves = kThreads / 64;

struct Pred {
    const int4 *nbr;          // [T] rows of four partners
    const float *occ;         // [B,T]
    int T, mode;
    double htres;             // THRESHOLD: |no - o| > htres in double (the scipy product is float64) ...
    float thres2;             // ... and o > (float)(htres * 2) in fp32 (numpy compares an f32 array with a scalar in f32)
};

// bit i set <=> local face i of tet t of shape b is emitted.  The one predicate of both passes.
__device__ __forceinline__ unsigned face_mask(const Pred &p, int b, int t, int *bad)
{
    const float *occ = p.occ + (size_t)b * p.T;
    const float o = occ[t];
    const int4 n4 = p.nbr[t];
    const int n[4] = {n4.x, n4.y, n4.z, n4.w};
    unsigned m = 0u;
    if (p.mode == DEFTET_SX_BINARY) {
        if (!(o == 1.0f)) return 0u;                                   // center_occ == 1 (NaN == 1 is false)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (n[i] >= p.T) { if (bad) *bad = 1; continue; }
            if (n[i] >= 0 && occ[n[i]] != o) m |= 1u << i;             // has_adj and neibor_occ != center_occ (NaN != x is true)
        }
    } else {
        if (!(o > p.thres2)) return 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (n[i] >= p.T) { if (bad) *bad = 1; continue; }
            const double no = n[i] >= 0 ? (double)occ[n[i]] : 0.0;     // no neighbour: the empty matrix row gives 0
            if (fabs(no - (double)o) > p.htres) m |= 1u << i;
        }
    }
    return m;
}

// np.max over the four corner weights: the largest, NaN if any is NaN
__device__ __forceinline__ float max_nan(float m, float x) { return (m != m) ? m : ((x != x || x > m) ? x : m); }

__global__ __launch_bounds__(256) void k_sx_occ_max(const float *__restrict__ w, const int4 *__restrict__ idx, int V, int T, float *occ,
                                                    int *bad)
{
    const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int4 q = idx[t];
    const int v[4] = {q.x, q.y, q.z, q.w};
    const float *wb = w + (size_t)b * V;
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v[k] < 0 || v[k] >= V) { *bad = 1; continue; }
        m = max_nan(m, wb[v[k]]);
    }
    occ[(size_t)b * T + t] = m;
}

// totals of the wave's four ballots; `below` = faces of the lanes below this one
__device__ __forceinline__ unsigned wave_rank(unsigned mask, int lane, unsigned &below)
{
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned tot = 0u;
    below = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long bal = __ballot((mask >> i) & 1u);
        tot += (unsigned)__popcll(bal);
        below += (unsigned)__popcll(bal & lt);
    }
    return tot;
}

__global__ __launch_bounds__(kThreads) void k_sx_count(Pred p, int nblk, int B, int *blk, int *bad)
{
    __shared__ unsigned s_w[kWaves];
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
    const unsigned mask = t < p.T ? face_mask(p, b, t, bad) : 0u;
    unsigned below;
    const unsigned tot = wave_rank(mask, threadIdx.x & 63, below);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        blk[(size_t)b * nblk + blockIdx.x] = (int)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
        if (b == 0 && blockIdx.x == 0) blk[(size_t)B * nblk] = 0;      // the scan's last element: its exclusive value is the total
    }
}

// offsets[b] = first row of shape b, offsets[B] = number of rows; all -1 when an index was out of range
// state[0] = bad flag, state[1] = which occupancy the count pass ran on (kOccGiven / kOccFused): the fill pass writes nothing
// when it is asked for the other one (its fused occupancy would be uninitialised workspace)
constexpr int kOccGiven = 0x5A01, kOccFused = 0x5A02;
__global__ void k_sx_offsets(const int *__restrict__ pos, int nblk, int B, int *state, int occ_kind, int *offsets)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= B) offsets[b] = state[0] ? -1 : pos[(size_t)b * nblk];
    if (b == 0) state[1] = occ_kind;
}

struct Out {
    const float *tet;         // [B,T,4,3]
    const float *attr;        // [B,T,4,C] or null
    const int *tet_idx;       // [T,4] or null (with faces)
    float *face;              // [F,3,3]
    float *face_attr;         // [F,3,C] or null
    long long *index;         // [F,2] or null
    long long *faces;         // [F,3] or null
    long long capacity;       // rows the outputs hold
    int C;
};

__global__ __launch_bounds__(kThreads) void k_sx_fill(Pred p, Out o, int nblk, const int *__restrict__ pos, const int *__restrict__ state,
                                                      int occ_kind)
{
    if (state[1] != occ_kind) return;                                  // not the workspace of a count pass on this occupancy
    const int b = blockIdx.y;
    const size_t g = (size_t)b * nblk + blockIdx.x;
    const int base = pos[g], total = pos[g + 1] - base;
    if (total <= 0 || total > kThreads * 4 || base < 0) return;        // nothing to write (uniform over the workgroup); a foreign workspace writes nothing
    __shared__ unsigned short s_src[kThreads * 4];                     // row -> lane * 4 + local face, in rank order
    __shared__ unsigned s_w[kWaves];
    const int t0 = blockIdx.x * kThreads, t = t0 + threadIdx.x;
    const unsigned mask = t < p.T ? face_mask(p, b, t, nullptr) : 0u;
    unsigned r;
    const unsigned tot = wave_rank(mask, threadIdx.x & 63, r);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_w[w] = tot;
    __syncthreads();
    for (int k = 0; k < w; ++k) r += s_w[k];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if ((mask >> i) & 1u) s_src[r++] = (unsigned short)(threadIdx.x * 4 + i);
    __syncthreads();
    // rows this workgroup may write: its span, cut at the capacity the caller allocated
    const long long room = o.capacity - (long long)base;
    int rows = (int)(room < (long long)total ? (room > 0 ? room : 0) : (long long)total);
    rows = min(rows, (int)(s_w[0] + s_w[1] + s_w[2] + s_w[3]));       // (== total with the count pass's workspace: only staged rows are read)
    const size_t tb = (size_t)b * p.T + t0;                            // first tet of the workgroup in the flat [B*T] order
    {
        float *dst = o.face + (size_t)base * 9;
        for (int e = threadIdx.x; e < rows * 9; e += kThreads) {
            const int row = e / 9, k = e - row * 9, j = k / 3;
            const unsigned s = s_src[row];
            dst[e] = o.tet[(tb + (s >> 2)) * 12 + ((s & 3u) ^ (unsigned)j) * 3 + (k - j * 3)];
        }
    }
    if (o.face_attr) {
        const int C = o.C, C3 = 3 * C;
        float *dst = o.face_attr + (size_t)base * C3;
        for (int e = threadIdx.x; e < rows * C3; e += kThreads) {
            const int row = e / C3, k = e - row * C3, j = k / C;
            const unsigned s = s_src[row];
            dst[e] = o.attr[((tb + (s >> 2)) * 4 + ((s & 3u) ^ (unsigned)j)) * C + (k - j * C)];
        }
    }
    if (o.index) {
        long long *dst = o.index + (size_t)base * 2;
        for (int e = threadIdx.x; e < rows * 2; e += kThreads) {
            const unsigned s = s_src[e >> 1];
            dst[e] = (e & 1) ? (long long)(s & 3u) : (long long)(t0 + (int)(s >> 2));
        }
    }
    if (o.faces) {
        long long *dst = o.faces + (size_t)base * 3;
        for (int e = threadIdx.x; e < rows * 3; e += kThreads) {
            const int row = e / 3, j = e - row * 3;
            const unsigned s = s_src[row];
            dst[e] = (long long)o.tet_idx[(size_t)(t0 + (int)(s >> 2)) * 4 + ((s & 3u) ^ (unsigned)j)];
        }
    }
}

// ---------------------------------------------------------------------------- neighbour table by local face
__global__ __launch_bounds__(256) void k_face_nbr_scatter(const long long *__restrict__ tetidx, const long long *__restrict__ tetfaceidx,
                                                          int F, int T, long long *nbr64, int *nbr32)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const long long t0 = tetidx[2 * f], t1 = tetidx[2 * f + 1], f0 = tetfaceidx[2 * f], f1 = tetfaceidx[2 * f + 1];
    if (t1 < 0 || t0 < 0 || t0 >= T || t1 >= T || f0 < 0 || f0 > 3 || f1 < 0 || f1 > 3) return;     // boundary face (or a foreign table)
    if (nbr64) { nbr64[t0 * 4 + f0] = t1; nbr64[t1 * 4 + f1] = t0; }
    if (nbr32) { nbr32[t0 * 4 + f0] = (int)t1; nbr32[t1 * 4 + f1] = (int)t0; }
}

// ---------------------------------------------------------------------------- weld: used vertices in ascending id
__global__ __launch_bounds__(256) void k_weld_flag(const long long *__restrict__ faces, long long n, int V, int *flag, int *n_out)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long long v = faces[e];
    if (v < 0 || v >= V) { n_out[1] = 1; return; }
    flag[v] = 1;                                                       // (every writer stores the same word)
}

__global__ __launch_bounds__(256) void k_weld_gather(const int *__restrict__ pos, const float *__restrict__ verts, const float *__restrict__ attr,
                                                     int C, int V, int capacity, long long *old_id, float *verts_out, float *attr_out,
                                                     int *n_out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > V) return;
    if (v == V) { n_out[0] = pos[V]; return; }
    const int q = pos[v];
    if (pos[v + 1] == q || q >= capacity) return;
    old_id[q] = v;
#pragma unroll
    for (int k = 0; k < 3; ++k) verts_out[(size_t)q * 3 + k] = verts[(size_t)v * 3 + k];
    if (attr_out)
        for (int k = 0; k < C; ++k) attr_out[(size_t)q * C + k] = attr[(size_t)v * C + k];
}

__global__ __launch_bounds__(256) void k_weld_remap(const long long *__restrict__ faces, long long n, int V, const int *__restrict__ pos,
                                                    long long *faces_out)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long long v = faces[e];
    faces_out[e] = (v < 0 || v >= V) ? -1 : (long long)pos[v];
}

}  // namespace sx
}  // namespace deftet

using namespace deftet;
using namespace deftet::sx;

extern "C" int deftet_tet_face_neighbours_i64(const int64_t *tetidx_fx2, const int64_t *tetfaceidx_fx2, int n_face, int T,
                                              int64_t *nbr_tx4, int32_t *nbr32_tx4, void *stream_)
{
    DEFTET_CHECK_ARG(n_face >= 0 && T > 0, "n_face=%d, n_tet=%d: n_tet must be positive, n_face not negative", n_face, T);
    DEFTET_CHECK_ARG(T <= 500000000, "n_tet too large");
    DEFTET_CHECK_ARG(nbr_tx4 || nbr32_tx4, "null pointer: both neighbour tables");
    DEFTET_CHECK_ARG(n_face == 0 || (tetidx_fx2 && tetfaceidx_fx2), "null pointer: face table");
    hipStream_t st = as_stream(stream_);
    if (nbr_tx4) DEFTET_HIP(hipMemsetAsync(nbr_tx4, 0xFF, (size_t)T * 32, st));
    if (nbr32_tx4) DEFTET_HIP(hipMemsetAsync(nbr32_tx4, 0xFF, (size_t)T * 16, st));
    if (n_face > 0)
        DEFTET_LAUNCH(k_face_nbr_scatter, dim3(blocks_for(n_face, 256)), dim3(256), st, (const long long *)tetidx_fx2,
                      (const long long *)tetfaceidx_fx2, n_face, T, (long long *)nbr_tx4, (int *)nbr32_tx4);
    return DEFTET_OK;
}

static inline int sx_nblk(int T) { return (T + kThreads - 1) / kThreads; }

namespace {
// state: the bad flag and which occupancy the count pass ran on (k_sx_offsets); pos: faces per workgroup, scanned in place;
// occ: the occupancy the count pass derives from vertex weights, kept for the fill pass
struct Ws {
    int *bad, *pos;
    void *tmp;
    size_t n, tmp_bytes, bytes;
    float *occ;
};
Ws carve(void *workspace, int B, int T, int with_vertex_weights)
{
    Arena A(workspace);
    Ws w{};
    w.n = (size_t)B * sx_nblk(T) + 1;
    w.bad = A.take<int>(2);
    w.pos = A.take<int>(w.n);
    w.tmp_bytes = prims::scan_temp_bytes<int>(w.n);
    w.tmp = A.take<char>(w.tmp_bytes);
    if (with_vertex_weights) w.occ = A.take<float>((size_t)B * T);
    w.bytes = A.end();
    return w;
}

// flag: one word per vertex and one behind them, scanned in place into the new ids and their count
struct WeldWs {
    int *flag;
    void *tmp;
    size_t tmp_bytes, bytes;
};
WeldWs weld_carve(void *workspace, int V)
{
    Arena A(workspace);
    WeldWs w{};
    w.flag = A.take<int>((size_t)V + 1);
    w.tmp_bytes = prims::scan_temp_bytes<int>((size_t)V + 1);
    w.tmp = A.take<char>(w.tmp_bytes);
    w.bytes = A.end();
    return w;
}
int check_shape(int B, int T, int mode, double htres, const void *nbr, void *workspace, size_t wsb, int with_w, Ws &W)
{
    DEFTET_CHECK_ARG(T > 0, "n_tet=%d must be positive", T);
    DEFTET_CHECK_ARG(B > 0 && B <= 65535, "n_batch=%d outside 1..65535", B);
    DEFTET_CHECK_ARG((long long)B * T * 4 < 2147483647LL, "n_batch * n_tet * 4 does not fit 31 bits");
    DEFTET_CHECK_ARG(mode == DEFTET_SX_BINARY || mode == DEFTET_SX_THRESHOLD, "mode=%d is neither DEFTET_SX_BINARY nor DEFTET_SX_THRESHOLD", mode);
    DEFTET_CHECK_ARG(mode == DEFTET_SX_BINARY || htres == htres, "htres is NaN");
    DEFTET_CHECK_ARG(nbr && ((uintptr_t)nbr & 15) == 0, "null or misaligned pointer: nbr32_tx4");
    W = carve(workspace, B, T, with_w);
    DEFTET_TRY(workspace_ok("deftet_surface_extract*", workspace, wsb, W.bytes));
    return DEFTET_OK;
}
}  // namespace

extern "C" size_t deftet_surface_extract_workspace_bytes(int B, int T, int with_vertex_weights)
{
    return B <= 0 || T <= 0 ? 256 : carve(nullptr, B, T, with_vertex_weights).bytes;
}

extern "C" int deftet_surface_extract_count_f32(const float *occ_bxt, const float *weights_bxv, const int32_t *tet_idx_tx4, int V,
                                                const int32_t *nbr32_tx4, int B, int T, int mode, double htres, int32_t *offsets,
                                                void *workspace, size_t wsb, void *stream_)
{
    const int with_w = weights_bxv != nullptr;
    Ws W;
    DEFTET_TRY(check_shape(B, T, mode, htres, nbr32_tx4, workspace, wsb, with_w, W));
    DEFTET_CHECK_ARG(offsets, "null pointer: offsets");
    DEFTET_CHECK_ARG((occ_bxt != nullptr) != (weights_bxv != nullptr), "exactly one of occ_bxt and weights_bxv");
    DEFTET_CHECK_ARG(!with_w || (tet_idx_tx4 && ((uintptr_t)tet_idx_tx4 & 15) == 0 && V > 0),
                     "vertex weights need a 16-byte aligned tet_idx_tx4 and n_vertex > 0");
    hipStream_t st = as_stream(stream_);
    const int nblk = sx_nblk(T);
    DEFTET_HIP(hipMemsetAsync(W.bad, 0, 4, st));
    if (with_w)
        DEFTET_LAUNCH(k_sx_occ_max, dim3(blocks_for(T, 256), B), dim3(256), st, weights_bxv, (const int4 *)tet_idx_tx4, V, T, W.occ, W.bad);
    Pred p{(const int4 *)nbr32_tx4, with_w ? W.occ : occ_bxt, T, mode, htres, (float)(htres * 2.0)};
    DEFTET_LAUNCH(k_sx_count, dim3(nblk, B), dim3(kThreads), st, p, nblk, B, W.pos, W.bad);
    DEFTET_TRY(prims::scan<int, prims::Plus, true>(W.pos, W.pos, W.n, 0, prims::Plus(), W.tmp, W.tmp_bytes, st));
    DEFTET_LAUNCH(k_sx_offsets, dim3((B + 256) / 256), dim3(256), st, (const int *)W.pos, nblk, B, W.bad, with_w ? kOccFused : kOccGiven, offsets);
    return DEFTET_OK;
}

extern "C" int deftet_surface_extract_fill_f32(const float *tet_bxtx4x3, const float *attr_bxtx4xc, int C, const float *occ_bxt,
                                               const int32_t *tet_idx_tx4, const int32_t *nbr32_tx4, int B, int T, int mode,
                                               double htres, long long capacity, float *face, float *face_attr, int64_t *index,
                                               int64_t *faces, void *workspace, size_t wsb, void *stream_)
{
    const int with_w = occ_bxt == nullptr;                             // the count pass left the fused occupancy in the workspace
    Ws W;
    DEFTET_TRY(check_shape(B, T, mode, htres, nbr32_tx4, workspace, wsb, with_w, W));
    DEFTET_CHECK_ARG(capacity >= 0, "negative capacity");
    DEFTET_CHECK_ARG(!attr_bxtx4xc || (C >= 1 && C <= 8), "n_attr=%d outside 1..8", C);
    DEFTET_CHECK_ARG(!faces || tet_idx_tx4, "null pointer: faces needs tet_idx_tx4");
    if (capacity == 0) return DEFTET_OK;                               // (no row: the outputs may be empty, hence null)
    DEFTET_CHECK_ARG((attr_bxtx4xc != nullptr) == (face_attr != nullptr), "attr_bxtx4xc and face_attr go together");
    DEFTET_CHECK_ARG(tet_bxtx4x3 && face, "null pointer: tet_bxtx4x3 / face");
    hipStream_t st = as_stream(stream_);
    const int nblk = sx_nblk(T);
    Pred p{(const int4 *)nbr32_tx4, with_w ? W.occ : occ_bxt, T, mode, htres, (float)(htres * 2.0)};
    Out o{tet_bxtx4x3, attr_bxtx4xc, tet_idx_tx4, face, face_attr, (long long *)index, (long long *)faces, capacity, C};
    DEFTET_LAUNCH(k_sx_fill, dim3(nblk, B), dim3(kThreads), st, p, o, nblk, (const int *)W.pos, (const int *)W.bad, with_w ? kOccFused : kOccGiven);
    return DEFTET_OK;
}

extern "C" size_t deftet_surface_weld_workspace_bytes(int V)
{
    return V <= 0 ? 256 : weld_carve(nullptr, V).bytes;
}

extern "C" int deftet_surface_weld_f32(const int64_t *faces_fx3, long long n_face, const float *verts_vx3, const float *attr_vxc, int C,
                                       int V, int capacity, int32_t *n_out, int64_t *old_id, float *verts_out, float *attr_out,
                                       int64_t *faces_out, void *workspace, size_t wsb, void *stream_)
{
    DEFTET_CHECK_ARG(n_face >= 0 && n_face <= 700000000LL, "n_face=%lld outside 0..7e8", n_face);
    DEFTET_CHECK_ARG(V > 0, "n_vertex=%d must be positive", V);
    DEFTET_CHECK_ARG(n_out, "null pointer: n_out");
    DEFTET_CHECK_ARG(!attr_vxc || (C >= 1 && C <= 8), "n_attr=%d outside 1..8", C);
    DEFTET_CHECK_ARG(capacity >= 0, "negative capacity");
    hipStream_t st = as_stream(stream_);
    if (n_face == 0) { DEFTET_HIP(hipMemsetAsync(n_out, 0, 8, st)); return DEFTET_OK; }
    DEFTET_CHECK_ARG((attr_vxc != nullptr) == (attr_out != nullptr), "attr_vxc and attr_out go together");
    DEFTET_CHECK_ARG(faces_fx3 && verts_vx3 && old_id && verts_out && faces_out, "null pointer");
    DEFTET_CHECK_ARG((long long)capacity >= (n_face * 3 < (long long)V ? n_face * 3 : (long long)V),
                     "capacity=%d below min(n_vertex, 3 n_face)", capacity);
    const WeldWs W = weld_carve(workspace, V);
    DEFTET_TRY(workspace_ok(__func__, workspace, wsb, W.bytes));
    const long long n = n_face * 3;
    DEFTET_HIP(hipMemsetAsync(W.flag, 0, ((size_t)V + 1) * 4, st));
    DEFTET_HIP(hipMemsetAsync(n_out, 0, 8, st));
    DEFTET_LAUNCH(k_weld_flag, dim3(blocks_for(n, 256)), dim3(256), st, (const long long *)faces_fx3, n, V, W.flag, n_out);
    DEFTET_TRY(prims::scan<int, prims::Plus, true>(W.flag, W.flag, (size_t)V + 1, 0, prims::Plus(), W.tmp, W.tmp_bytes, st));
    DEFTET_LAUNCH(k_weld_gather, dim3((V + 256) / 256), dim3(256), st, (const int *)W.flag, verts_vx3, attr_vxc, C, V, capacity,
                  (long long *)old_id, verts_out, attr_out, n_out);
    DEFTET_LAUNCH(k_weld_remap, dim3(blocks_for(n, 256)), dim3(256), st, (const long long *)faces_fx3, n, V, (const int *)W.flag,
                  (long long *)faces_out);
    return DEFTET_OK;
}
