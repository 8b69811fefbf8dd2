// tet_iso_measure.hip — the solid {field > iso} of a per-vertex field, measured tet by tet: the share of every tet
// that lies inside, the area of the iso polygon in it, and per shape the enclosed volume, the surface area and the overlap with a
// per-tet occupancy.  It is the solid marching_tets.hip bounds: the same predicate (a corner is inside iff field > iso in fp32,
// strict) and the same crossing parameters.  A tet is LIVE iff tet_frame (tet_frame.hpp, tet_field_gradient's routine) says so
// and its four corner values are finite; a dead tet has fraction 0, area 0, volume 0 and takes part in no sum and no backward.
// (The one deliberate difference from marching_tets, where a NaN corner is outside and faces are still emitted.)
//
// Per live tet, in double from the fp32 inputs, rounded once.  With the case code (bit k = corner k inside) the corners are put
// in a LOCAL ORDER l0..l3 (tim_order); tau(i,o) = (f_i - iso) / (f_i - f_o), q(i,o) = p_i + tau (p_o - p_i), e_x = p_lx - p_l0:
//   1 inside  (l0; outside l1 l2 l3)   u_x = tau(l0,lx):  frac = u1 u2 u3,      area = |(u1 e1 - u3 e3) x (u2 e2 - u3 e3)| / 2
//   3 inside  (l0 OUTSIDE; l1 l2 l3)   the same u_x:      frac = 1 - u1 u2 u3,  the same area (the triangle of the three cuts)
//             (1 - tau is formed as (iso - f_o) / (f_i - f_o) and 1 - u1 u2 u3 as (1 - u1) + u1 (1 - u2) + u1 u2 (1 - u3): no cancellation)
//   2 inside  (l0 l1; outside l2 l3)   al = tau(l0,l2), be = tau(l0,l3), ga = tau(l1,l2), de = tau(l1,l3):
//             frac = al be + (1 - al) be ga + (1 - be) ga de,  area = |(q(l1,l3) - q(l0,l2)) x (q(l1,l2) - q(l0,l3))| / 2
//   0 / 4 inside                        frac = 0 / 1, area = 0
// The differences of cut points are formed from the e_x, never from two positions, so a thin crossing (tau of 1e-6) keeps its
// relative accuracy.  Backward: d tau / d f_i = (1 - tau) / (f_i - f_o), d tau / d f_o = tau / (f_i - f_o) (never the squared
// gap), d area / d q by the unit normal of the polygon (0 where the area is 0); on a kink the case the predicate picks.
// The per-tet volume written out is tet_frame's det / 6 in fp32 (the bits of tet_volumes); the totals and every backward take
// the volume in double from the same fp32 positions.
// No float atomics; every sum has one order:
//   to the vertices   one double per output over the vertex's incidences in the CSR's order (ascending 4 t + corner), from 0,
//                     the case recomputed per incidence, rounded once
//   totals            per thread a double per sum over its tets in ascending t, the wave butterfly, the waves of a workgroup in
//                     ascending order, then the 64 workgroups of a shape by the butterfly again (k_tim_final), rounded once
#include "common.hpp"
#include "tet_frame.hpp"
#include "wave.hpp"

namespace deftet {
namespace {

constexpr int kTimBlock = 256;
constexpr int kTimParts = 64;                                        // workgroups per shape of the totals' pass: one partial per lane of k_tim_final
constexpr int kTimSums = 5;                                          // inside volume, area, intersection, weighted volume, live volume

// the local order of a case code, two bits per slot: 1 inside — the inside corner, then the others ascending; 3 inside — the
// OUTSIDE corner, then the others ascending; 2 inside — the inside pair ascending, then the outside pair ascending
__device__ __forceinline__ unsigned tim_order(unsigned code)
{
    const unsigned long long w = code < 8u ? 0x93C9D8D2E4E1E4E4ull : 0xE4E4E14ED28D9C93ull;
    return (unsigned)(w >> ((code & 7u) * 8u)) & 0xFFu;
}
__device__ __forceinline__ double pick4(const double x[4], unsigned k) { return k == 0u ? x[0] : k == 1u ? x[1] : k == 2u ? x[2] : x[3]; }
__device__ __forceinline__ void cross3d(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3d(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ bool finite32(float x) { return x - x == 0.0f; }

// a live tet as the measures read it
struct TimTet {
    int vi[4];
    double x[4][3], f[4];                                            // positions and corner values, in the tet's own order
    double vol;                                                      // det / 6 in double
    float vol32;                                                     // det / 6 as tet_frame has it
    unsigned code;                                                   // bit k: corner k inside
};

__device__ __forceinline__ bool tim_load(const float *__restrict__ p, const float *__restrict__ field, const int32_t *__restrict__ tet_idx,
                                         size_t trow, int V, float iso, TimTet &t)
{
    float n32[3][3], det32;
    if (!tet_frame(p, tet_idx, trow, V, t.vi, n32, det32)) return false;
    float f32[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f32[k] = field[t.vi[k]];
    if (!(finite32(f32[0]) && finite32(f32[1]) && finite32(f32[2]) && finite32(f32[3]))) return false;
    t.code = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.f[k] = (double)f32[k];
        t.code |= f32[k] > iso ? 1u << k : 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) t.x[k][a] = (double)p[(size_t)t.vi[k] * 3 + a];
    }
    t.vol32 = det32 / 6.0f;
    return true;
}

// the adjugate rows of the tet in double (as tet_frame's in fp32), its volume; m_k = d det / d x_k
__device__ __forceinline__ void tim_volume(TimTet &t, double n[3][3])
{
    double e[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) e[k][a] = t.x[k + 1][a] - t.x[0][a];
    cross3d(e[1], e[2], n[0]);
    cross3d(e[2], e[0], n[1]);
    cross3d(e[0], e[1], n[2]);
    t.vol = dot3d(e[0], n[0]) / 6.0;
}

// One cut of the iso polygon with an edge (local corners i -> o): tau, 1 - tau = (iso - f_o) / (f_i - f_o), the gap f_i - f_o,
// d frac / d tau, d area / d q, p_o - p_i
struct TimCut {
    double tau, ctau, gap, dfrac, G[3], dir[3];                      // ctau = 1 - tau
};

// the case of a tet with 1, 2 or 3 corners inside, in the local order: fl the corner values, e[x] = p_lx - p_l0 (e[0] unused).
// WithGrad: the cuts c[0..ncut) with their derivatives — (0,1) (0,2) (0,3), or with two inside (0,2) (0,3) (1,2) (1,3)
template <bool WithGrad>
__device__ __forceinline__ void tim_case(int n_in, const double fl[4], const double e[4][3], double iso, double &frac, double &area, TimCut c[4])
{
    double N[3];
    if (n_in != 2) {
        double u[4], cu[4], a[3], b[3];                               // cu = 1 - u, formed without the cancellation
#pragma unroll
        for (int x = 1; x < 4; ++x) {
            u[x] = (fl[0] - iso) / (fl[0] - fl[x]);
            cu[x] = (iso - fl[x]) / (fl[0] - fl[x]);
        }
        frac = n_in == 1 ? (u[1] * u[2]) * u[3] : (cu[1] + u[1] * cu[2]) + (u[1] * u[2]) * cu[3];      // (1 - u1 u2 u3, term by term)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = u[1] * e[1][k] - u[3] * e[3][k];
            b[k] = u[2] * e[2][k] - u[3] * e[3][k];
        }
        cross3d(a, b, N);
        const double len = sqrt(dot3d(N, N));
        area = 0.5 * len;
        if (WithGrad) {
            const double sgn = n_in == 1 ? 1.0 : -1.0, inv = len > 0.0 ? 1.0 / len : 0.0;
            const double nh[3] = {N[0] * inv, N[1] * inv, N[2] * inv};
            double g1[3], g2[3];
            cross3d(b, nh, g1);
            cross3d(nh, a, g2);
            c[0].dfrac = sgn * (u[2] * u[3]);
            c[1].dfrac = sgn * (u[1] * u[3]);
            c[2].dfrac = sgn * (u[1] * u[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[0].G[k] = 0.5 * g1[k];
                c[1].G[k] = 0.5 * g2[k];
                c[2].G[k] = -(c[0].G[k] + c[1].G[k]);
            }
#pragma unroll
            for (int x = 1; x < 4; ++x) {
                c[x - 1].tau = u[x];
                c[x - 1].ctau = cu[x];
                c[x - 1].gap = fl[0] - fl[x];
#pragma unroll
                for (int k = 0; k < 3; ++k) c[x - 1].dir[k] = e[x][k];
            }
        }
    } else {
        const double al = (fl[0] - iso) / (fl[0] - fl[2]), be = (fl[0] - iso) / (fl[0] - fl[3]);
        const double ga = (fl[1] - iso) / (fl[1] - fl[2]), de = (fl[1] - iso) / (fl[1] - fl[3]);
        const double cal = (iso - fl[2]) / (fl[0] - fl[2]), cbe = (iso - fl[3]) / (fl[0] - fl[3]);      // 1 - al, ... without the cancellation
        const double cga = (iso - fl[2]) / (fl[1] - fl[2]), cde = (iso - fl[3]) / (fl[1] - fl[3]);
        frac = (al * be + (cal * be) * ga) + (cbe * ga) * de;
        double d1[3], d2[3], e21[3], e31[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e21[k] = e[2][k] - e[1][k];
            e31[k] = e[3][k] - e[1][k];
            d1[k] = (e[1][k] + de * e31[k]) - al * e[2][k];          // q(l1,l3) - q(l0,l2)
            d2[k] = (e[1][k] + ga * e21[k]) - be * e[3][k];          // q(l1,l2) - q(l0,l3)
        }
        cross3d(d1, d2, N);
        const double len = sqrt(dot3d(N, N));
        area = 0.5 * len;
        if (WithGrad) {
            const double inv = len > 0.0 ? 1.0 / len : 0.0;
            const double nh[3] = {N[0] * inv, N[1] * inv, N[2] * inv};
            double g13[3], g12[3];
            cross3d(d2, nh, g13);                                     // 2 d area / d q(l1,l3)
            cross3d(nh, d1, g12);                                     // 2 d area / d q(l1,l2)
            c[0].tau = al; c[0].ctau = cal; c[0].gap = fl[0] - fl[2]; c[0].dfrac = be * cga;
            c[1].tau = be; c[1].ctau = cbe; c[1].gap = fl[0] - fl[3]; c[1].dfrac = (al + cal * ga) - ga * de;
            c[2].tau = ga; c[2].ctau = cga; c[2].gap = fl[1] - fl[2]; c[2].dfrac = cal * be + cbe * de;
            c[3].tau = de; c[3].ctau = cde; c[3].gap = fl[1] - fl[3]; c[3].dfrac = cbe * ga;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[0].G[k] = -0.5 * g13[k]; c[0].dir[k] = e[2][k];
                c[1].G[k] = -0.5 * g12[k]; c[1].dir[k] = e[3][k];
                c[2].G[k] = 0.5 * g12[k];  c[2].dir[k] = e21[k];
                c[3].G[k] = 0.5 * g13[k];  c[3].dir[k] = e31[k];
            }
        }
    }
}

// the local frame of a loaded tet: the order, the inside count, the corner values and the edges from local corner 0
__device__ __forceinline__ int tim_local(const TimTet &t, unsigned &order, double fl[4], double e[4][3])
{
    order = tim_order(t.code);
    double xa[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) xa[a][k] = t.x[k][a];
    double x0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x0[a] = pick4(xa[a], order & 3u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned k = (order >> (2 * j)) & 3u;
        fl[j] = pick4(t.f, k);
#pragma unroll
        for (int a = 0; a < 3; ++a) e[j][a] = pick4(xa[a], k) - x0[a];
    }
    return __popc(t.code);
}

// frac and area of a loaded tet
__device__ __forceinline__ void tim_measure(const TimTet &t, double iso, double &frac, double &area)
{
    area = 0.0;
    if (t.code == 0u || t.code == 15u) {
        frac = t.code ? 1.0 : 0.0;
        return;
    }
    unsigned order;
    double fl[4], e[4][3];
    TimCut unused[4];
    const int n_in = tim_local(t, order, fl, e);
    tim_case<false>(n_in, fl, e, iso, frac, area, unused);
}

// grid (T / 256, B): one lane per tet
__global__ __launch_bounds__(kTimBlock) void k_tim_fwd(const float *__restrict__ field, const float *__restrict__ pos,
                                                       const int32_t *__restrict__ tet_idx, float *frac_out, float *area_out, float *vol_out,
                                                       float iso, int V, int T, int idx_batch)
{
    const int t = blockIdx.x * kTimBlock + threadIdx.x, b = blockIdx.y;
    if (t >= T) return;
    TimTet tet;
    double frac = 0.0, area = 0.0;
    const bool live = tim_load(pos + (size_t)b * V * 3, field + (size_t)b * V, tet_idx, (idx_batch > 1 ? (size_t)b * T : 0) + t, V, iso, tet);
    if (live) tim_measure(tet, (double)iso, frac, area);
    const size_t o = (size_t)b * T + t;
    frac_out[o] = (float)frac;
    if (area_out) area_out[o] = (float)area;
    if (vol_out) vol_out[o] = live ? tet.vol32 : 0.0f;
}

// What arrives on a tet's fraction (gF), area (gA) and volume (gV).  Explicit: the rows of grad_frac, grad_area, grad_vol
// [B,T], each optional.  Measures: from the five upstream scalars go of the shape and the weight w_t (1 without weights), with
// s = go0 + w_t go2:  gF = s vol,  gA = go1,  gV = (s frac + w_t go3) + go4.
struct TimExplicit {
    const float *gfrac, *garea, *gvol;                               // of the shape
    __device__ __forceinline__ void on_tet(int t, double, double, double &gF, double &gA, double &gV) const
    {
        gF = gfrac ? (double)gfrac[t] : 0.0;
        gA = garea ? (double)garea[t] : 0.0;
        gV = gvol ? (double)gvol[t] : 0.0;
    }
};
struct TimMeasures {
    const float *go, *w;                                             // of the shape: [5] and [T] (or null)
    __device__ __forceinline__ void on_tet(int t, double frac, double vol, double &gF, double &gA, double &gV) const
    {
        const double wt = w ? (double)w[t] : 1.0, s = (double)go[0] + wt * (double)go[2];
        gF = s * vol;
        gA = (double)go[1];
        gV = (s * frac + wt * (double)go[3]) + (double)go[4];
    }
};

// grid (V / 256, B): one lane per vertex walks its incidences; per incidence the tet's case is recomputed and the share of the
// vertex's corner taken
template <typename Up>
__device__ __forceinline__ void tim_bwd(const Up up, const float *__restrict__ field, const float *__restrict__ pos,
                                        const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                        const int32_t *__restrict__ slots, float *gfield, float *gpos, float iso32, int b, int V, int T,
                                        int idx_batch)
{
    const int v = blockIdx.x * kTimBlock + threadIdx.x;
    if (v >= V) return;
    const size_t row = (idx_batch > 1 ? (size_t)b * V : 0) + v, tbase = idx_batch > 1 ? (size_t)b * T : 0;
    const int i0 = offsets[row], i1 = offsets[row + 1];
    const float *p = pos + (size_t)b * V * 3, *f = field + (size_t)b * V;
    const double iso = (double)iso32;
    double accf = 0.0, accp[3] = {0.0, 0.0, 0.0};
    for (int i = i0; i < i1; ++i) {
        const int s = slots[i], t = s >> 2, corner = s & 3;
        if ((unsigned)t >= (unsigned)T) continue;
        TimTet tet;
        if (!tim_load(p, f, tet_idx, tbase + t, V, iso32, tet)) continue;
        double n[3][3], frac = tet.code == 15u ? 1.0 : 0.0, area = 0.0, gF, gA, gV;
        tim_volume(tet, n);
        const bool cut = tet.code != 0u && tet.code != 15u;
        unsigned order = 0xE4u;
        double fl[4], e[4][3];
        TimCut c[4];
        int n_in = 0;
        if (cut) {
            n_in = tim_local(tet, order, fl, e);
            tim_case<true>(n_in, fl, e, iso, frac, area, c);
        }
        up.on_tet(t, frac, tet.vol, gF, gA, gV);
        // the volume's share: m_k / 6 with m_0 = -(n0 + n1 + n2), m_k = n_{k-1}
        double tf = 0.0, tp[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double m = corner == 0 ? -((n[0][a] + n[1][a]) + n[2][a]) : corner == 1 ? n[0][a] : corner == 2 ? n[1][a] : n[2][a];
            tp[a] = gV * (m / 6.0);
        }
        if (cut) {
            // the local slot of this corner, then the cuts that end in it: as the edge's first end (i) or its second (o)
            unsigned j = 0u;
#pragma unroll
            for (unsigned q = 1u; q < 4u; ++q) j = ((order >> (2u * q)) & 3u) == (unsigned)corner ? q : j;
            const int ncut = n_in == 2 ? 4 : 3;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= ncut) continue;
                const unsigned ci = n_in == 2 ? (unsigned)(k >> 1) : 0u, co = n_in == 2 ? 2u + (unsigned)(k & 1) : 1u + (unsigned)k;
                if (j != ci && j != co) continue;
                const double ck = gF * c[k].dfrac + gA * dot3d(c[k].G, c[k].dir);
                const double wgt = j == ci ? c[k].ctau : c[k].tau;
                tf = tf + ck * (wgt / c[k].gap);
#pragma unroll
                for (int a = 0; a < 3; ++a) tp[a] = tp[a] + (gA * wgt) * c[k].G[a];
            }
        }
        accf = accf + tf;
#pragma unroll
        for (int a = 0; a < 3; ++a) accp[a] = accp[a] + tp[a];
    }
    if (gfield) gfield[(size_t)b * V + v] = (float)accf;
    if (gpos) {
        float *o = gpos + ((size_t)b * V + v) * 3;
        o[0] = (float)accp[0]; o[1] = (float)accp[1]; o[2] = (float)accp[2];
    }
}

__global__ __launch_bounds__(kTimBlock) void k_tim_bwd(const float *__restrict__ gfrac, const float *__restrict__ garea,
                                                       const float *__restrict__ gvol, const float *__restrict__ field,
                                                       const float *__restrict__ pos, const int32_t *__restrict__ tet_idx,
                                                       const int32_t *__restrict__ offsets, const int32_t *__restrict__ slots, float *gfield,
                                                       float *gpos, float iso, int V, int T, int idx_batch)
{
    const int b = blockIdx.y;
    const size_t o = (size_t)b * T;
    tim_bwd(TimExplicit{gfrac ? gfrac + o : nullptr, garea ? garea + o : nullptr, gvol ? gvol + o : nullptr}, field, pos, tet_idx, offsets,
            slots, gfield, gpos, iso, b, V, T, idx_batch);
}
__global__ __launch_bounds__(kTimBlock) void k_tim_sums_bwd(const float *__restrict__ go, const float *__restrict__ weights,
                                                            const float *__restrict__ field, const float *__restrict__ pos,
                                                            const int32_t *__restrict__ tet_idx, const int32_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ slots, float *gfield, float *gpos, float iso, int V,
                                                            int T, int idx_batch)
{
    const int b = blockIdx.y;
    tim_bwd(TimMeasures{go + (size_t)b * kTimSums, weights ? weights + (size_t)b * T : nullptr}, field, pos, tet_idx, offsets, slots, gfield,
            gpos, iso, b, V, T, idx_batch);
}

// grid (kTimParts, B): per workgroup the five sums over its tets, in doubles
__global__ __launch_bounds__(kTimBlock) void k_tim_pass(const float *__restrict__ field, const float *__restrict__ pos,
                                                        const int32_t *__restrict__ tet_idx, const float *__restrict__ weights, double *part,
                                                        float iso, int V, int T, int idx_batch)
{
    __shared__ double sh[kTimBlock / 64][kTimSums];
    const int b = blockIdx.y;
    const float *p = pos + (size_t)b * V * 3, *f = field + (size_t)b * V, *w = weights ? weights + (size_t)b * T : nullptr;
    const size_t tbase = idx_batch > 1 ? (size_t)b * T : 0;
    double acc[kTimSums];
#pragma unroll
    for (int k = 0; k < kTimSums; ++k) acc[k] = 0.0;
    for (int t = blockIdx.x * kTimBlock + threadIdx.x; t < T; t += kTimParts * kTimBlock) {
        TimTet tet;
        if (!tim_load(p, f, tet_idx, tbase + t, V, iso, tet)) continue;
        double n[3][3], frac, area;
        tim_volume(tet, n);
        tim_measure(tet, (double)iso, frac, area);
        const double wt = w ? (double)w[t] : 1.0, fv = frac * tet.vol;
        acc[0] += fv;
        acc[1] += area;
        acc[2] += wt * fv;
        acc[3] += wt * tet.vol;
        acc[4] += tet.vol;
    }
#pragma unroll
    for (int k = 0; k < kTimSums; ++k) acc[k] = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < kTimSums; ++k) sh[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < kTimSums) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kTimBlock / 64; ++w) s += sh[w][threadIdx.x];
        part[((size_t)b * kTimParts + blockIdx.x) * kTimSums + threadIdx.x] = s;
    }
}

// grid (B), one wave: lane l holds the partial of workgroup l
__global__ __launch_bounds__(64) void k_tim_final(const double *__restrict__ part, float *out)
{
    const int b = blockIdx.x;
    const double *src = part + ((size_t)b * kTimParts + threadIdx.x) * kTimSums;
    double v[kTimSums];
#pragma unroll
    for (int k = 0; k < kTimSums; ++k) v[k] = wave_sum(src[k]);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < kTimSums; ++k) out[(size_t)b * kTimSums + k] = (float)v[k];
}
static_assert(kTimParts == 64, "k_tim_final reads one partial per lane of a wave");

// the workspace of the totals: the partial sums of the pass
struct TimLayout {
    size_t bytes;
    double *part;
};
TimLayout tim_layout(size_t B, void *ws)
{
    TimLayout L{};
    Arena A(ws);
    L.part = A.take<double>(B * kTimParts * kTimSums);
    L.bytes = A.end();
    return L;
}

int tim_check(int B, int V, int T, int idx_batch, float iso, const char *what)
{
    if (B < 0 || V < 0 || T < 0) return set_error(DEFTET_EINVAL, "%s: negative size", what);
    if (!(iso == iso && iso - iso == 0.0f)) return set_error(DEFTET_EINVAL, "%s: iso is not finite", what);
    if (B > 65535) return set_error(DEFTET_ELIMIT, "%s: more than 65535 shapes", what);
    if (idx_batch != 1 && idx_batch != B) return set_error(DEFTET_EINVAL, "%s: tet list batch must be 1 or n_batch (got %d)", what, idx_batch);
    if ((long long)B * V >= 0x7FFFFFFFll || (long long)B * T * 4 >= 0x7FFFFFFFll)
        return set_error(DEFTET_ELIMIT, "%s: B V or 4 B T does not fit 31 bits", what);
    return DEFTET_OK;
}

}  // namespace
}  // namespace deftet

using namespace deftet;

extern "C" {

int deftet_tet_iso_fraction_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, float *frac, float *area, float *vol,
                                    float iso, int n_batch, int n_vertex, int n_tet, int idx_batch, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet;
    DEFTET_TRY(tim_check(B, V, T, idx_batch, iso, "tet_iso_fraction"));
    if (B == 0 || T == 0) return DEFTET_OK;
    DEFTET_CHECK_ARG(tet_idx && frac && ((field && pos) || V == 0), "tet_iso_fraction: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_iso_fraction: tet_idx must be 16-byte aligned");
    DEFTET_LAUNCH(k_tim_fwd, dim3(blocks_for(T, kTimBlock), (unsigned)B), dim3(kTimBlock), as_stream(stream), field, pos, tet_idx, frac, area, vol,
                  iso, V, T, idx_batch);
    return DEFTET_OK;
}

int deftet_tet_iso_fraction_bwd_f32(const float *grad_frac, const float *grad_area, const float *grad_vol, const float *field,
                                    const float *pos, const int32_t *tet_idx, const int32_t *offsets, const int32_t *slots,
                                    float *grad_field, float *grad_pos, float iso, int n_batch, int n_vertex, int n_tet, int idx_batch,
                                    void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet;
    DEFTET_TRY(tim_check(B, V, T, idx_batch, iso, "tet_iso_fraction_bwd"));
    if (B == 0 || V == 0 || !(grad_field || grad_pos)) return DEFTET_OK;
    DEFTET_CHECK_ARG(field && pos && offsets && (T == 0 || (tet_idx && slots)), "tet_iso_fraction_bwd: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_iso_fraction_bwd: tet_idx must be 16-byte aligned");
    DEFTET_LAUNCH(k_tim_bwd, dim3(blocks_for(V, kTimBlock), (unsigned)B), dim3(kTimBlock), as_stream(stream), grad_frac, grad_area, grad_vol, field,
                  pos, tet_idx, offsets, slots, grad_field, grad_pos, iso, V, T, idx_batch);
    return DEFTET_OK;
}

size_t deftet_tet_iso_measures_workspace_bytes(int n_batch)
{
    return n_batch < 0 ? 0 : tim_layout((size_t)n_batch, nullptr).bytes;
}

int deftet_tet_iso_measures_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, const float *weights, float *out, float iso,
                                    int n_batch, int n_vertex, int n_tet, int idx_batch, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet;
    DEFTET_TRY(tim_check(B, V, T, idx_batch, iso, "tet_iso_measures"));
    const TimLayout L = tim_layout((size_t)B, workspace);
    if (B == 0) return DEFTET_OK;
    DEFTET_TRY(workspace_ok(__func__, workspace, workspace_bytes, L.bytes));
    DEFTET_CHECK_ARG(out && (T == 0 || tet_idx) && ((field && pos) || V == 0 || T == 0), "tet_iso_measures: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_iso_measures: tet_idx must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    DEFTET_LAUNCH(k_tim_pass, dim3(kTimParts, (unsigned)B), dim3(kTimBlock), st, field, pos, tet_idx, weights, L.part, iso, V, T, idx_batch);
    DEFTET_LAUNCH(k_tim_final, dim3((unsigned)B), dim3(64), st, (const double *)L.part, out);
    return DEFTET_OK;
}

int deftet_tet_iso_measures_bwd_f32(const float *grad_out, const float *weights, const float *field, const float *pos, const int32_t *tet_idx,
                                    const int32_t *offsets, const int32_t *slots, float *grad_field, float *grad_pos, float iso, int n_batch,
                                    int n_vertex, int n_tet, int idx_batch, void *stream)
{
    const int B = n_batch, V = n_vertex, T = n_tet;
    DEFTET_TRY(tim_check(B, V, T, idx_batch, iso, "tet_iso_measures_bwd"));
    if (B == 0 || V == 0 || !(grad_field || grad_pos)) return DEFTET_OK;
    DEFTET_CHECK_ARG(grad_out && field && pos && offsets && (T == 0 || (tet_idx && slots)), "tet_iso_measures_bwd: null pointer");
    DEFTET_CHECK_ARG(((uintptr_t)tet_idx & 15) == 0, "tet_iso_measures_bwd: tet_idx must be 16-byte aligned");
    DEFTET_LAUNCH(k_tim_sums_bwd, dim3(blocks_for(V, kTimBlock), (unsigned)B), dim3(kTimBlock), as_stream(stream), grad_out, weights, field, pos,
                  tet_idx, offsets, slots, grad_field, grad_pos, iso, V, T, idx_batch);
    return DEFTET_OK;
}

}  // extern "C"
