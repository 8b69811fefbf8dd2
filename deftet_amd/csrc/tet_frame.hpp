// tet_frame.hpp — the one routine that reads a tet of an indexed mesh and decides whether it is LIVE, shared by the operators on
// per-vertex fields (tet_field_grad.hip, tet_iso_measure.hip): all of them call a tet dead for the same bits of the same inputs.
#pragma once
#include "common.hpp"

namespace deftet {

// the tet at row `trow` of the index list over the positions p of its shape: the adjugate rows n, det; false for a dead tet
// (an index outside [0,V), or det > 0 fails in fp32: NaN, flat, inverted).  vol = det / 6.
__device__ __forceinline__ bool tet_frame(const float *__restrict__ p, const int32_t *__restrict__ tet_idx, size_t trow, int V, int vi[4],
                                          float n[3][3], float &det)
{
    const int4 q = *reinterpret_cast<const int4 *>(tet_idx + trow * 4);
    vi[0] = q.x; vi[1] = q.y; vi[2] = q.z; vi[3] = q.w;
    det = 0.0f;
    if ((unsigned)q.x >= (unsigned)V || (unsigned)q.y >= (unsigned)V || (unsigned)q.z >= (unsigned)V || (unsigned)q.w >= (unsigned)V)
        return false;
    float x[4][3], e[3][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) x[k][a] = p[(size_t)vi[k] * 3 + a];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) e[k][a] = x[k + 1][a] - x[0][a];
    cross3(e[1], e[2], n[0]);
    cross3(e[2], e[0], n[1]);
    cross3(e[0], e[1], n[2]);
    det = dot3(e[0], n[0]);
    return det > 0.0f;                                                // (a NaN is not)
}

}  // namespace deftet
