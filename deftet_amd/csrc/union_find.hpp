// union_find.hpp — the lock-free union-find of the component labellings (tet_components.hip, mesh_components.hip), stated once.
//
// One invariant: parent[x] <= x, and parent[x] == x only for a root.  Every write keeps it — a root r is hooked under a smaller
// root by compare-and-swap (r -> q, q < r), a non-root is shortened to an ancestor by fetch_min — so a parent chain strictly
// descends, ends after at most x steps, and the root of a finished forest is the smallest index of its component whatever order
// the hooks happened in.  Parent words change under other workgroups, on any XCD: every access is a relaxed agent-scope atomic
// (L2-served, never a CU's L1).  No lane waits for another: a failed compare-and-swap means another lane hooked that root, and
// the retry starts from strictly smaller roots.  Every loop has a trip bound in the code; a chain that breaks the invariant or a
// loop that runs out is counted in `bad`.
#pragma once
#include <hip/hip_runtime.h>

namespace deftet {
namespace uf {

__device__ __forceinline__ int pload(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with every visited node shortened to its grandparent; -1 (and one count in bad) when the chain does not descend
__device__ __forceinline__ int find_root(int *par, int x, int *bad)
{
    const int limit = x;                                               // a descending chain from x has at most x links
    int p = pload(par + x);
    for (int step = 0; p != x; ++step) {
        if ((unsigned)p > (unsigned)x || step > limit) { atomicAdd(bad, 1); return -1; }  // (p in [0, x) from here on)
        const int gp = pload(par + p);
        if (gp != p && (unsigned)gp < (unsigned)p)
            __hip_atomic_fetch_min(par + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

// a failure re-reads the roots: they only ever move down, so ra + rb falls with every trip and 2 N + 2 trips cannot be used up
__device__ __forceinline__ void unite(int *par, int a, int b, int trips, int *bad)
{
    for (int k = 0; k < trips; ++k) {
        int ra = find_root(par, a, bad), rb = find_root(par, b, bad);
        if (ra < 0 || rb < 0 || ra == rb) return;
        if (ra > rb) { const int s = ra; ra = rb; rb = s; }
        int expect = rb;
        if (__hip_atomic_compare_exchange_strong(par + rb, &expect, ra, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = ra;
        b = rb;
    }
    atomicAdd(bad, 1);
}

}  // namespace uf
}  // namespace deftet
