// gm_unionfind.hpp -- the lock-free union-find helpers shared by k_wall_regions.hip and k_wall_objects.hip (device only).
// A parent only ever decreases and stays inside its component, so the root of a finished forest is the component's
// smallest index.  The LDS pair serves one workgroup's tile; the global pair runs between workgroups of one launch, so
// EVERY access to the parent array there is an agent-scope atomic (a plain load may be served stale from L1 or another
// XCD's L2).
#pragma once
#include "gm_internal.hpp"

namespace gm {

__device__ __forceinline__ uint32_t wr_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t wr_lds_find(uint32_t *L, uint32_t x)
{
    for (;;) {
        const uint32_t y = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (y == x) return x;
        x = y;
    }
}
__device__ __forceinline__ void wr_lds_union(uint32_t *L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = wr_lds_find(L, a);
        b = wr_lds_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&L[a], b);   // a was a root when read; old != a: another wave linked it meanwhile
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ uint32_t wr_find(uint32_t *p, uint32_t x)
{
    for (;;) {
        const uint32_t y = wr_load(&p[x]);
        if (y == x) return x;
        const uint32_t z = wr_load(&p[y]);
        if (z == y) return y;
        atomicMin(&p[x], z);   // path halving: z is an ancestor of x, below its parent
        x = z;
    }
}
__device__ __forceinline__ void wr_union(uint32_t *p, uint32_t a, uint32_t b)
{
    for (;;) {
        a = wr_find(p, a);
        b = wr_find(p, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&p[a], b);
        if (old == a) return;
        a = old;   // a lost its root to another thread: what it pointed to still has to meet b
    }
}

}  // namespace gm
