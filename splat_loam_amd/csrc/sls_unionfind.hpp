// sls_unionfind.hpp — the lock-free union-find shared by sls_mesh.hip (clusters of triangles) and sls_fill.hip (chains of
// boundary half-edges): agent-scope integer atomics, no waiting.  The larger root is always linked under the smaller, so
// the root of a component is its lowest element whatever the order of the threads.
#pragma once
#include "sls_common.hpp"

namespace sls {

__device__ __forceinline__ uint32_t uf_load(uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x; on the way every visited node is pointed at its grandparent (an atomic min: a parent only decreases)
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = uf_load(parent + x);
    while (p != x) {
        const uint32_t gp = uf_load(parent + p);
        if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

// links the larger of the two roots under the smaller; a lost compare-and-swap (the root was linked by another thread in
// the meantime, to something smaller) is retried from the new roots
__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t s = a; a = b; b = s; }
        uint32_t expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

}  // namespace sls
