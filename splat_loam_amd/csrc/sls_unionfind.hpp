// sls_unionfind.hpp — the lock-free union-find shared by sls_mesh.hip (clusters of triangles), sls_fill.hip (chains of
// boundary half-edges) and sls_cluster.hip (the cores of a cloud): agent-scope integer atomics, no waiting.  The larger root
// is always linked under the smaller, so the root of a component is its lowest element whatever the order of the threads.
// Behind it what sls_mesh.hip and sls_cluster.hip share once nothing writes parent any more: uf_root, the walk of their
// flatten kernels, and uf_kth_largest, the k-th largest component count of their "keep the K largest" rule.
#pragma once
#include "sls_scan.hpp"

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

// the root above x by plain loads: for a launch of its own, in which parent is only read
__device__ __forceinline__ uint32_t uf_root(const uint32_t *__restrict__ parent, uint32_t x)
{
    uint32_t p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    return x;
}

// One workgroup of CH::kThreads: the k-th largest of the C counts = the largest value v with #{c : counts[c] >= v} >= k,
// by bisection over v in [1, n] (every count is at least 1, so v = 1 qualifies whenever k <= C); 0 for k = 0
template <typename CH>
__device__ __forceinline__ uint32_t uf_kth_largest(uint32_t n, uint32_t C, uint32_t k, const int32_t *__restrict__ counts)
{
    __shared__ uint32_t s_wave[CH::kThreads / 64];
    uint32_t lo = 0u;
    if (k > 0u) {
        uint32_t hi = n;
        lo = 1u;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            uint32_t mine = 0u;
            for (uint32_t c = threadIdx.x; c < C; c += CH::kThreads) mine += (uint32_t)counts[c] >= mid ? 1u : 0u;
            uint32_t total;
            block_scan<uint32_t, CH::kThreads>(mine, s_wave, &total);
            if (total >= k) lo = mid; else hi = mid - 1u;
            __syncthreads();                        // (s_wave is written again in the next round)
        }
    }
    return lo;
}

}  // namespace sls
