// sls_sweep.hpp — what the box sweep of sls_knn.hip and the ray traversal of sls_raycast.hip both stand on: the shape of an
// index (items in curve order, boxes over runs of 256, sub-boxes over runs of 32), its wave-private LDS, the lane
// broadcast and the ballot compaction, and the triangle item with its guarded load.
#pragma once
#include <float.h>

#include "sls_geom.hpp"

namespace sls {

constexpr int kSweepBox = 256;                          // items per box
constexpr int kSweepSub = 32;                           // items per sub-box
constexpr int kSweepSubs = kSweepBox / kSweepSub;       // 8 sub-boxes per box

// The sweep knows an index by its boxes alone; what an ITEM is (a point: float4, xyz + original index; a triangle: TriItem
// below) matters to the stage, which copies items, and to the search, which reads them.
template <class ItemT>
struct SweepIndex {         // M items in curve order, boxes over runs of 256, sub-boxes over runs of 32
    typedef ItemT Item;
    int M, nboxes;
    const Item *__restrict__ pts;
    const float4 *__restrict__ boxes, *__restrict__ subboxes;
    __device__ __forceinline__ int nsub() const { return (M + kSweepSub - 1) / kSweepSub; }
};

template <class Item>
struct SweepLdsOf {         // wave-private: 2 816 bytes for points, 3 840 for triangles
    Item run[kSweepSub];
    uint32_t box[64], sub[64 * kSweepSubs];
};

__device__ __forceinline__ float rl(float v, int k)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}

// Ballot compaction: the lanes with `keep` write v to dst in lane order; the count of them.
__device__ __forceinline__ int wave_compact(bool keep, uint32_t v, uint32_t *dst)
{
    const uint64_t m = __ballot(keep);
    if (keep) dst[__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = v;
    return __builtin_popcountll(m);
}

// a run's 32 items -> LDS, for every lane to scan
template <class Item>
__device__ __forceinline__ void stage(SweepLdsOf<Item> &lds, const Item &p)
{
    __builtin_amdgcn_wave_barrier();
    if (threadIdx.x < kSweepSub) lds.run[threadIdx.x] = p;
    __syncthreads();
}

// A triangle of an index: the three vertices, the face index in a.w
struct TriItem { float4 a, b, c; };
typedef SweepIndex<TriItem> TriIndex;

// the face's vertices; false for an index outside [0, V) (*bad_index) or a non-finite coordinate
__device__ __forceinline__ bool tri_load(int V, const float *__restrict__ vertices, const int32_t *__restrict__ faces, size_t f,
                                         float4 &a, float4 &b, float4 &c, bool *bad_index)
{
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    a = b = c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    *bad_index = i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V;
    if (*bad_index) return false;
    const float4 ta = make_float4(vertices[3 * (size_t)i0], vertices[3 * (size_t)i0 + 1], vertices[3 * (size_t)i0 + 2], 0.0f);
    const float4 tb = make_float4(vertices[3 * (size_t)i1], vertices[3 * (size_t)i1 + 1], vertices[3 * (size_t)i1 + 2], 0.0f);
    const float4 tc = make_float4(vertices[3 * (size_t)i2], vertices[3 * (size_t)i2 + 1], vertices[3 * (size_t)i2 + 2], 0.0f);
    auto finite = [](const float4 v) { return fabsf(v.x) <= FLT_MAX && fabsf(v.y) <= FLT_MAX && fabsf(v.z) <= FLT_MAX; };
    if (!(finite(ta) && finite(tb) && finite(tc))) return false;
    a = ta; b = tb; c = tc;
    return true;
}

}  // namespace sls
