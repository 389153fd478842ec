// sls_sweep.hpp — the ONE exact spatial search of the project and what it stands on, for every file that searches an index:
// the shape of an index (items in curve order, boxes over runs of 256, sub-boxes over runs of 32), its wave-private LDS, the
// lane broadcast and the ballot compaction, the triangle item with its guarded load; store_boxes, which every index build
// ends with; and the sweep itself (knn_sweep) behind its two fronts — nn_search for queries of another cloud, self_search
// for a cloud queried by itself.  Its users: the point searches (sls_knn.hip), the point-to-mesh distance
// (sls_meshdist.hip), the radius searches of the clustering (sls_cluster.hip); the ray traversal (sls_raycast.hip) walks
// the same index with a test of its own.  The host side of an index, its layouts and builds, is declared in sls_launch.hpp.
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

typedef SweepIndex<float4> KnnIndex;       // a cloud in curve order (knn_build)

typedef SweepLdsOf<float4> SweepLds;

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

// a bounding box (mn, mx) grown to hold another one
__device__ __forceinline__ void box_join(float4 &mn, float4 &mx, const float4 omn, const float4 omx)
{
    mn = make_float4(fminf(mn.x, omn.x), fminf(mn.y, omn.y), fminf(mn.z, omn.z), 0.0f);
    mx = make_float4(fmaxf(mx.x, omx.x), fmaxf(mx.y, omx.y), fmaxf(mx.z, omx.z), 0.0f);
}

// ... by the box of the lane `off` away: one step of a butterfly
__device__ __forceinline__ void box_merge(float4 &mn, float4 &mx, int off)
{
    box_join(mn, mx, make_float4(__shfl_xor(mn.x, off, 64), __shfl_xor(mn.y, off, 64), __shfl_xor(mn.z, off, 64), 0.0f),
             make_float4(__shfl_xor(mx.x, off, 64), __shfl_xor(mx.y, off, 64), __shfl_xor(mx.z, off, 64), 0.0f));
}

// One block per box of kSweepBox == blockDim.x items, (mn, mx) the thread's item's box (none: min > max): the boxes of the
// block's 8 runs and of the block itself
__device__ __forceinline__ void store_boxes(float4 mn, float4 mx, float4 *__restrict__ boxes, float4 *__restrict__ subboxes)
{
    __shared__ float4 s_mn[4], s_mx[4];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) box_merge(mn, mx, off);
    if ((threadIdx.x & (kSweepSub - 1)) == 0) {   // tight boxes over runs of 32 points (empty run: min > max)
        const size_t sb = (size_t)blockIdx.x * kSweepSubs + threadIdx.x / kSweepSub;
        subboxes[2 * sb] = mn;
        subboxes[2 * sb + 1] = mx;
    }
    box_merge(mn, mx, 32);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {                     // (its own box is wave 0's)
        for (int w = 1; w < 4; ++w) box_join(mn, mx, s_mn[w], s_mx[w]);
        boxes[2 * blockIdx.x] = mn;
        boxes[2 * blockIdx.x + 1] = mx;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The sweep: the ONE exact spatial search of all the query kernels.  One WAVE per 64 curve-consecutive queries (lane =
// query), the workgroup IS the wave: no workgroup waits on another, every loop is bounded by the box count.  A kernel sets
// up its queries and a SEARCH (what a lane keeps of the targets it is shown), scans one box for a first bound (its own, or
// the one a binary search names) and calls knn_sweep for the others:
//   1. chunks of 64 boxes (256 points each), outwards from the scanned box, so the bounds shrink early;
//   2. lane = box: a box is listed if its gap to the wave's bounding box beats the wave's worst bound AND its gap to the box
//      of one of the 8 groups of 8 consecutive queries beats that group's worst bound (one bound for all 64 would be ruined
//      by a single isolated query, or by a sparse stretch of the curve whose box swallows the dense regions in between);
//   3. the listed boxes' sub-boxes (32 points; even a Hilbert run of 256 is loose) pass the same test, 8 boxes per step,
//      lane = (box slot, sub-box), into a wave-private LDS list;
//   4. 64 listed sub-boxes at a time, lane = candidate: the point-to-box gap against EACH query's own bound (broadcast
//      with v_readlane); a run that can still matter to one goes through LDS to all lanes, the next one fetched meanwhile.
// A search supplies bound(), the squared distance beyond which a target cannot matter to the lane (+inf while anything
// would); scan(s_run), which shows it 32 staged targets; pad(pts, r0), the point that fills a short last run from r0 on.
// Exact whatever the search, because
//   * every gap test is `gap * 0.99999f <= bound`: equality passes, a gap never exceeds the distance to a point inside the
//     box (float subtraction, fma and max are monotone) and bounds only shrink, so a target that could enter or tie with
//     what a lane holds — an equally near one of lower index in another box — is always shown to it;
//   * sweep_chunk permutes the chunks and a run is listed once: no target is shown twice, which a search that COUNTS what
//     it meets (the list) needs, and one shown for another lane's sake lies beyond this lane's bound;
//   * each pad() changes nothing, for the reason given there.
// (TriBestSearch's d2 is a longer float32 computation than a point's: it may fall below the true distance by 2e-7 of the
// scale, so there the argument holds up to that — the returned face is a nearest one within the header's own error, and
// exact duplicates, equal to the bit, still resolve to the lower index wherever the 1e-5 slack covers that error.)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float box_gap2(const float4 amn, const float4 amx, const float4 bmn, const float4 bmx)
{
    const float gx = fmaxf(fmaxf(bmn.x - amx.x, amn.x - bmx.x), 0.0f);
    const float gy = fmaxf(fmaxf(bmn.y - amx.y, amn.y - bmx.y), 0.0f);
    const float gz = fmaxf(fmaxf(bmn.z - amx.z, amn.z - bmx.z), 0.0f);
    return fmaf(gz, gz, fmaf(gy, gy, gx * gx));
}

// the conservative test of every level: relative slack 1e-5, and equality passes
__device__ __forceinline__ bool within(float gap2, float bound) { return gap2 * 0.99999f <= bound; }

// bounding boxes of the 8 groups of 8 consecutive queries (dead lanes: empty), valid in every lane of the group
__device__ __forceinline__ void group_boxes(bool live, const float4 me, float4 &gmn, float4 &gmx)
{
    gmn = live ? me : make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.0f);
    gmx = live ? me : make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f);
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) box_merge(gmn, gmx, off);
}

// chunks outwards from c0: c0, c0+1, c0-1, c0+2, ... while both sides exist, then the rest of the longer side
__device__ __forceinline__ int sweep_chunk(int it, int c0, int nchunks)
{
    const int near = min(c0, nchunks - 1 - c0);            // both sides available for 2*near steps
    if (it <= 2 * near) return c0 + ((it & 1) ? (it + 1) / 2 : -(it / 2));
    return (c0 < nchunks - 1 - c0) ? it : nchunks - 1 - it;
}

// item `lane & 31` of run sb for the LDS stage; LOW: loaded by lanes 0..31 alone, the ones that stage it
template <bool LOW, class Index, class Search>
__device__ __forceinline__ typename Index::Item run_point(const Index &ix, int sb, const Search &s)
{
    const int r0 = sb * kSweepSub, i = r0 + ((int)threadIdx.x & (kSweepSub - 1));
    if (LOW && threadIdx.x >= kSweepSub) return typename Index::Item{};
    return i < ix.M ? ix.pts[i] : s.pad(ix.pts, r0);
}

template <class Index, class Search>
__device__ __forceinline__ void knn_sweep(const Index &ix, const int start_box, const bool live, const float4 me,
                                          const float4 wmn, const float4 wmx, const float4 gmn, const float4 gmx, Search &s,
                                          SweepLdsOf<typename Index::Item> &lds)
{
    typedef typename Index::Item Item;
    const int lane = threadIdx.x, nboxes = ix.nboxes, nsub = ix.nsub();   // start_box: scanned by the caller, skipped here
    const int nchunks = (nboxes + 63) / 64, c0 = start_box / 64;
    for (int it = 0; it < nchunks; ++it) {
        // the worst bound of my group of 8, and of the wave
        float gB = live ? s.bound() : 0.0f;
        gB = fmaxf(gB, __shfl_xor(gB, 1, 64)); gB = fmaxf(gB, __shfl_xor(gB, 2, 64)); gB = fmaxf(gB, __shfl_xor(gB, 4, 64));
        float B2 = gB;
#pragma unroll
        for (int off = 8; off < 64; off <<= 1) B2 = fmaxf(B2, __shfl_xor(B2, off, 64));
        auto reaches = [&](const float4 bmn, const float4 bmx) -> bool {
            if (!within(box_gap2(wmn, wmx, bmn, bmx), B2)) return false;
            bool r = false;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 mn = make_float4(rl(gmn.x, 8 * g), rl(gmn.y, 8 * g), rl(gmn.z, 8 * g), 0.0f);
                const float4 mx = make_float4(rl(gmx.x, 8 * g), rl(gmx.y, 8 * g), rl(gmx.z, 8 * g), 0.0f);
                r = r || within(box_gap2(mn, mx, bmn, bmx), rl(gB, 8 * g));
            }
            return r;
        };
        // 2. the chunk's boxes, lane = box
        const int b = sweep_chunk(it, c0, nchunks) * 64 + lane;
        bool c = false;
        if (b < nboxes && b != start_box) c = reaches(ix.boxes[2 * b], ix.boxes[2 * b + 1]);
        __builtin_amdgcn_wave_barrier();
        const int nb = wave_compact(c, (uint32_t)b, lds.box);
        if (nb == 0) continue;
        __syncthreads();
        // 3. their sub-boxes, 8 boxes per step
        int ns = 0;                                     // <= 8 * nb <= 512 = the size of lds.sub
        for (int g = 0; g < nb; g += 8) {
            const int slot = g + (lane >> 3);
            bool cs = false;
            uint32_t sb = 0;
            if (slot < nb) {
                sb = lds.box[slot] * kSweepSubs + (uint32_t)(lane & 7);
                if ((int)sb < nsub) cs = reaches(ix.subboxes[2 * (size_t)sb], ix.subboxes[2 * (size_t)sb + 1]);
            }
            ns += wave_compact(cs, sb, lds.sub + ns);
        }
        __syncthreads();
        // 4. the listed runs, 64 at a time
        for (int base = 0; base < ns; base += 64) {
            const int nk = min(64, ns - base);
            const uint32_t sbl = lds.sub[base + min(lane, nk - 1)];
            const float4 mnl = ix.subboxes[2 * (size_t)sbl], mxl = ix.subboxes[2 * (size_t)sbl + 1];
            const float qb2 = live ? s.bound() : -1.0f;
            bool need = false;
            for (int qi = 0; qi < 64; ++qi) {
                const float4 qp = make_float4(rl(me.x, qi), rl(me.y, qi), rl(me.z, qi), 0.0f);
                need = need || within(box_gap2(qp, qp, mnl, mxl), rl(qb2, qi));
            }
            uint64_t todo = __ballot(need && lane < nk);
            Item pre = Item{};
            if (todo) pre = run_point<false>(ix, __builtin_amdgcn_readlane((int)sbl, __builtin_ctzll(todo)), s);
            while (todo) {
                todo &= todo - 1;
                const Item cur = pre;
                if (todo) pre = run_point<false>(ix, __builtin_amdgcn_readlane((int)sbl, __builtin_ctzll(todo)), s);
                stage(lds, cur);
                s.scan(lds.run);
            }
        }
    }
}

// The body of a query kernel behind its set-up, the queries being ANOTHER cloud's: the start box is the one holding the
// first target whose code is not below the wave's first code; its runs give a first bound; the wave's box is a
// reduction over its own queries.
template <class Index, class Search>
__device__ __forceinline__ void nn_search(const Index &ix, const uint32_t *__restrict__ tkeys, const uint32_t code,
                                          const bool live, const float4 me, Search &s, SweepLdsOf<typename Index::Item> &lds)
{
    int lo = 0, hi = ix.M;                              // lower bound in tkeys[0, M): at most 31 halvings
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tkeys[mid] < code) lo = mid + 1; else hi = mid;
    }
    const int start_box = __builtin_amdgcn_readfirstlane(min(lo, ix.M - 1) / kSweepBox);
    for (int t = 0; t < kSweepSubs; ++t) {
        const int sb = start_box * kSweepSubs + t;
        if (sb >= ix.nsub()) break;
        stage(lds, run_point<true>(ix, sb, s));
        s.scan(lds.run);
    }
    float4 gmn, gmx;
    group_boxes(live, me, gmn, gmx);
    float4 wmn = gmn, wmx = gmx;
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) box_merge(wmn, wmx, off);
    knn_sweep(ix, start_box, live, me, wmn, wmx, gmn, gmx, s, lds);
}

// ... the queries being the indexed cloud ITSELF, wave w its points 64 w ..: the wave's own box in full, then the sweep
// over the others.  A point is shown itself (knn_query_kernel, which leaves it out, scans its own box by a loop of its own)
template <class Search>
__device__ __forceinline__ void self_search(const KnnIndex &ix, const bool live, const float4 me, Search &s, SweepLds &lds)
{
    const int own_box = (blockIdx.x * 64) / kSweepBox, own_sub0 = (blockIdx.x * 64) / kSweepSub, nsub = ix.nsub();
    for (int t = 0; t < kSweepSubs; ++t) {
        const int sb = own_box * kSweepSubs + ((t + (own_sub0 % kSweepSubs)) % kSweepSubs);
        if (sb >= nsub) continue;
        stage(lds, run_point<true>(ix, sb, s));
        s.scan(lds.run);
    }
    float4 wmn = ix.subboxes[2 * (size_t)own_sub0], wmx = ix.subboxes[2 * (size_t)own_sub0 + 1];
    if (own_sub0 + 1 < nsub) box_join(wmn, wmx, ix.subboxes[2 * (size_t)own_sub0 + 2], ix.subboxes[2 * (size_t)own_sub0 + 3]);
    float4 gmn, gmx;
    group_boxes(live, me, gmn, gmx);
    knn_sweep(ix, own_box, live, me, wmn, wmx, gmn, gmx, s, lds);
}

}  // namespace sls
