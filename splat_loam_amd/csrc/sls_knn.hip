// sls_knn.hip — simple-knn's distCUDA2 for MI355X:
// out[i] = mean of the squared distances from point i to its 3 nearest
// other points (slam/mapper.py:113-115, scene/gaussian_model.py:77-81).
//
// Exact 3-NN, built for LiDAR-like (very non-uniform) clouds:
//   1. bounding cube, 30-bit Hilbert-curve index per point;
//   2. wave64 LSD radix sort of (code, index) — the sorter of sls_radix.hip;
//   3. points gathered in curve order (float4: xyz + original index) and
//      axis-aligned boxes over runs of 256 consecutive points;
//   4. one wave per 64 consecutive points, one lane per point: the own box first for a tight bound, then the sweep
//      (knn_sweep below) over the other boxes; the two-cloud searches (sls_nn_query, sls_nn_query_k) run it too, and so
//      does the point-to-mesh distance (sls_mesh_distance), whose index holds triangles, and so do the three radius
//      searches of sls_cloud_dbscan (count, unite, border: at the end of this file).
// Squared distances use the fixed expression fma(dz,dz,fma(dy,dy,dx*dx)), so
// the result is reproducible bit for bit by a CPU brute force.
#include <float.h>

#include "sls_sweep.hpp"
#include "../../include/sls_nn_math.h"
#include "../../include/sls_meshdist_math.h"
#include "../../include/sls_outlier_math.h"
#include "../../include/sls_cluster_math.h"
#include "sls_unionfind.hpp"

namespace sls {

constexpr int kKnnBox = 256;
constexpr int kKnnSub = kSweepSub;              // points per sub-box
constexpr int kKnnSubs = kSweepSubs;            // 8 sub-boxes per box
static_assert(kKnnBox == kSweepBox, "the boxes of this file are the sweep's (sls_sweep.hpp)");

__global__ void knn_init_bbox_kernel(uint32_t *bbox, uint32_t M, uint32_t M2)
{
    if (threadIdx.x < 3) bbox[threadIdx.x] = 0xFFFFFFFFu;       // min (ordered domain)
    else if (threadIdx.x < 6) bbox[threadIdx.x] = 0u;           // max
    else if (threadIdx.x == 6) bbox[6] = M;                     // item count for the sorter
    else if (threadIdx.x == 7) bbox[7] = M2;                    // ... and of the second cloud's sort (sls_nn_query)
}

__global__ __launch_bounds__(256) void knn_bbox_kernel(int M, const float *__restrict__ xyz, uint32_t *bbox)
{
    float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = xyz[3 * i + k];
            mn[k] = fminf(mn[k], v);
            mx[k] = fmaxf(mx[k], v);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
        }
    }
    // block combine in LDS, then 6 global atomics per block (same-address global atomics serialise)
    __shared__ uint32_t s_box[6];
    if (threadIdx.x < 6) s_box[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(&s_box[k], f2ord(mn[k]));
            atomicMax(&s_box[3 + k], f2ord(mx[k]));
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&bbox[threadIdx.x], s_box[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&bbox[threadIdx.x], s_box[threadIdx.x]);
}

__global__ __launch_bounds__(256) void knn_morton_kernel(int M, const float *__restrict__ xyz,
                                                         const uint32_t *__restrict__ bbox,
                                                         uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, int key_bits)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    keys[i] = curve_code(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], bbox, key_bits);
    vals[i] = (uint32_t)i;
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

// One block per box of kKnnBox == blockDim.x items, (mn, mx) the thread's item's box (none: min > max): the boxes of the
// block's 8 runs and of the block itself
__device__ __forceinline__ void store_boxes(float4 mn, float4 mx, float4 *__restrict__ boxes, float4 *__restrict__ subboxes)
{
    __shared__ float4 s_mn[4], s_mx[4];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) box_merge(mn, mx, off);
    if ((threadIdx.x & (kKnnSub - 1)) == 0) {   // tight boxes over runs of 32 points (empty run: min > max)
        const size_t sb = (size_t)blockIdx.x * kKnnSubs + threadIdx.x / kKnnSub;
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

__global__ __launch_bounds__(256) void knn_gather_boxes_kernel(int M, const float *__restrict__ xyz,
                                                               const uint32_t *__restrict__ sorted_idx,
                                                               float4 *__restrict__ pts, float4 *__restrict__ boxes,
                                                               float4 *__restrict__ subboxes)
{
    const int j = blockIdx.x * kKnnBox + threadIdx.x;
    float4 mn = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.0f), mx = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f);
    if (j < M) {
        const uint32_t i = sorted_idx[j];
        mn = mx = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
        pts[j] = make_float4(mn.x, mn.y, mn.z, __uint_as_float(i));
    }
    store_boxes(mn, mx, boxes, subboxes);
}

// ---------------------------------------------------------------------------------------------------------------------
// The sweep: the ONE exact spatial search of all four query kernels.  One WAVE per 64 curve-consecutive queries (lane =
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
typedef SweepIndex<float4> KnnIndex;       // a cloud in curve order (knn_build)

typedef SweepLdsOf<float4> SweepLds;

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
    const int r0 = sb * kKnnSub, i = r0 + ((int)threadIdx.x & (kKnnSub - 1));
    if (LOW && threadIdx.x >= kKnnSub) return typename Index::Item{};
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
                sb = lds.box[slot] * kKnnSubs + (uint32_t)(lane & 7);
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

// The body of both nn_* kernels behind their set-up, the queries being ANOTHER cloud's: the start box is the one holding
// the first target whose code is not below the wave's first code; its runs give a first bound; the wave's box is a
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
    const int start_box = __builtin_amdgcn_readfirstlane(min(lo, ix.M - 1) / kKnnBox);
    for (int t = 0; t < kKnnSubs; ++t) {
        const int sb = start_box * kKnnSubs + t;
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

// sls_knn_dist2: the three smallest squared distances to OTHER points of the same cloud
__device__ __forceinline__ void best3_update(float d2, float &b0, float &b1, float &b2)
{   // insertion into the sorted triple b0 <= b1 <= b2, branch-free (nested ifs end up as an indexed
    // stack array here: scratch traffic in the innermost loop)
    const float u0 = fmaxf(b0, d2);
    b0 = fminf(b0, d2);
    const float u1 = fmaxf(b1, u0);
    b1 = fminf(b1, u0);
    b2 = fminf(b2, u1);
}

struct Best3Search {
    const float4 me;
    float b0, b1, b2;
    __device__ __forceinline__ float bound() const { return b2; }
    // a far point: its d2 overflows to +inf, which lowers no entry of the triple
    __device__ __forceinline__ float4 pad(const float4 *, int) const { return make_float4(1.0e30f, 1.0e30f, 1.0e30f, 0.0f); }
    // SELF: the lane's own point, at s_run[self], is left out
    template <bool SELF = false>
    __device__ __forceinline__ void scan(const float4 *s_run, int self = -1)
    {
#pragma unroll 8
        for (int k = 0; k < kKnnSub; ++k) {
            const float4 p = s_run[k];
            const float d2 = sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z);
            best3_update((SELF && k == self) ? FLT_MAX : d2, b0, b1, b2);
        }
    }
};

__global__ __launch_bounds__(64) void knn_query_kernel(int M, int nboxes, const float4 *__restrict__ pts,
                                                       const float4 *__restrict__ boxes,
                                                       const float4 *__restrict__ subboxes, float *__restrict__ out, uint32_t Mq)
{
    __shared__ SweepLds lds;
    const KnnIndex ix = { M, nboxes, pts, boxes, subboxes };
    const int q = blockIdx.x * 64 + threadIdx.x;
    const float4 me = pts[q < M ? q : M - 1];
    // Mq < M (sls_knn_dist2_first): only the points whose ORIGINAL index is below Mq are queries — Mapper.densify asks
    // for the new surfels' distances among new + existing centres (slam/mapper.py:109-117) and drops the rest.  A wave
    // of 64 neighbours on the curve without one leaves; the others search exactly as they would
    const bool live = q < M && __float_as_uint(me.w) < Mq;
    if (!__ballot(live)) return;
    const int own_box = (blockIdx.x * 64) / kKnnBox, own_sub0 = (blockIdx.x * 64) / kKnnSub;   // my runs: own_sub0, +1
    const int nsub = ix.nsub();
    Best3Search s = { me, FLT_MAX, FLT_MAX, FLT_MAX };

    // the own box for a first bound: my two runs, then the other six; every lane leaves itself out
    for (int t = 0; t < kKnnSubs; ++t) {
        const int sb = own_box * kKnnSubs + ((t + (own_sub0 % kKnnSubs)) % kKnnSubs);
        if (sb >= nsub) continue;
        stage(lds, run_point<true>(ix, sb, s));
        s.scan<true>(lds.run, (live && (q / kKnnSub) == sb) ? (q % kKnnSub) : -1);
    }

    // the wave's bounding box is that of its two runs (dead and non-query lanes included), the groups' are of live lanes
    float4 wmn = subboxes[2 * (size_t)own_sub0], wmx = subboxes[2 * (size_t)own_sub0 + 1];
    if (own_sub0 + 1 < nsub) box_join(wmn, wmx, subboxes[2 * (size_t)own_sub0 + 2], subboxes[2 * (size_t)own_sub0 + 3]);
    float4 gmn, gmx;
    group_boxes(live, me, gmn, gmx);
    knn_sweep(ix, own_box, live, me, wmn, wmx, gmn, gmx, s, lds);
    if (live) out[__float_as_uint(me.w)] = (s.b0 + s.b1 + s.b2) / 3.0f;
}

// scratch layout (all 256-byte aligned)
struct KnnScratch {
    uint32_t *bbox;
    uint32_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp;
    float4 *pts, *boxes, *subboxes;
    void *sort;
    size_t sort_bytes, total;
};

// sort_items: what the sorter's scratch, the last piece, is sized for
static KnnScratch knn_layout(int M, void *base, int sort_items)
{
    const size_t nboxes = (size_t)((M + kKnnBox - 1) / kKnnBox);
    Arena a(base);
    KnnScratch s;
    s.bbox = a.take<uint32_t>(8);
    s.keys = a.take<uint32_t>((size_t)M);
    s.keys_tmp = a.take<uint32_t>((size_t)M);
    s.vals = a.take<uint32_t>((size_t)M);
    s.vals_tmp = a.take<uint32_t>((size_t)M);
    s.pts = a.take<float4>((size_t)M);
    s.boxes = a.take<float4>(2 * nboxes);
    s.subboxes = a.take<float4>(2 * nboxes * kKnnSubs);
    s.sort_bytes = sort_scratch_bytes((uint64_t)sort_items);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t knn_scratch_bytes(int M) { return M > 0 ? knn_layout(M, nullptr, M).total : 0; }

// The front half of both searches: bounding cube, Hilbert codes, sort, points in curve order, boxes and sub-boxes.
// M2: the item count of a second sort that follows (bbox[7]).  *which: where the sorted (code, index) pairs ended up.
static int knn_build(int M, const float *xyz, const KnnScratch &s, int key_bits, uint32_t M2, hipStream_t st, int *which)
{
    const int nb = (M + 255) / 256;
    hipLaunchKernelGGL(knn_init_bbox_kernel, dim3(1), dim3(64), 0, st, s.bbox, (uint32_t)M, M2);
    SLS_LAUNCH_CHECK("knn_init_bbox_kernel");
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(nb < 256 ? nb : 256), dim3(256), 0, st, M, xyz, s.bbox);
    SLS_LAUNCH_CHECK("knn_bbox_kernel");
    hipLaunchKernelGGL(knn_morton_kernel, dim3(nb), dim3(256), 0, st, M, xyz, s.bbox, s.keys, s.vals, key_bits);
    SLS_LAUNCH_CHECK("knn_morton_kernel");
    int rc = radix_sort_pairs_u32(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.bbox + 6, (uint32_t)M, key_bits, s.sort,
                                  s.sort_bytes, which, st);
    if (rc) return rc;
    const int nboxes = (M + kKnnBox - 1) / kKnnBox;
    hipLaunchKernelGGL(knn_gather_boxes_kernel, dim3(nboxes), dim3(kKnnBox), 0, st, M, xyz,
                       *which ? s.vals_tmp : s.vals, s.pts, s.boxes, s.subboxes);
    SLS_LAUNCH_CHECK("knn_gather_boxes_kernel");
    return SLS_OK;
}

// small clouds are sorted on 21 code bits (knn_morton_kernel)
static int knn_key_bits(int M) { return M <= 200000 ? 21 : 30; }

int launch_knn(int M, const float *xyz, float *out, void *scratch, size_t scratch_bytes, hipStream_t st, int Mq)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    if (scratch_bytes < s.total) {
        set_error("knn scratch too small: %zu < %zu", scratch_bytes, s.total);
        return SLS_E_SCRATCH;
    }
    if (((uintptr_t)scratch & 255) != 0) {
        set_error("knn scratch must be 256-byte aligned");
        return SLS_E_ARG;
    }
    ScopedTimer tm(T_KNN, st);
    int which = 0;
    int rc = knn_build(M, xyz, s, knn_key_bits(M), 0u, st, &which);
    if (rc) return rc;
    const int nboxes = (M + kKnnBox - 1) / kKnnBox;
    static_assert(kKnnBox == 256 && kKnnSub == 32, "the query kernel's lane mappings are written for 8 runs of 32");
    hipLaunchKernelGGL(knn_query_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, nboxes, s.pts, s.boxes, s.subboxes, out,
                       (uint32_t)(Mq < 0 || Mq > M ? M : Mq));
    SLS_LAUNCH_CHECK("knn_query_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sls_nn_query: for every point of a SECOND cloud the nearest point of the indexed one — squared distance and the lowest
// original index attaining it (include/sls_nn_math.h).  The queries are sorted along the target's curve (nn_front below)
// and searched by nn_search above; the search is ONE packed key (bits(d2) << 32 | index), minimised, so the lowest index
// among equally near targets wins.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn_gather_kernel(int Mq, const float *__restrict__ xyz,
                                                        const uint32_t *__restrict__ sorted_idx, float4 *__restrict__ qpts)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Mq) return;
    const uint32_t i = sorted_idx[j];
    qpts[j] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
}

struct BestKeySearch {
    const float4 me;
    uint64_t best;
    __device__ __forceinline__ float bound() const { return sls_nn_key_dist2(best); }
    // a copy of the run's first point: a minimum meets it twice and does not change, so no sentinel distance exists
    __device__ __forceinline__ float4 pad(const float4 *__restrict__ pts, int r0) const { return pts[r0]; }
    __device__ __forceinline__ void scan(const float4 *s_run)
    {
#pragma unroll 8
        for (int k = 0; k < kKnnSub; ++k) {
            const float4 p = s_run[k];
            const uint64_t key = sls_nn_key(sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z), __float_as_uint(p.w));
            best = key < best ? key : best;
        }
    }
};

__global__ __launch_bounds__(64) void nn_query_kernel(int Mt, int nboxes, const float4 *__restrict__ pts,
                                                      const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                      const uint32_t *__restrict__ tkeys, int Mq,
                                                      const float4 *__restrict__ qpts, const uint32_t *__restrict__ qkeys,
                                                      float *__restrict__ out_dist2, int32_t *__restrict__ out_index)
{
    __shared__ SweepLds lds;
    const KnnIndex ix = { Mt, nboxes, pts, boxes, subboxes };
    const int q0 = blockIdx.x * 64, q = q0 + threadIdx.x;   // (the grid has ceil(Mq / 64) waves: q0 < Mq)
    const bool live = q < Mq;
    const float4 me = qpts[live ? q : Mq - 1];
    BestKeySearch s = { me, SLS_NN_KEY_NONE };
    nn_search(ix, tkeys, qkeys[q0], live, me, s, lds);
    if (live) {
        const uint32_t i = __float_as_uint(me.w);
        out_dist2[i] = sls_nn_key_dist2(s.best);
        if (out_index) out_index[i] = (int32_t)sls_nn_key_index(s.best);
    }
}

// scratch: the target's index (KnnScratch, its sorter scratch sized for the larger cloud), then the queries' buffers
struct NnScratch {
    KnnScratch t;
    uint32_t *qkeys, *qkeys_tmp, *qvals, *qvals_tmp;
    float4 *qpts;
    size_t total;
};

static NnScratch nn_layout(int Mt, int Mq, void *base)
{
    NnScratch s;
    s.t = knn_layout(Mt, base, Mt > Mq ? Mt : Mq);
    Arena a(base);
    a.off = s.t.total;
    s.qkeys = a.take<uint32_t>((size_t)Mq);
    s.qkeys_tmp = a.take<uint32_t>((size_t)Mq);
    s.qvals = a.take<uint32_t>((size_t)Mq);
    s.qvals_tmp = a.take<uint32_t>((size_t)Mq);
    s.qpts = a.take<float4>((size_t)Mq);
    s.total = a.off < (size_t)SLS_NN_STATS_SCRATCH_BYTES ? (size_t)SLS_NN_STATS_SCRATCH_BYTES : a.off;
    return s;
}

size_t nn_scratch_bytes(int Mt, int Mq) { return (Mt > 0 && Mq >= 0) ? nn_layout(Mt, Mq, nullptr).total : 0; }

// What both two-cloud launchers do before their query kernel: the target's index, then the queries' codes in the TARGET's
// cube (knn_morton_kernel clamps to the border cells outside), the same sorter and the gather in curve order.  self_ok: a
// cloud queried by itself is its own sorted query set, and the second code / sort / gather is skipped.
struct NnFront {
    NnScratch s;
    const uint32_t *tkeys, *qkeys;      // the sorted codes of the targets and of the queries
    const float4 *qpts;
};

// the target half: its index, built once.  Mq: the item count of the queries' sort that follows (bbox[7])
static int nn_front_target(int Mt, const float *target_xyz, int Mq, void *scratch, hipStream_t st, NnFront *f)
{
    const NnScratch &s = f->s = nn_layout(Mt, Mq, scratch);
    int which = 0;
    const int rc = knn_build(Mt, target_xyz, s.t, knn_key_bits(Mt), (uint32_t)Mq, st, &which);
    if (rc) return rc;
    f->tkeys = f->qkeys = which ? s.t.keys_tmp : s.t.keys;
    f->qpts = s.t.pts;
    return SLS_OK;
}

// the query half behind codes that are already in s.qkeys / s.qvals: the sort and the gather in curve order
static int nn_front_sorted_queries(int Mt, int Mq, const float *query_xyz, hipStream_t st, NnFront *f)
{
    const NnScratch &s = f->s;
    int qwhich = 0;
    const int rc = radix_sort_pairs_u32(s.qkeys, s.qvals, s.qkeys_tmp, s.qvals_tmp, s.t.bbox + 7, (uint32_t)Mq, knn_key_bits(Mt),
                                        s.t.sort, s.t.sort_bytes, &qwhich, st);
    if (rc) return rc;
    hipLaunchKernelGGL(nn_gather_kernel, dim3((Mq + 255) / 256), dim3(256), 0, st, Mq, query_xyz,
                       qwhich ? s.qvals_tmp : s.qvals, s.qpts);
    SLS_LAUNCH_CHECK("nn_gather_kernel");
    f->qkeys = qwhich ? s.qkeys_tmp : s.qkeys;
    f->qpts = s.qpts;
    return SLS_OK;
}

static int nn_front(int Mt, const float *target_xyz, int Mq, const float *query_xyz, bool self_ok, void *scratch, hipStream_t st,
                    NnFront *f)
{
    int rc = nn_front_target(Mt, target_xyz, Mq, scratch, st, f);
    if (rc) return rc;
    if (self_ok && query_xyz == target_xyz && Mq == Mt) return SLS_OK;
    hipLaunchKernelGGL(knn_morton_kernel, dim3((Mq + 255) / 256), dim3(256), 0, st, Mq, query_xyz, f->s.t.bbox, f->s.qkeys,
                       f->s.qvals, knn_key_bits(Mt));
    SLS_LAUNCH_CHECK("knn_morton_kernel");
    return nn_front_sorted_queries(Mt, Mq, query_xyz, st, f);
}

static int nn_query_launch(int Mt, int Mq, const NnFront &f, float *out_dist2, int32_t *out_index, hipStream_t st)
{
    hipLaunchKernelGGL(nn_query_kernel, dim3((Mq + 63) / 64), dim3(64), 0, st, Mt, (Mt + kKnnBox - 1) / kKnnBox, f.s.t.pts,
                       f.s.t.boxes, f.s.t.subboxes, f.tkeys, Mq, f.qpts, f.qkeys, out_dist2, out_index);
    SLS_LAUNCH_CHECK("nn_query_kernel");
    return SLS_OK;
}

int launch_nn_query(int Mt, const float *target_xyz, int Mq, const float *query_xyz, float *out_dist2, int32_t *out_index,
                    void *scratch, hipStream_t st)
{
    ScopedTimer tm(T_KNN, st);
    NnFront f;
    const int rc = nn_front(Mt, target_xyz, Mq, query_xyz, false, scratch, st, &f);
    if (rc) return rc;
    return nn_query_launch(Mt, Mq, f, out_dist2, out_index, st);
}

// One target index queried many times (sls_icp.hip).  nn_index_target builds it and names where the caller's own kernel
// writes the queries' codes (curve_code in the target's cube) and the identity; nn_index_query then sorts them, gathers
// the queries from query_xyz and runs nn_query_kernel, as launch_nn_query does behind its code kernel.
int nn_index_target(int Mt, const float *target_xyz, int Mq, void *scratch, hipStream_t st, NnIndexRef *ref)
{
    NnFront f;
    const int rc = nn_front_target(Mt, target_xyz, Mq, scratch, st, &f);
    if (rc) return rc;
    ref->bbox = f.s.t.bbox; ref->tkeys = f.tkeys; ref->qkeys = f.s.qkeys; ref->qvals = f.s.qvals; ref->key_bits = knn_key_bits(Mt);
    return SLS_OK;
}

int nn_index_query(int Mt, int Mq, const float *query_xyz, const NnIndexRef &ref, float *out_dist2, int32_t *out_index, void *scratch,
                   hipStream_t st)
{
    NnFront f;
    f.s = nn_layout(Mt, Mq, scratch);
    f.tkeys = ref.tkeys;
    const int rc = nn_front_sorted_queries(Mt, Mq, query_xyz, st, &f);
    if (rc) return rc;
    return nn_query_launch(Mt, Mq, f, out_dist2, out_index, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// sls_nn_query_k: the k nearest targets of every query (include/sls_outlier_math.h).  The search is a per-lane ascending
// list of K keys in registers (K = 4, 8, 16 or 32, the smallest >= k; every index into it is a compile-time constant after
// unrolling) and its bound the lane's k-th best distance, +inf until k targets are held.  The K - k slots in front are
// filled with the key 0, which nothing beats: the k real entries then live in list[K - k .. K) and list[K - 1] is the k-th
// best whatever k is.  A candidate enters the list on a comparison of WHOLE keys.  Unlike a minimum, a list counts what it
// meets, so it rests on the sweep presenting every target exactly once.
// Beyond k = 32 (sls_cloud_normals alone, up to SLS_NORMALS_NN_MAX = 64) the list is found in TWO passes: the 32 nearest,
// whose last key L goes to a per-query buffer; then, with SECOND set, the k - 32 nearest among the targets with key > L —
// a key names its target, so exactly those the first pass did not list — written behind the first 32 of the row and
// pruned by the second list alone.  (A 64-long register list gave wrong lists on the device: DESIGN.md, "Beyond k = 32".)
// ---------------------------------------------------------------------------------------------------------------------
template <int K, bool SECOND>
struct ListSearch {
    const float4 me;
    const uint64_t floor_key;       // SECOND only: keys up to it belong to the first pass
    uint64_t list[K];
    __device__ __forceinline__ float bound() const { return sls_nn_key_dist2(list[K - 1]); }
    // a point nothing is near to: d2 = +inf and index 0xFFFFFFFF make SLS_NN_KEY_NONE, which never enters
    __device__ __forceinline__ float4 pad(const float4 *, int) const
    {
        return make_float4(1.0e30f, 1.0e30f, 1.0e30f, __uint_as_float(0xFFFFFFFFu));
    }
    __device__ __forceinline__ void scan(const float4 *s_run)
    {
#pragma clang loop unroll_count(K <= 8 ? 4 : 1)
        for (int j = 0; j < kKnnSub; ++j) {
            const float4 p = s_run[j];
            const uint64_t key = sls_nn_key(sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z), __float_as_uint(p.w));
            if (key < list[K - 1] && (!SECOND || key > floor_key)) sls_knn_insert(list, K, key);
        }
    }
};

// stride: the floats (int32s) between two queries' rows of out_dist2 (out_index); floor_keys: SECOND only, by original index
template <int K, bool SECOND>
__global__ __launch_bounds__(64) void nn_query_k_kernel(int Mt, int nboxes, const float4 *__restrict__ pts,
                                                        const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                        const uint32_t *__restrict__ tkeys, int Mq,
                                                        const float4 *__restrict__ qpts, const uint32_t *__restrict__ qkeys, int k,
                                                        float *__restrict__ out_dist2, int32_t *__restrict__ out_index,
                                                        double *__restrict__ out_mean, uint64_t *__restrict__ out_last_key,
                                                        int stride, const uint64_t *__restrict__ floor_keys)
{
    __shared__ SweepLds lds;
    const KnnIndex ix = { Mt, nboxes, pts, boxes, subboxes };
    const int q0 = blockIdx.x * 64, q = q0 + threadIdx.x;   // (the grid has ceil(Mq / 64) waves: q0 < Mq)
    const bool live = q < Mq;
    const float4 me = qpts[live ? q : Mq - 1];
    const int first = K - k;                            // (the launcher guarantees K / 2 < k <= K, or k <= K = 4)
    ListSearch<K, SECOND> s = { me, SECOND ? floor_keys[__float_as_uint(me.w)] : 0ull, {} };
#pragma unroll
    for (int j = 0; j < K; ++j) s.list[j] = j < first ? 0ull : SLS_NN_KEY_NONE;
    nn_search(ix, tkeys, qkeys[q0], live, me, s, lds);
    if (live) {
        const size_t i = __float_as_uint(me.w);
        if (out_dist2 || out_index) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j >= first) {
                    const size_t o = i * (size_t)stride + (size_t)(j - first);
                    if (out_dist2) out_dist2[o] = sls_nn_key_dist2(s.list[j]);
                    if (out_index) out_index[o] = (int32_t)sls_nn_key_index(s.list[j]);    // (SLS_NN_KEY_NONE: -1)
                }
        }
        if (out_mean) out_mean[i] = sls_knn_mean(s.list, K, first, min(k, Mt));
        if (out_last_key) out_last_key[i] = s.list[K - 1];
    }
}

size_t nn_k_scratch_bytes(int Mt, int Mq, int k) { return (k >= 1 && k <= SLS_NN_K_MAX) ? nn_scratch_bytes(Mt, Mq) : 0; }

// one launch of the instantiation whose list length k needs
template <bool SECOND>
static void nnk_launch(int Mt, int Mq, const NnFront &f, int k, float *d2, int32_t *idx, double *mean, uint64_t *last_key,
                       int stride, const uint64_t *floor_keys, hipStream_t st)
{
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((Mq + 63) / 64), dim3(64), 0, st, Mt, (Mt + kKnnBox - 1) / kKnnBox, f.s.t.pts, f.s.t.boxes,
                           f.s.t.subboxes, f.tkeys, Mq, f.qpts, f.qkeys, k, d2, idx, mean, last_key, stride, floor_keys);
    };
    switch (sls_knn_list_length(k)) {
    case 4: go(nn_query_k_kernel<4, SECOND>); break;
    case 8: go(nn_query_k_kernel<8, SECOND>); break;
    case 16: go(nn_query_k_kernel<16, SECOND>); break;
    default: go(nn_query_k_kernel<32, SECOND>); break;
    }
}

int launch_nn_query_k(int Mt, const float *target_xyz, int Mq, const float *query_xyz, int k, int k_max, float *out_dist2,
                      int32_t *out_index, double *out_mean, uint64_t *out_last_key, void *scratch, hipStream_t st)
{
    if (k < 1 || k > k_max || k_max > 2 * SLS_NN_K_MAX || (k > SLS_NN_K_MAX && (out_mean || !out_last_key))) {
        set_error("launch_nn_query_k: k = %d outside [1, %d], or beyond %d with a mean or without the key buffer", k, k_max, SLS_NN_K_MAX);
        return SLS_E_ARG;
    }
    ScopedTimer tm(T_KNN, st);
    NnFront f;
    const int rc = nn_front(Mt, target_xyz, Mq, query_xyz, true, scratch, st, &f);
    if (rc) return rc;
    if (k <= SLS_NN_K_MAX) {
        nnk_launch<false>(Mt, Mq, f, k, out_dist2, out_index, out_mean, out_last_key, k, nullptr, st);
    } else {
        // two passes (see above): the 32 nearest and their last key, then the k - 32 nearest beyond that key
        nnk_launch<false>(Mt, Mq, f, SLS_NN_K_MAX, out_dist2, out_index, nullptr, out_last_key, k, nullptr, st);
        SLS_LAUNCH_CHECK("nn_query_k_kernel");
        nnk_launch<true>(Mt, Mq, f, k - SLS_NN_K_MAX, out_dist2 ? out_dist2 + SLS_NN_K_MAX : nullptr,
                         out_index ? out_index + SLS_NN_K_MAX : nullptr, nullptr, nullptr, k, out_last_key, st);
    }
    SLS_LAUNCH_CHECK("nn_query_k_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sls_nn_stats: count, count below the threshold and float64 sum of the distances (sls_nn_stats_term), in a FIXED order:
// block b of a grid that depends on M alone sums its entries b*256 + t, + grid*256, ... per thread, the 64 lanes by a
// butterfly, the 4 waves in order; one block then adds the partials the same way.  No atomics: the same bits every run.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kNnStatsMaxBlocks = SLS_NN_STATS_SCRATCH_BYTES / 32;     // 32 bytes per partial: n, n_below, sum, pad

struct NnPartial { unsigned long long n, below; double sum; };

__device__ __forceinline__ NnPartial nn_block_sum(NnPartial v)
{   // valid in thread 0
    __shared__ unsigned long long s_n[4], s_b[4];
    __shared__ double s_s[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v.n += __shfl_xor(v.n, off, 64);
        v.below += __shfl_xor(v.below, off, 64);
        v.sum += __shfl_xor(v.sum, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_n[threadIdx.x >> 6] = v.n; s_b[threadIdx.x >> 6] = v.below; s_s[threadIdx.x >> 6] = v.sum; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) { v.n += s_n[w]; v.below += s_b[w]; v.sum += s_s[w]; }
    return v;
}

__global__ __launch_bounds__(256) void nn_stats_partial_kernel(int M, const float *__restrict__ dist2, float truncation,
                                                               float threshold, int include_truncated,
                                                               unsigned long long *__restrict__ partials)
{
    NnPartial v = { 0ull, 0ull, 0.0 };
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)M; i += (size_t)gridDim.x * 256) {
        float d;
        if (sls_nn_stats_term(dist2[i], truncation, include_truncated, &d)) {
            v.n += 1ull;
            v.below += d < threshold ? 1ull : 0ull;
            v.sum += (double)d;
        }
    }
    v = nn_block_sum(v);
    if (threadIdx.x == 0) {
        partials[4 * blockIdx.x] = v.n;
        partials[4 * blockIdx.x + 1] = v.below;
        partials[4 * blockIdx.x + 2] = (unsigned long long)__double_as_longlong(v.sum);
    }
}

__global__ __launch_bounds__(256) void nn_stats_final_kernel(int M, int nblocks, const unsigned long long *__restrict__ partials,
                                                             unsigned long long *__restrict__ out)
{
    NnPartial v = { 0ull, 0ull, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        v.n += partials[4 * b];
        v.below += partials[4 * b + 1];
        v.sum += __longlong_as_double((long long)partials[4 * b + 2]);
    }
    v = nn_block_sum(v);
    if (threadIdx.x == 0) {
        out[0] = v.n;
        out[1] = v.below;
        out[2] = (unsigned long long)__double_as_longlong(v.sum);
        out[3] = (unsigned long long)M;
    }
}

int launch_nn_stats(int M, const float *dist2, float truncation, float threshold, int include_truncated, uint64_t *out_stats,
                    void *scratch, hipStream_t st)
{
    int nblocks = (M + 255) / 256;
    if (nblocks > kNnStatsMaxBlocks) nblocks = kNnStatsMaxBlocks;
    unsigned long long *partials = (unsigned long long *)scratch;
    if (nblocks > 0) {
        hipLaunchKernelGGL(nn_stats_partial_kernel, dim3(nblocks), dim3(256), 0, st, M, dist2, truncation, threshold,
                           include_truncated, partials);
        SLS_LAUNCH_CHECK("nn_stats_partial_kernel");
    }
    hipLaunchKernelGGL(nn_stats_final_kernel, dim3(1), dim3(256), 0, st, M, nblocks, partials,
                       (unsigned long long *)out_stats);
    SLS_LAUNCH_CHECK("nn_stats_final_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sls_mesh_distance: for every query point the nearest TRIANGLE of a mesh — the squared distance of
// include/sls_meshdist_math.h and the lowest face index attaining it.  The fourth user of the sweep: an index whose items
// are triangles (three float4: the vertices, the face index in a.w) in the curve order of their CENTROIDS, and whose boxes
// and sub-boxes bound ALL THREE vertices of their 256 / 32 triangles — the sweep prunes by "a gap never exceeds the
// distance to anything in the box", which a box over centroids would break.  A few huge triangles among many small ones
// make their runs' boxes loose: more runs are scanned, nothing is missed.  The codes live in the cube of the valid faces'
// vertices, so the queries' codes (knn_morton_kernel, nn_front_sorted_queries: unchanged) live there too.
// A face with a vertex index outside [0, V) or a non-finite vertex is counted in the status words and indexed as three
// points at the origin: nothing is read out of range, and the caller discards the outputs.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void tri_init_kernel(uint32_t *bbox, uint32_t *status, uint32_t F, uint32_t Mq, uint32_t word3)
{
    if (threadIdx.x < 3) bbox[threadIdx.x] = 0xFFFFFFFFu;
    else if (threadIdx.x < 6) bbox[threadIdx.x] = 0u;
    else if (threadIdx.x == 6) bbox[6] = F;
    else if (threadIdx.x == 7) bbox[7] = Mq;
    else if (threadIdx.x < 12) status[threadIdx.x - 8] = threadIdx.x == 8 ? F : (threadIdx.x == 11 ? word3 : 0u);
}

// the cube of the valid faces' vertices and the counts of the others (integer atomics: any order gives the same words)
__global__ __launch_bounds__(256) void tri_bbox_kernel(int V, const float *__restrict__ vertices, int F,
                                                       const int32_t *__restrict__ faces, uint32_t *bbox, uint32_t *status)
{
    float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    uint32_t n_index = 0, n_nonfinite = 0;
    for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) {
        float4 a, b, c;
        bool bad_index;
        if (!tri_load(V, vertices, faces, (size_t)f, a, b, c, &bad_index)) {
            if (bad_index) ++n_index; else ++n_nonfinite;
            continue;
        }
        mn[0] = fminf(mn[0], fminf(a.x, fminf(b.x, c.x))); mx[0] = fmaxf(mx[0], fmaxf(a.x, fmaxf(b.x, c.x)));
        mn[1] = fminf(mn[1], fminf(a.y, fminf(b.y, c.y))); mx[1] = fmaxf(mx[1], fmaxf(a.y, fmaxf(b.y, c.y)));
        mn[2] = fminf(mn[2], fminf(a.z, fminf(b.z, c.z))); mx[2] = fmaxf(mx[2], fmaxf(a.z, fmaxf(b.z, c.z)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
        }
        n_index += __shfl_xor(n_index, off, 64);
        n_nonfinite += __shfl_xor(n_nonfinite, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (mn[k] <= mx[k]) { atomicMin(&bbox[k], f2ord(mn[k])); atomicMax(&bbox[3 + k], f2ord(mx[k])); }
        }
        if (n_index) atomicAdd(&status[1], n_index);
        if (n_nonfinite) atomicAdd(&status[2], n_nonfinite);
    }
}

__global__ __launch_bounds__(256) void tri_code_kernel(int V, const float *__restrict__ vertices, int F,
                                                       const int32_t *__restrict__ faces, const uint32_t *__restrict__ bbox,
                                                       uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, int key_bits)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float4 a, b, c;
    bool bad_index;
    tri_load(V, vertices, faces, (size_t)f, a, b, c, &bad_index);
    const float third = 1.0f / 3.0f;
    keys[f] = curve_code(((a.x + b.x) + c.x) * third, ((a.y + b.y) + c.y) * third, ((a.z + b.z) + c.z) * third, bbox, key_bits);
    vals[f] = (uint32_t)f;
}

__global__ __launch_bounds__(256) void tri_gather_boxes_kernel(int V, const float *__restrict__ vertices, int F,
                                                               const int32_t *__restrict__ faces,
                                                               const uint32_t *__restrict__ sorted_idx,
                                                               TriItem *__restrict__ items, float4 *__restrict__ boxes,
                                                               float4 *__restrict__ subboxes)
{
    const int j = blockIdx.x * kKnnBox + threadIdx.x;
    float4 mn = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.0f), mx = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f);
    if (j < F) {
        const uint32_t f = sorted_idx[j];
        TriItem t;
        bool bad_index;
        tri_load(V, vertices, faces, (size_t)f, t.a, t.b, t.c, &bad_index);
        mn = make_float4(fminf(t.a.x, fminf(t.b.x, t.c.x)), fminf(t.a.y, fminf(t.b.y, t.c.y)), fminf(t.a.z, fminf(t.b.z, t.c.z)), 0.0f);
        mx = make_float4(fmaxf(t.a.x, fmaxf(t.b.x, t.c.x)), fmaxf(t.a.y, fmaxf(t.b.y, t.c.y)), fmaxf(t.a.z, fmaxf(t.b.z, t.c.z)), 0.0f);
        t.a.w = __uint_as_float(f);
        items[j] = t;
    }
    store_boxes(mn, mx, boxes, subboxes);
}

struct TriBestSearch {
    const float4 me;
    uint64_t best;
    __device__ __forceinline__ float bound() const { return sls_nn_key_dist2(best); }
    // a copy of the run's first triangle, as BestKeySearch pads: a sentinel at 1e30 would give inf - inf inside the arithmetic
    __device__ __forceinline__ TriItem pad(const TriItem *__restrict__ items, int r0) const { return items[r0]; }
    __device__ __forceinline__ void scan(const TriItem *s_run)
    {
#pragma unroll 2
        for (int k = 0; k < kKnnSub; ++k) {
            const float4 a = s_run[k].a, b = s_run[k].b, c = s_run[k].c;
            const float d2 = sls_meshdist_triangle(me.x, me.y, me.z, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, nullptr);
            const uint64_t key = sls_nn_key(d2, __float_as_uint(a.w));
            best = key < best ? key : best;
        }
    }
};

__global__ __launch_bounds__(64) void tri_query_kernel(int F, int nboxes, const TriItem *__restrict__ items,
                                                       const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                       const uint32_t *__restrict__ tkeys, int Mq,
                                                       const float4 *__restrict__ qpts, const uint32_t *__restrict__ qkeys, int V,
                                                       const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                       float *__restrict__ out_dist2, int32_t *__restrict__ out_face,
                                                       float *__restrict__ out_closest)
{
    __shared__ SweepLdsOf<TriItem> lds;
    const TriIndex ix = { F, nboxes, items, boxes, subboxes };
    const int q0 = blockIdx.x * 64, q = q0 + threadIdx.x;   // (the grid has ceil(Mq / 64) waves: q0 < Mq)
    const bool live = q < Mq;
    const float4 me = qpts[live ? q : Mq - 1];
    TriBestSearch s = { me, SLS_NN_KEY_NONE };
    nn_search(ix, tkeys, qkeys[q0], live, me, s, lds);
    if (live) {
        const size_t i = __float_as_uint(me.w);
        const uint32_t face = sls_nn_key_index(s.best);
        out_dist2[i] = sls_nn_key_dist2(s.best);
        if (out_face) out_face[i] = (int32_t)face;
        if (out_closest) {
            // the winner's closest point, recomputed once from (q, face); a query that met only NaN holds no face
            float cp[3] = { me.x, me.y, me.z };
            float4 a, b, c;
            bool bad_index;
            if (face < (uint32_t)F && tri_load(V, vertices, faces, (size_t)face, a, b, c, &bad_index))
                sls_meshdist_triangle(me.x, me.y, me.z, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, cp);
            out_closest[3 * i] = cp[0];
            out_closest[3 * i + 1] = cp[1];
            out_closest[3 * i + 2] = cp[2];
        }
    }
}

// scratch: sls_nn_query's for (F, Mq) — codes, sorter, boxes, the queries' buffers; its float4 per target stays unused —
// then the triangles
static NnScratch mesh_distance_layout(int F, int Mq, void *base, TriItem **items)
{
    NnScratch s = nn_layout(F, Mq, base);
    Arena a(base);
    a.off = (s.total + 255) & ~(size_t)255;
    *items = a.take<TriItem>((size_t)F);
    s.total = a.off;
    return s;
}

size_t mesh_distance_scratch_bytes(int V, int F, int Mq)
{
    TriItem *items;
    return (V >= 1 && F >= 1 && Mq >= 0) ? mesh_distance_layout(F, Mq, nullptr, &items).total : 0;
}

// The index of a mesh's triangles, for launch_mesh_distance and for launch_mesh_rayindex_build (sls_raycast.hip) alike: the
// status words [F, faces with a bad index, faces with a non-finite vertex, word3] and the cube of the valid faces; then,
// unless counts_only, the centroids' codes, the sort, the triangles in curve order and their boxes and sub-boxes.
// count2: the item count of a second sort that follows (bbox[7]).  *which: where the sorted (code, index) pairs ended up.
int tri_index_build(int V, const float *vertices, int F, const int32_t *faces, const TriIndexBuild &b, uint32_t count2,
                    uint32_t *out_status, uint32_t word3, bool counts_only, hipStream_t st, int *which)
{
    const int nb = (F + 255) / 256, key_bits = knn_key_bits(F), nboxes = (F + kKnnBox - 1) / kKnnBox;
    hipLaunchKernelGGL(tri_init_kernel, dim3(1), dim3(64), 0, st, b.bbox, out_status, (uint32_t)F, count2, word3);
    SLS_LAUNCH_CHECK("tri_init_kernel");
    hipLaunchKernelGGL(tri_bbox_kernel, dim3(nb < 256 ? nb : 256), dim3(256), 0, st, V, vertices, F, faces, b.bbox, out_status);
    SLS_LAUNCH_CHECK("tri_bbox_kernel");
    if (counts_only) return SLS_OK;
    hipLaunchKernelGGL(tri_code_kernel, dim3(nb), dim3(256), 0, st, V, vertices, F, faces, b.bbox, b.keys, b.vals, key_bits);
    SLS_LAUNCH_CHECK("tri_code_kernel");
    const int rc = radix_sort_pairs_u32(b.keys, b.vals, b.keys_tmp, b.vals_tmp, b.bbox + 6, (uint32_t)F, key_bits, b.sort, b.sort_bytes,
                                        which, st);
    if (rc) return rc;
    hipLaunchKernelGGL(tri_gather_boxes_kernel, dim3(nboxes), dim3(kKnnBox), 0, st, V, vertices, F, faces,
                       *which ? b.vals_tmp : b.vals, b.items, b.boxes, b.subboxes);
    SLS_LAUNCH_CHECK("tri_gather_boxes_kernel");
    return SLS_OK;
}

int launch_mesh_distance(int V, const float *vertices, int F, const int32_t *faces, int Mq, const float *query_xyz,
                         float *out_dist2, int32_t *out_face, float *out_closest, uint32_t *out_status, void *scratch,
                         hipStream_t st)
{
    ScopedTimer tm(T_KNN, st);
    NnFront f;
    TriItem *items;
    const NnScratch &s = f.s = mesh_distance_layout(F, Mq, scratch, &items);
    const int key_bits = knn_key_bits(F), nboxes = (F + kKnnBox - 1) / kKnnBox;
    TriIndexBuild b{};
    b.bbox = s.t.bbox; b.keys = s.t.keys; b.keys_tmp = s.t.keys_tmp; b.vals = s.t.vals; b.vals_tmp = s.t.vals_tmp;
    b.items = items; b.boxes = s.t.boxes; b.subboxes = s.t.subboxes; b.sort = s.t.sort; b.sort_bytes = s.t.sort_bytes;
    int which = 0;
    int rc = tri_index_build(V, vertices, F, faces, b, (uint32_t)Mq, out_status, 1u, Mq == 0, st, &which);
    if (rc || Mq == 0) return rc;                       // (Mq == 0: the status alone)
    f.tkeys = which ? s.t.keys_tmp : s.t.keys;
    hipLaunchKernelGGL(knn_morton_kernel, dim3((Mq + 255) / 256), dim3(256), 0, st, Mq, query_xyz, s.t.bbox, s.qkeys, s.qvals,
                       key_bits);
    SLS_LAUNCH_CHECK("knn_morton_kernel");
    rc = nn_front_sorted_queries(F, Mq, query_xyz, st, &f);
    if (rc) return rc;
    hipLaunchKernelGGL(tri_query_kernel, dim3((Mq + 63) / 64), dim3(64), 0, st, F, nboxes, items, s.t.boxes, s.t.subboxes, f.tkeys,
                       Mq, f.qpts, f.qkeys, V, vertices, faces, out_dist2, out_face, out_closest);
    SLS_LAUNCH_CHECK("tri_query_kernel");
    return SLS_OK;
}

__global__ __launch_bounds__(256) void error_colors_kernel(int M, const float *__restrict__ dist2, float truncation,
                                                           uint8_t *__restrict__ out_rgb)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M) return;
    uint8_t rgb[3];
    sls_error_color(dist2[i], truncation, rgb);
    out_rgb[3 * i] = rgb[0];
    out_rgb[3 * i + 1] = rgb[1];
    out_rgb[3 * i + 2] = rgb[2];
}

int launch_error_colors(int M, const float *dist2, float truncation, uint8_t *out_rgb, hipStream_t st)
{
    if (M == 0) return SLS_OK;
    hipLaunchKernelGGL(error_colors_kernel, dim3((M + 255) / 256), dim3(256), 0, st, M, dist2, truncation, out_rgb);
    SLS_LAUNCH_CHECK("error_colors_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sls_cloud_dbscan's three searches (include/sls_cluster_math.h; the stages between them live in sls_cluster.hip).  All
// three are the cloud's SELF-query at the constant radius r2 — the own box first, then the sweep, as knn_query_kernel
// does, but a point is its own neighbour: no lane leaves itself out.
//   count   CountSearch: the neighbours within r2, the bound r2 until the lane's count reaches min_points and after that
//           a value nothing passes, so a wave whose lanes are all core lists nothing more.  A count rests on the sweep
//           showing every target once; a saturated lane may be shown more for another lane's sake, which only raises a
//           count that is read as `>= min_points`.
//   unite   UniteSearch, core lanes alone: uf_unite(own index, target's index) for the core targets of LOWER index within
//           r2 — each pair joined once.  parent is indexed by ORIGINAL index, so a root is its component's lowest core.
//   border  BorderSearch, non-core lanes alone: the lowest root among the core targets within r2.
// The core flag rides in the staged item: cluster_mark_kernel, between count and unite, sets the top bit of pts[].w (an
// original index is below 2^31).  The pad of a short last run is a far point: d2 = +inf passes no radius.
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kClusterCoreBit = 0x80000000u;

__device__ __forceinline__ float4 cluster_pad() { return make_float4(1.0e30f, 1.0e30f, 1.0e30f, 0.0f); }

struct CountSearch {
    const float4 me;
    const float r2;
    const int min_points;
    int count;
    __device__ __forceinline__ float bound() const { return sls_cluster_count_bound(count, min_points, r2); }
    __device__ __forceinline__ float4 pad(const float4 *, int) const { return cluster_pad(); }
    __device__ __forceinline__ void scan(const float4 *s_run)
    {
#pragma unroll 8
        for (int k = 0; k < kKnnSub; ++k) {
            const float4 p = s_run[k];
            count += sls_cluster_near(sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z), r2);
        }
    }
};

struct UniteSearch {
    const float4 me;
    const float r2;
    const bool active;              // a core lane: the others are shown the runs and do nothing
    const uint32_t mine;            // the lane's original index
    uint32_t *parent;
    __device__ __forceinline__ float bound() const { return r2; }
    __device__ __forceinline__ float4 pad(const float4 *, int) const { return cluster_pad(); }
    __device__ __forceinline__ void scan(const float4 *s_run)
    {
        for (int k = 0; k < kKnnSub; ++k) {
            const float4 p = s_run[k];
            const uint32_t w = __float_as_uint(p.w);        // a core target of lower index: w - bit < mine
            if (active && sls_cluster_near(sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z), r2) && w >= kClusterCoreBit &&
                (w ^ kClusterCoreBit) < mine)
                uf_unite(parent, mine, w ^ kClusterCoreBit);
        }
    }
};

struct BorderSearch {
    const float4 me;
    const float r2;
    const bool active;
    const uint32_t *__restrict__ root;
    uint32_t best;
    __device__ __forceinline__ float bound() const { return r2; }
    __device__ __forceinline__ float4 pad(const float4 *, int) const { return cluster_pad(); }
    __device__ __forceinline__ void scan(const float4 *s_run)
    {
        for (int k = 0; k < kKnnSub; ++k) {
            const float4 p = s_run[k];
            const uint32_t w = __float_as_uint(p.w);
            if (active && sls_cluster_near(sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z), r2) && w >= kClusterCoreBit)
                best = min(best, root[w ^ kClusterCoreBit]);
        }
    }
};

// the body of the three kernels behind their set-up: the wave's own box in full, then the sweep over the others
template <class Search>
__device__ __forceinline__ void self_search(const KnnIndex &ix, const bool live, const float4 me, Search &s, SweepLds &lds)
{
    const int own_box = (blockIdx.x * 64) / kKnnBox, own_sub0 = (blockIdx.x * 64) / kKnnSub, nsub = ix.nsub();
    for (int t = 0; t < kKnnSubs; ++t) {
        const int sb = own_box * kKnnSubs + ((t + (own_sub0 % kKnnSubs)) % kKnnSubs);
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

// core[i] = 1 / 0 and parent[i] = i, both by original index
__global__ __launch_bounds__(64) void cluster_count_kernel(int M, int nboxes, const float4 *__restrict__ pts,
                                                           const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                           float r2, int min_points, uint32_t *__restrict__ core,
                                                           uint32_t *__restrict__ parent)
{
    __shared__ SweepLds lds;
    const KnnIndex ix = { M, nboxes, pts, boxes, subboxes };
    const int q = blockIdx.x * 64 + threadIdx.x;
    const bool live = q < M;
    const float4 me = pts[live ? q : M - 1];
    CountSearch s = { me, r2, min_points, 0 };
    self_search(ix, live, me, s, lds);
    if (live) {
        const uint32_t i = __float_as_uint(me.w);
        core[i] = (uint32_t)sls_cluster_core(s.count, min_points);
        parent[i] = i;
    }
}

__global__ __launch_bounds__(256) void cluster_mark_kernel(int M, float4 *__restrict__ pts, const uint32_t *__restrict__ core)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const uint32_t i = __float_as_uint(pts[j].w);
    if (core[i]) pts[j].w = __uint_as_float(i | kClusterCoreBit);
}

__global__ __launch_bounds__(64) void cluster_unite_kernel(int M, int nboxes, const float4 *__restrict__ pts,
                                                           const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                           float r2, uint32_t *parent)
{
    __shared__ SweepLds lds;
    const KnnIndex ix = { M, nboxes, pts, boxes, subboxes };
    const int q = blockIdx.x * 64 + threadIdx.x;
    const float4 me = pts[q < M ? q : M - 1];
    const bool live = q < M && __float_as_uint(me.w) >= kClusterCoreBit;
    if (!__ballot(live)) return;                        // a wave without a core point joins nothing
    UniteSearch s = { me, r2, live, __float_as_uint(me.w) & ~kClusterCoreBit, parent };
    self_search(ix, live, me, s, lds);
}

// root[i] of the non-core points: the lowest root among their core neighbours, SLS_CLUSTER_NONE without one (the cores'
// entries, written by the flatten pass before this launch, are only read)
__global__ __launch_bounds__(64) void cluster_border_kernel(int M, int nboxes, const float4 *__restrict__ pts,
                                                            const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                            float r2, uint32_t *root)
{
    __shared__ SweepLds lds;
    const KnnIndex ix = { M, nboxes, pts, boxes, subboxes };
    const int q = blockIdx.x * 64 + threadIdx.x;
    const float4 me = pts[q < M ? q : M - 1];
    const bool live = q < M && __float_as_uint(me.w) < kClusterCoreBit;
    if (!__ballot(live)) return;                        // a wave of core points has no border to find
    BorderSearch s = { me, r2, live, root, SLS_CLUSTER_NONE };
    self_search(ix, live, me, s, lds);
    if (live) root[__float_as_uint(me.w)] = s.best;
}

// The cloud's index in `scratch` (knn_scratch_bytes(M), 256-byte aligned), the count and the mark; then, after the
// caller's own stages, the other two searches over the same index.  core, parent, root: [M] words by original index.
int cluster_index_count(int M, const float *xyz, float r2, int min_points, uint32_t *core, uint32_t *parent, void *scratch,
                        hipStream_t st)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    int which = 0;
    const int rc = knn_build(M, xyz, s, knn_key_bits(M), 0u, st, &which);
    if (rc) return rc;
    hipLaunchKernelGGL(cluster_count_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, (M + kKnnBox - 1) / kKnnBox,
                       (const float4 *)s.pts, (const float4 *)s.boxes, (const float4 *)s.subboxes, r2, min_points, core, parent);
    SLS_LAUNCH_CHECK("cluster_count_kernel");
    hipLaunchKernelGGL(cluster_mark_kernel, dim3((M + 255) / 256), dim3(256), 0, st, M, s.pts, (const uint32_t *)core);
    SLS_LAUNCH_CHECK("cluster_mark_kernel");
    return SLS_OK;
}

int cluster_unite(int M, float r2, uint32_t *parent, void *scratch, hipStream_t st)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    hipLaunchKernelGGL(cluster_unite_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, (M + kKnnBox - 1) / kKnnBox,
                       (const float4 *)s.pts, (const float4 *)s.boxes, (const float4 *)s.subboxes, r2, parent);
    SLS_LAUNCH_CHECK("cluster_unite_kernel");
    return SLS_OK;
}

int cluster_border(int M, float r2, uint32_t *root, void *scratch, hipStream_t st)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    hipLaunchKernelGGL(cluster_border_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, (M + kKnnBox - 1) / kKnnBox,
                       (const float4 *)s.pts, (const float4 *)s.boxes, (const float4 *)s.subboxes, r2, root);
    SLS_LAUNCH_CHECK("cluster_border_kernel");
    return SLS_OK;
}

}  // namespace sls
