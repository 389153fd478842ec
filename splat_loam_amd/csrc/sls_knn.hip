// sls_knn.hip — the index of a point cloud and the three searches among points.  It began as simple-knn's distCUDA2 for
// MI355X: out[i] = mean of the squared distances from point i to its 3 nearest other points
// (slam/mapper.py:113-115, scene/gaussian_model.py:77-81).
//
// Exact, built for LiDAR-like (very non-uniform) clouds:
//   1. bounding cube, 30-bit Hilbert-curve index per point;
//   2. wave64 LSD radix sort of (code, index) — the sorter of sls_radix.hip;
//   3. points gathered in curve order (float4: xyz + original index) and
//      axis-aligned boxes over runs of 256 consecutive points;
//   4. one wave per 64 consecutive points, one lane per point: the own box first for a tight bound, then the sweep
//      (knn_sweep, sls_sweep.hpp) over the other boxes; the two-cloud searches (sls_nn_query, sls_nn_query_k) run it too.
// The index front (knn_layout, knn_build, nn_layout, nn_query_codes, nn_front_sorted_queries: declared in sls_launch.hpp)
// also serves the point-to-mesh distance (sls_meshdist.hip) and the clustering (sls_cluster.hip).
// Squared distances use the fixed expression fma(dz,dz,fma(dy,dy,dx*dx)), so
// the result is reproducible bit for bit by a CPU brute force.
#include <float.h>

#include "sls_sweep.hpp"
#include "../../include/sls_nn_math.h"
#include "../../include/sls_outlier_math.h"

namespace sls {

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

__global__ __launch_bounds__(256) void knn_gather_boxes_kernel(int M, const float *__restrict__ xyz,
                                                               const uint32_t *__restrict__ sorted_idx,
                                                               float4 *__restrict__ pts, float4 *__restrict__ boxes,
                                                               float4 *__restrict__ subboxes)
{
    const int j = blockIdx.x * kSweepBox + threadIdx.x;
    float4 mn = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.0f), mx = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f);
    if (j < M) {
        const uint32_t i = sorted_idx[j];
        mn = mx = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
        pts[j] = make_float4(mn.x, mn.y, mn.z, __uint_as_float(i));
    }
    store_boxes(mn, mx, boxes, subboxes);
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
        for (int k = 0; k < kSweepSub; ++k) {
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
    const int own_box = (blockIdx.x * 64) / kSweepBox, own_sub0 = (blockIdx.x * 64) / kSweepSub;   // my runs: own_sub0, +1
    const int nsub = ix.nsub();
    Best3Search s = { me, FLT_MAX, FLT_MAX, FLT_MAX };

    // the own box for a first bound: my two runs, then the other six; every lane leaves itself out
    for (int t = 0; t < kSweepSubs; ++t) {
        const int sb = own_box * kSweepSubs + ((t + (own_sub0 % kSweepSubs)) % kSweepSubs);
        if (sb >= nsub) continue;
        stage(lds, run_point<true>(ix, sb, s));
        s.scan<true>(lds.run, (live && (q / kSweepSub) == sb) ? (q % kSweepSub) : -1);
    }

    // the wave's bounding box is that of its two runs (dead and non-query lanes included), the groups' are of live lanes
    float4 wmn = subboxes[2 * (size_t)own_sub0], wmx = subboxes[2 * (size_t)own_sub0 + 1];
    if (own_sub0 + 1 < nsub) box_join(wmn, wmx, subboxes[2 * (size_t)own_sub0 + 2], subboxes[2 * (size_t)own_sub0 + 3]);
    float4 gmn, gmx;
    group_boxes(live, me, gmn, gmx);
    knn_sweep(ix, own_box, live, me, wmn, wmx, gmn, gmx, s, lds);
    if (live) out[__float_as_uint(me.w)] = (s.b0 + s.b1 + s.b2) / 3.0f;
}

KnnScratch knn_layout(int M, void *base, int sort_items)
{
    const size_t nboxes = (size_t)((M + kSweepBox - 1) / kSweepBox);
    Arena a(base);
    KnnScratch s;
    s.bbox = a.take<uint32_t>(8);
    s.keys = a.take<uint32_t>((size_t)M);
    s.keys_tmp = a.take<uint32_t>((size_t)M);
    s.vals = a.take<uint32_t>((size_t)M);
    s.vals_tmp = a.take<uint32_t>((size_t)M);
    s.pts = a.take<float4>((size_t)M);
    s.boxes = a.take<float4>(2 * nboxes);
    s.subboxes = a.take<float4>(2 * nboxes * kSweepSubs);
    s.sort_bytes = sort_scratch_bytes((uint64_t)sort_items);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t knn_scratch_bytes(int M) { return M > 0 ? knn_layout(M, nullptr, M).total : 0; }

// The front half of every search (see sls_launch.hpp)
int knn_build(int M, const float *xyz, const KnnScratch &s, int key_bits, uint32_t M2, hipStream_t st, int *which)
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
    const int nboxes = (M + kSweepBox - 1) / kSweepBox;
    hipLaunchKernelGGL(knn_gather_boxes_kernel, dim3(nboxes), dim3(kSweepBox), 0, st, M, xyz,
                       *which ? s.vals_tmp : s.vals, s.pts, s.boxes, s.subboxes);
    SLS_LAUNCH_CHECK("knn_gather_boxes_kernel");
    return SLS_OK;
}

// small clouds are sorted on 21 code bits (knn_morton_kernel)
int knn_key_bits(int M) { return M <= 200000 ? 21 : 30; }

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
    const int nboxes = (M + kSweepBox - 1) / kSweepBox;
    static_assert(kSweepBox == 256 && kSweepSub == 32, "the query kernel's lane mappings are written for 8 runs of 32");
    hipLaunchKernelGGL(knn_query_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, nboxes, s.pts, s.boxes, s.subboxes, out,
                       (uint32_t)(Mq < 0 || Mq > M ? M : Mq));
    SLS_LAUNCH_CHECK("knn_query_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sls_nn_query: for every point of a SECOND cloud the nearest point of the indexed one — squared distance and the lowest
// original index attaining it (include/sls_nn_math.h).  The queries are sorted along the target's curve (nn_front below)
// and searched by nn_search (sls_sweep.hpp); the search is ONE packed key (bits(d2) << 32 | index), minimised, so the
// lowest index among equally near targets wins.
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
        for (int k = 0; k < kSweepSub; ++k) {
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

NnScratch nn_layout(int Mt, int Mq, void *base)
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

// What both two-cloud launchers do before their query kernel (NnFront): the target's index, then the queries' codes in the
// TARGET's cube (knn_morton_kernel clamps to the border cells outside), the same sorter and the gather in curve order.
// self_ok: a cloud queried by itself is its own sorted query set, and the second code / sort / gather is skipped.

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

int nn_query_codes(int Mq, const float *query_xyz, const uint32_t *bbox, uint32_t *qkeys, uint32_t *qvals, int key_bits, hipStream_t st)
{
    hipLaunchKernelGGL(knn_morton_kernel, dim3((Mq + 255) / 256), dim3(256), 0, st, Mq, query_xyz, bbox, qkeys, qvals, key_bits);
    SLS_LAUNCH_CHECK("knn_morton_kernel");
    return SLS_OK;
}

// the query half behind codes that are already in s.qkeys / s.qvals: the sort and the gather in curve order
int nn_front_sorted_queries(int Mt, int Mq, const float *query_xyz, hipStream_t st, NnFront *f)
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
    rc = nn_query_codes(Mq, query_xyz, f->s.t.bbox, f->s.qkeys, f->s.qvals, knn_key_bits(Mt), st);
    if (rc) return rc;
    return nn_front_sorted_queries(Mt, Mq, query_xyz, st, f);
}

static int nn_query_launch(int Mt, int Mq, const NnFront &f, float *out_dist2, int32_t *out_index, hipStream_t st)
{
    hipLaunchKernelGGL(nn_query_kernel, dim3((Mq + 63) / 64), dim3(64), 0, st, Mt, (Mt + kSweepBox - 1) / kSweepBox, f.s.t.pts,
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
        for (int j = 0; j < kSweepSub; ++j) {
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
        hipLaunchKernelGGL(kernel, dim3((Mq + 63) / 64), dim3(64), 0, st, Mt, (Mt + kSweepBox - 1) / kSweepBox, f.s.t.pts, f.s.t.boxes,
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

}  // namespace sls
