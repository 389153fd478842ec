// sls_cluster.hip — density clustering of a point cloud and the selection of its large clusters
// (include/sls_cluster_math.h states the rule):
//   sls_cloud_dbscan   DBSCAN over exact radius neighbours: labels, counts, status words;
//   sls_cloud_select   the K largest clusters and those above a floor kept — the rule of sls_mesh_filter — as an ordered
//                      compaction of the cloud, normals travelling along.
// One native call each, nothing read back inside it.  sls_cloud_dbscan:
//   1. the index of the cloud's self-query (knn_build, sls_knn.hip) and the COUNT search (cluster_index_count) -> core[i],
//      parent[i] = i;
//   2. the UNITE search over the core points (cluster_unite): the lock-free union-find of sls_unionfind.hpp, parent by
//      original index, so a root is its component's lowest core whatever the order of the threads;
//   3. cluster_flatten: root[i] of every core (a launch of its own: parent is only read), SLS_CLUSTER_NONE elsewhere, and
//      the chunks' root counts;
//   4. the BORDER search over the non-core points (cluster_border): root[i] = the lowest root among the core neighbours;
//   5. cluster_rootscan (the shared chunked scan) -> C; cluster_rank: the roots' numbers in ascending order of the root,
//      which is the lowest core index; cluster_label: labels, counts and the three tallies by integer atomics — sums of
//      integers, the same words on every run; cluster_status: the largest count and the status words.
// Every loop is bounded by the box count or is the lock-free retry of uf_unite; nothing waits on another workgroup.
// Steps 3 and 5 number the components as sls_mesh.hip numbers its clusters of triangles, and sls_cloud_select keeps the
// largest as sls_mesh_filter does: uf_root and uf_kth_largest (sls_unionfind.hpp) serve both.  The compaction's rows are
// written by Chunks::write_rows (sls_scan.hpp), as sls_outlier.hip's.
#include "sls_sweep.hpp"
#include "sls_unionfind.hpp"
#include "../../include/sls_nn_math.h"
#include "../../include/sls_cluster_math.h"

namespace sls {

constexpr int kCluThreads = 256;
using CluChunks = Chunks<kCluThreads, 4>;
enum { CH_CORES = 0, CH_BORDERS = 1, CH_NOISE = 2, CH_NMIN = 3, CH_WORDS = 4 };

// ---------------------------------------------------------------------------------------------------------------------
// The three searches (the stages between them follow).  All three are the cloud's SELF-query at the constant radius r2 —
// the own box first, then the sweep (self_search, sls_sweep.hpp), as knn_query_kernel does, but a point is its own
// neighbour: no lane leaves itself out.
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
        for (int k = 0; k < kSweepSub; ++k) {
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
        for (int k = 0; k < kSweepSub; ++k) {
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
        for (int k = 0; k < kSweepSub; ++k) {
            const float4 p = s_run[k];
            const uint32_t w = __float_as_uint(p.w);
            if (active && sls_cluster_near(sls_nn_dist2(me.x, me.y, me.z, p.x, p.y, p.z), r2) && w >= kClusterCoreBit)
                best = min(best, root[w ^ kClusterCoreBit]);
        }
    }
};

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
static int cluster_index_count(int M, const float *xyz, float r2, int min_points, uint32_t *core, uint32_t *parent, void *scratch,
                               hipStream_t st)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    int which = 0;
    const int rc = knn_build(M, xyz, s, knn_key_bits(M), 0u, st, &which);
    if (rc) return rc;
    hipLaunchKernelGGL(cluster_count_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, (M + kSweepBox - 1) / kSweepBox,
                       (const float4 *)s.pts, (const float4 *)s.boxes, (const float4 *)s.subboxes, r2, min_points, core, parent);
    SLS_LAUNCH_CHECK("cluster_count_kernel");
    hipLaunchKernelGGL(cluster_mark_kernel, dim3((M + 255) / 256), dim3(256), 0, st, M, s.pts, (const uint32_t *)core);
    SLS_LAUNCH_CHECK("cluster_mark_kernel");
    return SLS_OK;
}

static int cluster_unite(int M, float r2, uint32_t *parent, void *scratch, hipStream_t st)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    hipLaunchKernelGGL(cluster_unite_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, (M + kSweepBox - 1) / kSweepBox,
                       (const float4 *)s.pts, (const float4 *)s.boxes, (const float4 *)s.subboxes, r2, parent);
    SLS_LAUNCH_CHECK("cluster_unite_kernel");
    return SLS_OK;
}

static int cluster_border(int M, float r2, uint32_t *root, void *scratch, hipStream_t st)
{
    const KnnScratch s = knn_layout(M, scratch, M);
    hipLaunchKernelGGL(cluster_border_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, (M + kSweepBox - 1) / kSweepBox,
                       (const float4 *)s.pts, (const float4 *)s.boxes, (const float4 *)s.subboxes, r2, root);
    SLS_LAUNCH_CHECK("cluster_border_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the stages between the searches
// ---------------------------------------------------------------------------------------------------------------------

__global__ void cluster_status0_kernel(uint32_t *status, int words, uint32_t n_min)
{
    if ((int)threadIdx.x < words) status[threadIdx.x] = (int)threadIdx.x == words - 1 ? 1u : 0u;
    if (words == SLS_CLUSTER_SELECT_STATUS_WORDS && threadIdx.x == 1) status[1] = n_min;
}

__global__ __launch_bounds__(kCluThreads) void cluster_flatten_kernel(uint32_t M, const uint32_t *__restrict__ core,
                                                                      const uint32_t *__restrict__ parent,
                                                                      uint32_t *__restrict__ root, uint32_t *__restrict__ blk,
                                                                      uint32_t *__restrict__ hdr)
{
    const uint32_t i0 = CluChunks::first();
    uint32_t nroots = 0u;
#pragma unroll
    for (int j = 0; j < CluChunks::kPer; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        if (i < M) {
            uint32_t x = SLS_CLUSTER_NONE;
            if (core[i]) {
                x = uf_root(parent, parent[i]);
                nroots += x == i ? 1u : 0u;
            }
            root[i] = x;
        }
    }
    CluChunks::total(nroots, blk);
    if (blockIdx.x == 0 && threadIdx.x < CH_WORDS) hdr[threadIdx.x] = 0u;       // the tallies of cluster_label_kernel
}

__global__ __launch_bounds__(kCluThreads) void cluster_rootscan_kernel(int nblk, uint32_t *blk, uint32_t *__restrict__ status)
{
    const uint32_t C = CluChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) status[0] = C;
}

// dense[i] = the rank of root i among the roots; its count starts at 0
__global__ __launch_bounds__(kCluThreads) void cluster_rank_kernel(uint32_t M, const uint32_t *__restrict__ core,
                                                                   const uint32_t *__restrict__ root,
                                                                   const uint32_t *__restrict__ blk, uint32_t *__restrict__ dense,
                                                                   int32_t *__restrict__ counts)
{
    const uint32_t i0 = CluChunks::first();
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < CluChunks::kPer; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        if (i < M && core[i] && root[i] == i) mask |= 1u << j;
    }
    uint32_t id = CluChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < CluChunks::kPer; ++j)
        if ((mask >> j) & 1u) {                     // (id < M: there are at most M roots, and counts holds M entries)
            dense[i0 + (uint32_t)j] = id;
            counts[id] = 0;
            ++id;
        }
}

__global__ __launch_bounds__(kCluThreads) void cluster_label_kernel(uint32_t M, const uint32_t *__restrict__ core,
                                                                    const uint32_t *__restrict__ root,
                                                                    const uint32_t *__restrict__ dense, int32_t *__restrict__ labels,
                                                                    int32_t *counts, uint32_t *hdr)
{
    const size_t i = (size_t)blockIdx.x * kCluThreads + threadIdx.x;
    bool is_core = false, is_border = false, is_noise = false;
    int32_t c = -1;
    if (i < M) {
        const uint32_t r = root[i];
        is_core = core[i] != 0u;
        is_border = !is_core && r != SLS_CLUSTER_NONE;
        is_noise = r == SLS_CLUSTER_NONE;
        if (!is_noise) c = (int32_t)dense[r];
        labels[i] = c;
    }
    // one atomic per distinct label of the wave, not per point: a cloud is mostly ONE cluster, and atomics on one address
    // serialise (a point each: 21 ms of a 30 ms call at 2 M points)
    uint64_t todo = __ballot(c >= 0);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int32_t lc = __builtin_amdgcn_readlane(c, leader);
        const uint64_t same = __ballot(c == lc);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&counts[lc], (int32_t)__popcll(same));
        todo &= ~same;
    }
    const uint64_t mc = __ballot(is_core), mb = __ballot(is_border), mn = __ballot(is_noise);
    if ((threadIdx.x & 63) == 0) {
        if (mc) atomicAdd(&hdr[CH_CORES], (uint32_t)__popcll(mc));
        if (mb) atomicAdd(&hdr[CH_BORDERS], (uint32_t)__popcll(mb));
        if (mn) atomicAdd(&hdr[CH_NOISE], (uint32_t)__popcll(mn));
    }
}

// one workgroup: the largest count, and the status words behind C
__global__ __launch_bounds__(kCluThreads) void cluster_status_kernel(uint32_t M, const int32_t *__restrict__ counts,
                                                                     const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    __shared__ uint32_t s_max[kCluThreads / 64];
    const uint32_t C = min(status[0], M);
    uint32_t mx = 0u;
    for (uint32_t c = threadIdx.x; c < C; c += kCluThreads) mx = max(mx, (uint32_t)counts[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kCluThreads / 64; ++w) mx = max(mx, s_max[w]);
        status[1] = hdr[CH_CORES]; status[2] = hdr[CH_BORDERS]; status[3] = hdr[CH_NOISE]; status[4] = mx; status[5] = M;
        status[6] = 0u; status[7] = 1u;
    }
}

struct DbscanScratch {
    void *index;
    uint32_t *core, *parent, *root, *dense, *blk, *hdr;
    size_t total;
    int nblk;
};

static DbscanScratch dbscan_layout(int M, void *base)
{
    DbscanScratch s;
    Arena a(base);
    s.nblk = CluChunks::count((size_t)M);
    s.index = a.take<char>(knn_scratch_bytes(M));
    s.core = a.take<uint32_t>((size_t)M);
    s.parent = a.take<uint32_t>((size_t)M);
    s.root = a.take<uint32_t>((size_t)M);
    s.dense = a.take<uint32_t>((size_t)M);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.hdr = a.take<uint32_t>(CH_WORDS);
    s.total = a.off;
    return s;
}

size_t cloud_dbscan_scratch_bytes(int M) { return M > 0 ? dbscan_layout(M, nullptr).total : 0; }

int launch_cloud_dbscan(int M, const float *xyz, float eps, int min_points, int32_t *out_labels, int32_t *out_counts,
                        uint32_t *out_status, void *scratch, hipStream_t st)
{
    if (M == 0) {
        hipLaunchKernelGGL(cluster_status0_kernel, dim3(1), dim3(64), 0, st, out_status, SLS_CLUSTER_STATUS_WORDS, 0u);
        SLS_LAUNCH_CHECK("cluster_status0_kernel");
        return SLS_OK;
    }
    const DbscanScratch s = dbscan_layout(M, scratch);
    const float r2 = sls_cluster_r2(eps);
    int rc = cluster_index_count(M, xyz, r2, min_points, s.core, s.parent, s.index, st);
    if (rc) return rc;
    rc = cluster_unite(M, r2, s.parent, s.index, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(s.nblk), dim3(kCluThreads), 0, st, (uint32_t)M, (const uint32_t *)s.core,
                       (const uint32_t *)s.parent, s.root, s.blk, s.hdr);
    SLS_LAUNCH_CHECK("cluster_flatten_kernel");
    rc = cluster_border(M, r2, s.root, s.index, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cluster_rootscan_kernel, dim3(1), dim3(kCluThreads), 0, st, s.nblk, s.blk, out_status);
    SLS_LAUNCH_CHECK("cluster_rootscan_kernel");
    hipLaunchKernelGGL(cluster_rank_kernel, dim3(s.nblk), dim3(kCluThreads), 0, st, (uint32_t)M, (const uint32_t *)s.core,
                       (const uint32_t *)s.root, (const uint32_t *)s.blk, s.dense, out_counts);
    SLS_LAUNCH_CHECK("cluster_rank_kernel");
    hipLaunchKernelGGL(cluster_label_kernel, grid_for((size_t)M, kCluThreads), dim3(kCluThreads), 0, st, (uint32_t)M,
                       (const uint32_t *)s.core, (const uint32_t *)s.root, (const uint32_t *)s.dense, out_labels, out_counts, s.hdr);
    SLS_LAUNCH_CHECK("cluster_label_kernel");
    hipLaunchKernelGGL(cluster_status_kernel, dim3(1), dim3(kCluThreads), 0, st, (uint32_t)M, (const int32_t *)out_counts,
                       (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("cluster_status_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// selection and compaction
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup: n_min from the k-th largest of the C counts (uf_kth_largest)
__global__ __launch_bounds__(kCluThreads) void cluster_nmin_kernel(uint32_t M, const uint32_t *__restrict__ cluster_status,
                                                                   const int32_t *__restrict__ counts, int keep,
                                                                   int min_cluster_points, uint32_t *__restrict__ hdr)
{
    const uint32_t C = min(cluster_status[0], M);
    const uint32_t lo = uf_kth_largest<CluChunks>(M, C, sls_cluster_keep_rank(keep, C), counts);
    if (threadIdx.x == 0) hdr[CH_NMIN] = sls_cluster_n_min(min_cluster_points, lo);
}

// the kept flags of this thread's four consecutive points, as a bit mask
__device__ __forceinline__ uint32_t cluster_kept_mask(uint32_t M, uint32_t C, uint32_t n_min, const int32_t *__restrict__ labels,
                                                      const int32_t *__restrict__ counts, uint32_t i0)
{
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < CluChunks::kPer; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        if (i < M && sls_cluster_keep(labels[i], counts, C, n_min)) mask |= 1u << j;
    }
    return mask;
}

__global__ __launch_bounds__(kCluThreads) void cluster_keep_count_kernel(uint32_t M, const uint32_t *__restrict__ cluster_status,
                                                                         const uint32_t *__restrict__ hdr,
                                                                         const int32_t *__restrict__ labels,
                                                                         const int32_t *__restrict__ counts, uint32_t *__restrict__ blk)
{
    const uint32_t C = min(cluster_status[0], M);
    CluChunks::total((uint32_t)__popc(cluster_kept_mask(M, C, hdr[CH_NMIN], labels, counts, CluChunks::first())), blk);
}

__global__ __launch_bounds__(kCluThreads) void cluster_keep_scan_kernel(uint32_t M, int nblk, uint32_t *blk,
                                                                        const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    const uint32_t kept = CluChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) { status[0] = kept; status[1] = hdr[CH_NMIN]; status[2] = M; status[3] = 1u; }
}

__global__ __launch_bounds__(kCluThreads) void cluster_keep_write_kernel(uint32_t M, const uint32_t *__restrict__ cluster_status,
                                                                         const uint32_t *__restrict__ hdr,
                                                                         const int32_t *__restrict__ labels,
                                                                         const int32_t *__restrict__ counts,
                                                                         const uint32_t *__restrict__ blk, const float *__restrict__ xyz,
                                                                         const float *__restrict__ normals, float *__restrict__ out_xyz,
                                                                         float *__restrict__ out_normals, int32_t *__restrict__ out_index)
{
    const uint32_t C = min(cluster_status[0], M);
    CluChunks::write_rows(cluster_kept_mask(M, C, hdr[CH_NMIN], labels, counts, CluChunks::first()), blk, xyz, normals, out_xyz,
                          out_normals, out_index);
}

struct SelectScratch {
    uint32_t *hdr, *blk;
    size_t total;
    int nblk;
};

static SelectScratch select_layout(int M, void *base)
{
    SelectScratch s;
    Arena a(base);
    s.nblk = CluChunks::count((size_t)M);
    s.hdr = a.take<uint32_t>(CH_WORDS);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.total = a.off;
    return s;
}

size_t cloud_select_scratch_bytes(int M) { return M > 0 ? select_layout(M, nullptr).total : 0; }

int launch_cloud_select(int M, const float *xyz, const float *normals, const int32_t *labels, const int32_t *counts,
                        const uint32_t *cluster_status, int keep, int min_cluster_points, float *out_xyz, float *out_normals,
                        int32_t *out_index, uint32_t *out_status, void *scratch, hipStream_t st)
{
    if (M == 0) {
        hipLaunchKernelGGL(cluster_status0_kernel, dim3(1), dim3(64), 0, st, out_status, SLS_CLUSTER_SELECT_STATUS_WORDS,
                           sls_cluster_n_min(min_cluster_points, 0u));
        SLS_LAUNCH_CHECK("cluster_status0_kernel");
        return SLS_OK;
    }
    const SelectScratch s = select_layout(M, scratch);
    hipLaunchKernelGGL(cluster_nmin_kernel, dim3(1), dim3(kCluThreads), 0, st, (uint32_t)M, cluster_status, counts, keep,
                       min_cluster_points, s.hdr);
    SLS_LAUNCH_CHECK("cluster_nmin_kernel");
    hipLaunchKernelGGL(cluster_keep_count_kernel, dim3(s.nblk), dim3(kCluThreads), 0, st, (uint32_t)M, cluster_status,
                       (const uint32_t *)s.hdr, labels, counts, s.blk);
    SLS_LAUNCH_CHECK("cluster_keep_count_kernel");
    hipLaunchKernelGGL(cluster_keep_scan_kernel, dim3(1), dim3(kCluThreads), 0, st, (uint32_t)M, s.nblk, s.blk,
                       (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("cluster_keep_scan_kernel");
    if (out_xyz || out_normals || out_index) {
        hipLaunchKernelGGL(cluster_keep_write_kernel, dim3(s.nblk), dim3(kCluThreads), 0, st, (uint32_t)M, cluster_status,
                           (const uint32_t *)s.hdr, labels, counts, (const uint32_t *)s.blk, xyz, normals, out_xyz, out_normals,
                           out_index);
        SLS_LAUNCH_CHECK("cluster_keep_write_kernel");
    }
    return SLS_OK;
}

}  // namespace sls
