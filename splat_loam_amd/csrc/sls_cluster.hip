// sls_cluster.hip — density clustering of a point cloud and the selection of its large clusters
// (include/sls_cluster_math.h states the rule):
//   sls_cloud_dbscan   DBSCAN over exact radius neighbours: labels, counts, status words;
//   sls_cloud_select   the K largest clusters and those above a floor kept — the rule of sls_mesh_filter — as an ordered
//                      compaction of the cloud, normals travelling along.
// One native call each, nothing read back inside it.  sls_cloud_dbscan:
//   1. the index of the cloud's self-query and the COUNT search (sls_knn.hip: cluster_index_count) -> core[i], parent[i] = i;
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
#include "sls_launch.hpp"
#include "sls_unionfind.hpp"
#include "../../include/sls_cluster_math.h"

namespace sls {

constexpr int kCluThreads = 256;
using CluChunks = Chunks<kCluThreads, 4>;
enum { CH_CORES = 0, CH_BORDERS = 1, CH_NOISE = 2, CH_NMIN = 3, CH_WORDS = 4 };

// (in sls_knn.hip: the searches share the sweep)
int cluster_index_count(int M, const float *xyz, float r2, int min_points, uint32_t *core, uint32_t *parent, void *scratch,
                        hipStream_t st);
int cluster_unite(int M, float r2, uint32_t *parent, void *scratch, hipStream_t st);
int cluster_border(int M, float r2, uint32_t *root, void *scratch, hipStream_t st);

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
