// sls_outlier.hip — the two outlier filters of a point cloud (include/sls_outlier_math.h states the rules):
//   sls_outlier_statistical   Open3D's remove_statistical_outlier, restated: the mean distance to the k nearest (the
//                             point itself included) against cloud_mean + std_ratio * std of those means;
//   sls_outlier_radius        more than nb_points points within the radius.
// One native call each, nothing read back inside it:
//   1. the self-query (sls_knn.hip: launch_nn_query_k) — the means only, or only the key at rank nb_points: 8 bytes a point;
//   2. statistical: two float64 reductions in the fixed order of sls_nn_stats (block b of a grid that depends on M alone
//      sums its entries b * 256 + t, + grid * 256, ... per thread, the 64 lanes by a butterfly, the 4 waves in order, one
//      workgroup then adds the partials the same way; no float atomics) — first the zero count and the sum, then the
//      squared deviations — and the threshold, all on the device;
//   3. an ordered compaction through Chunks (sls_scan.hpp): the keep flags are recomputed from the 8 bytes where they are
//      needed; write_rows, shared with sls_cluster.hip: kept rows in ascending original index, normals with their points.
#include "sls_launch.hpp"
#include "sls_scan.hpp"
#include "../../include/sls_outlier_math.h"

namespace sls {

constexpr int kOutThreads = 256;
constexpr int kOutMaxBlocks = 1024;                 // partials of the reductions: 16 bytes each
using OutChunks = Chunks<kOutThreads, 4>;
enum { OH_CLOUD_MEAN = 0, OH_THR = 1, OH_WORDS = 4 };                                  // the header's doubles
enum { OS_KEPT = 0, OS_ZERO = 1, OS_CLOUD_MEAN = 2, OS_STD = 3, OS_THR = 4, OS_M = 5 };   // out_status (sls_abi.h)

struct OutPartial { unsigned long long n; double sum; };

__device__ __forceinline__ OutPartial out_block_sum(OutPartial v)
{   // valid in thread 0
    __shared__ unsigned long long s_n[kOutThreads / 64];
    __shared__ double s_s[kOutThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v.n += __shfl_xor(v.n, off, 64);
        v.sum += __shfl_xor(v.sum, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_n[threadIdx.x >> 6] = v.n; s_s[threadIdx.x >> 6] = v.sum; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kOutThreads / 64; ++w) { v.n += s_n[w]; v.sum += s_s[w]; }
    return v;
}

// PASS 0: n = the means that do not count (zero: every neighbour a copy), sum = the sum of those that do;
// PASS 1: sum = the squared deviations of the counted means from hdr[OH_CLOUD_MEAN]
template <int PASS>
__global__ __launch_bounds__(kOutThreads) void outlier_partial_kernel(int M, const double *__restrict__ means,
                                                                      const double *__restrict__ hdr,
                                                                      unsigned long long *__restrict__ partials)
{
    OutPartial v = { 0ull, 0.0 };
    const double cloud_mean = PASS ? hdr[OH_CLOUD_MEAN] : 0.0;
    for (size_t i = (size_t)blockIdx.x * kOutThreads + threadIdx.x; i < (size_t)M; i += (size_t)gridDim.x * kOutThreads) {
        const double m = means[i];
        if (sls_outlier_counts(m)) v.sum += PASS ? sls_outlier_dev2(m, cloud_mean) : m;
        else v.n += 1ull;
    }
    v = out_block_sum(v);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = v.n;
        partials[2 * blockIdx.x + 1] = (unsigned long long)__double_as_longlong(v.sum);
    }
}

template <int PASS>
__global__ __launch_bounds__(kOutThreads) void outlier_final_kernel(int M, int nblocks, const unsigned long long *__restrict__ partials,
                                                                    double std_ratio, double *__restrict__ hdr,
                                                                    unsigned long long *__restrict__ status)
{
    OutPartial v = { 0ull, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += kOutThreads) {
        v.n += partials[2 * b];
        v.sum += __longlong_as_double((long long)partials[2 * b + 1]);
    }
    v = out_block_sum(v);
    if (threadIdx.x != 0) return;
    if (PASS == 0) {
        const double cloud_mean = sls_outlier_cloud_mean(v.sum, M);
        hdr[OH_CLOUD_MEAN] = cloud_mean;
        status[OS_ZERO] = v.n;
        status[OS_CLOUD_MEAN] = (unsigned long long)__double_as_longlong(cloud_mean);
        status[OS_M] = (unsigned long long)M;
        status[6] = 0ull; status[7] = 0ull;
    } else {
        const double cloud_mean = hdr[OH_CLOUD_MEAN];
        const double std = sls_outlier_std(v.sum, M);
        const double thr = sls_outlier_threshold(cloud_mean, std, std_ratio);
        hdr[OH_THR] = thr;
        status[OS_STD] = (unsigned long long)__double_as_longlong(std);
        status[OS_THR] = (unsigned long long)__double_as_longlong(thr);
    }
}

// the keep flags of this thread's four consecutive points, as a bit mask.  vals: the means (statistical) or the rank
// keys (RADIUS), 8 bytes a point
template <bool RADIUS>
__device__ __forceinline__ uint32_t outlier_keep_mask(uint32_t M, const uint64_t *__restrict__ vals, const double *__restrict__ hdr,
                                                      float radius, uint32_t i0)
{
    const double thr = RADIUS ? 0.0 : hdr[OH_THR];
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < OutChunks::kPer; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        if (i < M) {
            const uint64_t v = vals[i];
            const bool keep = RADIUS ? sls_outlier_keep_radius(v, radius) != 0
                                     : sls_outlier_keep_statistical(__longlong_as_double((long long)v), thr) != 0;
            if (keep) mask |= 1u << j;
        }
    }
    return mask;
}

template <bool RADIUS>
__global__ __launch_bounds__(kOutThreads) void outlier_count_kernel(uint32_t M, const uint64_t *__restrict__ vals,
                                                                    const double *__restrict__ hdr, float radius,
                                                                    uint32_t *__restrict__ blk)
{
    OutChunks::total((uint32_t)__popc(outlier_keep_mask<RADIUS>(M, vals, hdr, radius, OutChunks::first())), blk);
}

template <bool RADIUS>
__global__ __launch_bounds__(kOutThreads) void outlier_scan_kernel(uint32_t M, int nblk, uint32_t *blk,
                                                                   unsigned long long *__restrict__ status)
{
    const uint32_t kept = OutChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) {
        status[OS_KEPT] = kept;
        if (RADIUS) {
            status[OS_ZERO] = 0ull; status[OS_CLOUD_MEAN] = 0ull; status[OS_STD] = 0ull; status[OS_THR] = 0ull;
            status[OS_M] = M; status[6] = 0ull; status[7] = 0ull;
        }
    }
}

template <bool RADIUS>
__global__ __launch_bounds__(kOutThreads) void outlier_write_kernel(uint32_t M, const uint64_t *__restrict__ vals,
                                                                    const double *__restrict__ hdr, float radius,
                                                                    const uint32_t *__restrict__ blk, const float *__restrict__ xyz,
                                                                    const float *__restrict__ normals, float *__restrict__ out_xyz,
                                                                    float *__restrict__ out_normals, int32_t *__restrict__ out_index)
{
    OutChunks::write_rows(outlier_keep_mask<RADIUS>(M, vals, hdr, radius, OutChunks::first()), blk, xyz, normals, out_xyz,
                          out_normals, out_index);
}

struct OutlierScratch {
    void *nn;
    uint64_t *vals;
    unsigned long long *partials;
    double *hdr;
    uint32_t *blk;
    size_t total;
    int nblk;
};

static OutlierScratch outlier_layout(int M, int k, void *base)
{
    OutlierScratch s;
    Arena a(base);
    s.nblk = OutChunks::count((size_t)M);
    s.nn = a.take<char>(nn_k_scratch_bytes(M, M, k));
    s.vals = a.take<uint64_t>((size_t)M);
    s.partials = a.take<unsigned long long>(2 * (size_t)kOutMaxBlocks);
    s.hdr = a.take<double>(OH_WORDS);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.total = a.off;
    return s;
}

size_t outlier_scratch_bytes(int M, int k) { return (M > 0 && k >= 1 && k <= SLS_NN_K_MAX) ? outlier_layout(M, k, nullptr).total : 0; }

template <bool RADIUS>
static int outlier_compact(int M, const OutlierScratch &s, float radius, const float *xyz, const float *normals, float *out_xyz,
                           float *out_normals, int32_t *out_index, uint64_t *out_status, hipStream_t st)
{
    unsigned long long *status = (unsigned long long *)out_status;
    hipLaunchKernelGGL(outlier_count_kernel<RADIUS>, dim3(s.nblk), dim3(kOutThreads), 0, st, (uint32_t)M, (const uint64_t *)s.vals,
                       (const double *)s.hdr, radius, s.blk);
    SLS_LAUNCH_CHECK("outlier_count_kernel");
    hipLaunchKernelGGL(outlier_scan_kernel<RADIUS>, dim3(1), dim3(kOutThreads), 0, st, (uint32_t)M, s.nblk, s.blk, status);
    SLS_LAUNCH_CHECK("outlier_scan_kernel");
    if (out_xyz || out_normals || out_index) {
        hipLaunchKernelGGL(outlier_write_kernel<RADIUS>, dim3(s.nblk), dim3(kOutThreads), 0, st, (uint32_t)M, (const uint64_t *)s.vals,
                           (const double *)s.hdr, radius, (const uint32_t *)s.blk, xyz, normals, out_xyz, out_normals, out_index);
        SLS_LAUNCH_CHECK("outlier_write_kernel");
    }
    return SLS_OK;
}

int launch_outlier_statistical(int M, const float *xyz, const float *normals, int k, double std_ratio, float *out_xyz,
                               float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, hipStream_t st)
{
    const OutlierScratch s = outlier_layout(M, k, scratch);
    int rc = launch_nn_query_k(M, xyz, M, xyz, k, SLS_NN_K_MAX, nullptr, nullptr, (double *)s.vals, nullptr, s.nn, st);
    if (rc) return rc;
    int nblocks = (M + kOutThreads - 1) / kOutThreads;
    if (nblocks > kOutMaxBlocks) nblocks = kOutMaxBlocks;
    unsigned long long *status = (unsigned long long *)out_status;
    hipLaunchKernelGGL(outlier_partial_kernel<0>, dim3(nblocks), dim3(kOutThreads), 0, st, M, (const double *)s.vals,
                       (const double *)s.hdr, s.partials);
    SLS_LAUNCH_CHECK("outlier_partial_kernel");
    hipLaunchKernelGGL(outlier_final_kernel<0>, dim3(1), dim3(kOutThreads), 0, st, M, nblocks, (const unsigned long long *)s.partials,
                       std_ratio, s.hdr, status);
    SLS_LAUNCH_CHECK("outlier_final_kernel");
    hipLaunchKernelGGL(outlier_partial_kernel<1>, dim3(nblocks), dim3(kOutThreads), 0, st, M, (const double *)s.vals,
                       (const double *)s.hdr, s.partials);
    SLS_LAUNCH_CHECK("outlier_partial_kernel");
    hipLaunchKernelGGL(outlier_final_kernel<1>, dim3(1), dim3(kOutThreads), 0, st, M, nblocks, (const unsigned long long *)s.partials,
                       std_ratio, s.hdr, status);
    SLS_LAUNCH_CHECK("outlier_final_kernel");
    return outlier_compact<false>(M, s, 0.0f, xyz, normals, out_xyz, out_normals, out_index, out_status, st);
}

int launch_outlier_radius(int M, const float *xyz, const float *normals, int nb_points, float radius, float *out_xyz,
                          float *out_normals, int32_t *out_index, uint64_t *out_status, void *scratch, hipStream_t st)
{
    const OutlierScratch s = outlier_layout(M, nb_points + 1, scratch);
    const int rc = launch_nn_query_k(M, xyz, M, xyz, nb_points + 1, SLS_NN_K_MAX, nullptr, nullptr, nullptr, s.vals, s.nn, st);
    if (rc) return rc;
    return outlier_compact<true>(M, s, radius, xyz, normals, out_xyz, out_normals, out_index, out_status, st);
}

}  // namespace sls
