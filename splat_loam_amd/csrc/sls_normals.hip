// sls_normals.hip — sls_cloud_normals: the normals of a point cloud by PCA over each point's nearest neighbours, oriented
// towards a viewpoint (include/sls_normals_math.h states the rule).  One native call, nothing read back inside it:
//   1. the self-query (sls_knn.hip: launch_nn_query_k; beyond k = 32 its two passes) writes every point's k-list — the
//      out_dist2 / out_index rows of sls_nn_query_k — into the scratch;
//   2. cloud_normals_kernel, one thread per point: the header's functions on the point's rows.  The two rows of a point
//      are contiguous (k floats, k int32).  The neighbours' coordinates are 12-byte gathers from the caller's xyz: the
//      lists hold ORIGINAL row numbers, while the search's float4 copy is in curve order, so 16-byte reads from it would
//      need an inverse permutation built and read first (4 more bytes per neighbour than the 4 a float4 wastes anyway).
//      Each neighbour is read twice — the mean, then the covariance about it, as the rule demands — and the second pass
//      finds the first one's lines in cache.  All sums are per-thread loops in list order: no atomics, no reductions
//      across lanes, the same bits every run.
#include "sls_launch.hpp"
#include "../../include/sls_normals_math.h"

namespace sls {

constexpr int kNormalsThreads = 256;

struct NormalsView { float v[3]; };

__global__ __launch_bounds__(kNormalsThreads) void cloud_normals_kernel(int M, const float *__restrict__ xyz, int k, float radius,
                                                                        NormalsView view, const float *__restrict__ dist2,
                                                                        const int32_t *__restrict__ index,
                                                                        float *__restrict__ out_normals,
                                                                        int32_t *__restrict__ out_count,
                                                                        float *__restrict__ out_eigenvalues)
{
    const size_t i = (size_t)blockIdx.x * kNormalsThreads + threadIdx.x;
    if (i >= (size_t)M) return;
    float nrm[3], eig[3];
    const int n = sls_normals_point(xyz, (int)i, dist2 + i * (size_t)k, index + i * (size_t)k, k, radius, view.v, nrm, eig);
    out_normals[3 * i] = nrm[0]; out_normals[3 * i + 1] = nrm[1]; out_normals[3 * i + 2] = nrm[2];
    if (out_count) out_count[i] = n;
    if (out_eigenvalues) { out_eigenvalues[3 * i] = eig[0]; out_eigenvalues[3 * i + 1] = eig[1]; out_eigenvalues[3 * i + 2] = eig[2]; }
}

struct NormalsScratch {
    void *nn;
    float *dist2;
    int32_t *index;
    uint64_t *last;                                     // the search's key buffer between its two passes (k > 32)
    size_t total;
};

static NormalsScratch normals_layout(int M, int k, void *base)
{
    NormalsScratch s;
    Arena a(base);
    s.nn = a.take<char>(nn_scratch_bytes(M, M));
    s.dist2 = a.take<float>((size_t)M * (size_t)k);
    s.index = a.take<int32_t>((size_t)M * (size_t)k);
    s.last = a.take<uint64_t>((size_t)M);
    s.total = a.off;
    return s;
}

size_t cloud_normals_scratch_bytes(int M, int k)
{
    return (M > 0 && k >= 1 && k <= SLS_NORMALS_NN_MAX) ? normals_layout(M, k, nullptr).total : 0;
}

int launch_cloud_normals(int M, const float *xyz, int k, float radius, const float *viewpoint3, float *out_normals,
                         int32_t *out_count, float *out_eigenvalues, void *scratch, hipStream_t st)
{
    const NormalsScratch s = normals_layout(M, k, scratch);
    const int rc = launch_nn_query_k(M, xyz, M, xyz, k, SLS_NORMALS_NN_MAX, s.dist2, s.index, nullptr,
                                     k > SLS_NN_K_MAX ? s.last : nullptr, s.nn, st);
    if (rc) return rc;
    NormalsView view;
    view.v[0] = viewpoint3[0]; view.v[1] = viewpoint3[1]; view.v[2] = viewpoint3[2];
    hipLaunchKernelGGL(cloud_normals_kernel, grid_for((size_t)M, kNormalsThreads), dim3(kNormalsThreads), 0, st, M, xyz, k, radius,
                       view, (const float *)s.dist2, (const int32_t *)s.index, out_normals, out_count, out_eigenvalues);
    SLS_LAUNCH_CHECK("cloud_normals_kernel");
    return SLS_OK;
}

}  // namespace sls
