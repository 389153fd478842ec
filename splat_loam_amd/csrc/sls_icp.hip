// sls_icp.hip — sls_cloud_icp: Gauss-Newton ICP of a source cloud onto a target cloud on exact nearest neighbours
// (include/sls_icp_math.h states the rule).  One native call, nothing read back inside it, no float atomics:
//   once:      the target's spatial index (sls_knn.hip: nn_index_target) and icp_pack_kernel, which copies the target's
//              points and normals into float4 rows in ORIGINAL order — the search returns original row numbers, and a
//              16-byte row is one aligned load where a 12-byte row of the caller's array straddles two 16-byte segments
//              every other time;
//   per pass:  icp_transform_kernel moves the source by the device-resident pose and writes p' and its curve code in the
//              target's cube; the sorter, the gather and nn_query_kernel run unchanged (nn_index_query);
//              icp_linearize_kernel, a thread per source point, gathers its target row and normal, computes the 29 terms
//              in float64 and reduces them — xor butterfly across the wave, the 4 waves in order through LDS, one partial
//              row per block; icp_solve_kernel, one workgroup, adds the partial rows in a fixed order and lane 0 runs
//              the header's solve on the device-resident pose.
// The state lives in out_status: word 18 is the stage (0 updating, 1 updates ended, 2 evaluated).  Once it is 2 the
// linearise and solve kernels return at once and the transform kernel finds the pose unchanged, so the passes that are
// still enqueued rewrite what is already there: iterations = 50 gives the bits of iterations = k.
#include "sls_geom.hpp"
#include "../../include/sls_icp_math.h"

namespace sls {

constexpr int kIcpBlock = SLS_ICP_BLOCK;            // threads per block of the linearisation and of the solve
constexpr int kIcpRow = 32;                         // doubles per partial row (29 used): 256 bytes
constexpr int kIcpStage = 18;                       // out_status word: 0 updating, 1 updates ended, 2 evaluated
static_assert(kIcpBlock == 256, "the sum's order is written for 4 waves of 64 (include/sls_icp_math.h)");
static_assert(SLS_ICP_STATUS_WORDS == 20 && SLS_ICP_TERMS <= kIcpRow, "status layout");

struct IcpPose { double T[12]; };

// Ms == 0: nothing to associate — the status is final at once, "too few inliers" at the initial pose, the sums zeros
__global__ void icp_init_kernel(IcpPose init, int Ms, int Mt, unsigned long long *__restrict__ status, double *__restrict__ out_system)
{
    const int t = threadIdx.x;
    if (Ms == 0 && out_system && t < kIcpRow) out_system[t] = 0.0;
    if (t >= SLS_ICP_STATUS_WORDS) return;
    unsigned long long v = 0ull;
    if (t == 2) v = (unsigned long long)Ms;
    else if (t == 4) v = Ms == 0 ? (unsigned long long)SLS_ICP_FLAG_FEW : 0ull;
    else if (t == kIcpStage) v = Ms == 0 ? 2ull : 0ull;
    else if (t == 3) v = (unsigned long long)Mt;
    else if (t >= 6 && t < 18) v = (unsigned long long)__double_as_longlong(init.T[t - 6]);
    status[t] = v;
}

__global__ __launch_bounds__(256) void icp_pack_kernel(int Mt, const float *__restrict__ xyz, const float *__restrict__ normals,
                                                       float4 *__restrict__ rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Mt) return;
    rows[2 * i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
    rows[2 * i + 1] = normals ? make_float4(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], 0.0f)
                              : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// p' = (float)(R p + t) and its curve code in the target's cube: the transform fused with knn_morton_kernel
__global__ __launch_bounds__(256) void icp_transform_kernel(int Ms, const float *__restrict__ xyz,
                                                            const unsigned long long *__restrict__ status,
                                                            const uint32_t *__restrict__ bbox, int key_bits,
                                                            float *__restrict__ moved, uint32_t *__restrict__ keys,
                                                            uint32_t *__restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Ms) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = __longlong_as_double((long long)status[6 + k]);
    const float p[3] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
    float q[3];
    sls_icp_transform(T, p, q);
    moved[3 * i] = q[0]; moved[3 * i + 1] = q[1]; moved[3 * i + 2] = q[2];
    keys[i] = curve_code(q[0], q[1], q[2], bbox, key_bits);
    vals[i] = (uint32_t)i;
}

// the block's sum of every thread's acc[29], by the steps 2 and 3 of the header: valid in thread 0
__device__ __forceinline__ void icp_block_sum(double acc[SLS_ICP_TERMS])
{
    __shared__ double s_w[3][SLS_ICP_TERMS];
    xor_butterfly<SLS_ICP_TERMS>(acc);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0 && w > 0) {
#pragma unroll
        for (int k = 0; k < SLS_ICP_TERMS; ++k) s_w[w - 1][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SLS_ICP_TERMS; ++k) acc[k] = ((acc[k] + s_w[0][k]) + s_w[1][k]) + s_w[2][k];
    }
}

template <int METHOD>
__global__ __launch_bounds__(kIcpBlock) void icp_linearize_kernel(int Ms, const float *__restrict__ moved,
                                                                  const float4 *__restrict__ rows,
                                                                  const float *__restrict__ dist2,
                                                                  const int32_t *__restrict__ index, float gate2,
                                                                  const unsigned long long *__restrict__ status,
                                                                  double *__restrict__ partials)
{
    if (status[kIcpStage] == 2ull) return;              // (uniform over the grid: written by the previous solve alone)
    const size_t i = (size_t)blockIdx.x * kIcpBlock + threadIdx.x;
    double acc[SLS_ICP_TERMS];
    bool inlier = false;
    float pt[3] = { 0.0f, 0.0f, 0.0f }, q[3] = { 0.0f, 0.0f, 0.0f }, n[3] = { 0.0f, 0.0f, 0.0f };
    if (i < (size_t)Ms) {
        inlier = dist2[i] <= gate2 && index[i] >= 0;   // (the index is a real row whenever d2 is not NaN; a guard)
        if (inlier) {
            const size_t j = (size_t)index[i];          // (an inlier has a finite d2, so a real target row)
            const float4 tq = rows[2 * j];
            q[0] = tq.x; q[1] = tq.y; q[2] = tq.z;
            if (METHOD == SLS_ICP_PLANE) { const float4 tn = rows[2 * j + 1]; n[0] = tn.x; n[1] = tn.y; n[2] = tn.z; }
            pt[0] = moved[3 * i]; pt[1] = moved[3 * i + 1]; pt[2] = moved[3 * i + 2];
        }
    }
    sls_icp_terms(METHOD, inlier ? 1 : 0, pt, q, n, acc);
    icp_block_sum(acc);
    if (threadIdx.x == 0) {
        double *row = partials + (size_t)blockIdx.x * kIcpRow;
#pragma unroll
        for (int k = 0; k < SLS_ICP_TERMS; ++k) row[k] = acc[k];
    }
}

__global__ __launch_bounds__(kIcpBlock) void icp_solve_kernel(int nblocks, const double *__restrict__ partials, SlsIcpParams prm,
                                                              int update, unsigned long long *__restrict__ status,
                                                              double *__restrict__ out_system)
{
    const unsigned long long stage = status[kIcpStage];
    if (stage == 2ull) return;
    double acc[SLS_ICP_TERMS];
#pragma unroll
    for (int k = 0; k < SLS_ICP_TERMS; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kIcpBlock) {
        const double *row = partials + (size_t)b * kIcpRow;
#pragma unroll
        for (int k = 0; k < SLS_ICP_TERMS; ++k) acc[k] += row[k];
    }
    icp_block_sum(acc);
    if (threadIdx.x != 0) return;
    status[1] = (unsigned long long)acc[28];
    status[5] = (unsigned long long)__double_as_longlong(acc[27]);
    if (out_system) {
        for (int k = 0; k < SLS_ICP_TERMS; ++k) out_system[k] = acc[k];
        for (int k = SLS_ICP_TERMS; k < kIcpRow; ++k) out_system[k] = 0.0;
    }
    if (stage == 1ull || !update) { status[kIcpStage] = 2ull; return; }     // this was the evaluation pass
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = __longlong_as_double((long long)status[6 + k]);
    const int flags = sls_icp_solve(acc, &prm, T, nullptr);
    if (flags & (SLS_ICP_FLAG_FEW | SLS_ICP_FLAG_NOT_PD)) {                 // the pose is kept: this pass evaluated it
        status[4] |= (unsigned long long)flags;
        status[kIcpStage] = 2ull;
        return;
    }
    for (int k = 0; k < 12; ++k) status[6 + k] = (unsigned long long)__double_as_longlong(T[k]);
    status[0] += 1ull;
    if (flags & SLS_ICP_FLAG_CONVERGED) { status[4] |= (unsigned long long)SLS_ICP_FLAG_CONVERGED; status[kIcpStage] = 1ull; }
}

struct IcpScratch {
    void *nn;
    float *moved, *dist2;
    int32_t *index;
    float4 *rows;
    double *partials;
    size_t total;
};

static size_t icp_blocks(int Ms) { return ((size_t)Ms + kIcpBlock - 1) / kIcpBlock; }

static IcpScratch icp_layout(int Ms, int Mt, void *base)
{
    IcpScratch s;
    Arena a(base);
    s.nn = a.take<char>(nn_scratch_bytes(Mt, Ms));
    s.moved = a.take<float>(3 * (size_t)Ms);
    s.dist2 = a.take<float>((size_t)Ms);
    s.index = a.take<int32_t>((size_t)Ms);
    s.rows = a.take<float4>(2 * (size_t)Mt);
    s.partials = a.take<double>((icp_blocks(Ms) + 1) * kIcpRow);
    s.total = a.off;
    return s;
}

size_t cloud_icp_scratch_bytes(int Ms, int Mt) { return (Ms >= 0 && Mt >= 1) ? icp_layout(Ms, Mt, nullptr).total : 0; }

int launch_cloud_icp(int Ms, const float *source_xyz, int Mt, const float *target_xyz, const float *target_normals,
                     const SlsIcpParams &prm, const double *init_pose12, uint64_t *out_status, double *out_system,
                     int32_t *out_index, float *out_dist2, void *scratch, hipStream_t st)
{
    unsigned long long *status = (unsigned long long *)out_status;
    IcpPose init;
    for (int k = 0; k < 12; ++k) init.T[k] = init_pose12[k];
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, st, init, Ms, Mt, status, out_system);
    SLS_LAUNCH_CHECK("icp_init_kernel");
    if (Ms == 0) return SLS_OK;
    const IcpScratch s = icp_layout(Ms, Mt, scratch);
    const int nblocks = (int)icp_blocks(Ms);
    ScopedTimer tm(T_KNN, st);
    NnIndexRef ref;
    int rc = nn_index_target(Mt, target_xyz, Ms, s.nn, st, &ref);
    if (rc) return rc;
    const bool plane = prm.method == SLS_ICP_PLANE;
    hipLaunchKernelGGL(icp_pack_kernel, grid_for((size_t)Mt, 256), dim3(256), 0, st, Mt, target_xyz, plane ? target_normals : nullptr,
                       s.rows);
    SLS_LAUNCH_CHECK("icp_pack_kernel");
    float *d2 = out_dist2 ? out_dist2 : s.dist2;
    int32_t *idx = out_index ? out_index : s.index;
    const float gate2 = sls_icp_gate2(prm.max_distance);
    for (int it = 0; it <= prm.iterations; ++it) {
        hipLaunchKernelGGL(icp_transform_kernel, grid_for((size_t)Ms, 256), dim3(256), 0, st, Ms, source_xyz,
                           (const unsigned long long *)status, ref.bbox, ref.key_bits, s.moved, ref.qkeys, ref.qvals);
        SLS_LAUNCH_CHECK("icp_transform_kernel");
        rc = nn_index_query(Mt, Ms, s.moved, ref, d2, idx, s.nn, st);
        if (rc) return rc;
        if (plane)
            hipLaunchKernelGGL(icp_linearize_kernel<SLS_ICP_PLANE>, dim3(nblocks), dim3(kIcpBlock), 0, st, Ms, (const float *)s.moved,
                               (const float4 *)s.rows, (const float *)d2, (const int32_t *)idx, gate2,
                               (const unsigned long long *)status, s.partials);
        else
            hipLaunchKernelGGL(icp_linearize_kernel<SLS_ICP_POINT>, dim3(nblocks), dim3(kIcpBlock), 0, st, Ms, (const float *)s.moved,
                               (const float4 *)s.rows, (const float *)d2, (const int32_t *)idx, gate2,
                               (const unsigned long long *)status, s.partials);
        SLS_LAUNCH_CHECK("icp_linearize_kernel");
        hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(kIcpBlock), 0, st, nblocks, (const double *)s.partials, prm,
                           it < prm.iterations ? 1 : 0, status, out_system);
        SLS_LAUNCH_CHECK("icp_solve_kernel");
    }
    return SLS_OK;
}

}  // namespace sls
