// sls_ground.hip — sls_ground_segment: the ground of a LiDAR scan by a region-wise plane fit in the manner of Patchwork
// (include/sls_ground_math.h states the rule and what it is not).  One native call, nothing read back inside it, no float
// atomics; launches ordered by the stream alone:
//   ground_init     the header words (the item count for the sorter) and the status words
//   ground_keys     a thread per point: key = bin << 32 | ordered z (bin SLS_GROUND_BINS: no bin), value = the row; the
//                   label of a point without a bin is written 0 here, its bin -1; non-finite rows are counted with one
//                   integer atomic per wave
//   the stable LSD sort   41 key bits = four passes of 11-bit digits (sls_radix.hip: radix_sort_pairs_u64) — stable, so
//                   equal z inside a bin stay in row order
//   ground_gather   the sorted rows as float4 (x, y, z, row as bits): the fit reads contiguous 16-byte rows, several times
//                   each, instead of 12-byte gathers through the permutation (sls_normals.hip: what those cost there)
//   ground_fit      one wave = one 64-thread workgroup per bin, so the 504 bins spread over the CUs and a crowded near bin
//                   holds no other back: two lower-bound searches in the sorted keys give the bin's [lo, hi), then the
//                   header's sls_ground_fit — lane l sums the entries l, l + 64, ... (branch-free, four rows' loads in
//                   flight: the longest bin's walk is what the kernel costs), a fixed xor butterfly adds the lanes;
//                   the plane and the Jacobi state live in registers, the distance test is made again in the covariance
//                   pass, not stored (the entries per lane are unbounded) — then the bin's record, and the labels and bin
//                   numbers of its points through the row index.  The status counts are integer atomics, one per wave.
#include "sls_launch.hpp"
#include "../../include/sls_ground_math.h"

namespace sls {

constexpr int kGroundThreads = 256;

// hdr words of the scratch
enum { GH_COUNT = 0 };

__global__ void ground_init_kernel(uint32_t *hdr, uint32_t *status, uint32_t M)
{
    if (threadIdx.x < 8) status[threadIdx.x] = threadIdx.x == 7 ? 1u : 0u;
    if (hdr && threadIdx.x < 16) hdr[threadIdx.x] = threadIdx.x == GH_COUNT ? M : 0u;
}

__global__ __launch_bounds__(kGroundThreads) void ground_keys_kernel(int M, const float *__restrict__ xyz, SlsGroundParams prm,
                                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                                     uint8_t *__restrict__ label, int32_t *__restrict__ out_bin,
                                                                     uint32_t *status)
{
    const size_t i = (size_t)blockIdx.x * kGroundThreads + threadIdx.x;
    bool bad = false;
    if (i < (size_t)M) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        bad = !(sls_ground_finite(x) && sls_ground_finite(y) && sls_ground_finite(z));
        const int bin = sls_ground_bin(x, y, z, &prm);
        keys[i] = sls_ground_key(bin, z);
        vals[i] = (uint32_t)i;
        if (bin < 0) {
            label[i] = 0;
            if (out_bin) out_bin[i] = -1;
        }
    }
    const uint64_t m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&status[2], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(kGroundThreads) void ground_gather_kernel(uint32_t M, const float *__restrict__ xyz,
                                                                       const uint32_t *__restrict__ order, float4 *__restrict__ rows)
{
    const size_t p = (size_t)blockIdx.x * kGroundThreads + threadIdx.x;
    if (p >= (size_t)M) return;
    // (order is a permutation of [0, M) as long as the sorter is right; the index is a word read from memory and becomes
    //  an address, so it is clamped: a wrong word then gives a wrong row, not a read outside xyz)
    const size_t i = min(order[p], M - 1u);
    rows[p] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __uint_as_float((uint32_t)i));
}

// the first position in the ascending keys[0, M) whose key is >= key (every lane makes the same search)
__device__ __forceinline__ uint32_t ground_lower_bound(const uint64_t *__restrict__ keys, uint32_t M, uint64_t key)
{
    uint32_t lo = 0u, hi = M;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void ground_fit_kernel(uint32_t M, const uint64_t *__restrict__ keys, const float4 *__restrict__ rows,
                                                        SlsGroundParams prm, uint8_t *__restrict__ label,
                                                        int32_t *__restrict__ out_bin, double *__restrict__ out_planes,
                                                        int32_t *__restrict__ out_info, uint32_t *status)
{
    const int bin = (int)blockIdx.x, lane = (int)threadIdx.x;
    const uint32_t lo = ground_lower_bound(keys, M, (uint64_t)bin << 32);
    const uint32_t hi = ground_lower_bound(keys, M, (uint64_t)(bin + 1) << 32);
    const int n = (int)(hi - lo);
    const float *bin_rows = (const float *)(rows + lo);
    double plane[8];
    int32_t info[4];
    SlsGroundSet set;
    sls_ground_fit(bin_rows, n, bin, lane, &prm, plane, info, &set);
    const bool ground = info[3] == SLS_GROUND_GROUND;
    uint32_t found = 0u;
    for (int e = lane; e < n; e += 64) {
        const float4 r = rows[lo + (uint32_t)e];
        const size_t i = min(__float_as_uint(r.w), M - 1u);     // (likewise: it addresses two STORES; one v_min a row)
        const bool g = ground && sls_ground_member(&set, e, r.x, r.y, r.z);
        label[i] = g ? 1 : 0;
        if (out_bin) out_bin[i] = bin;
        found += g ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) found += __shfl_xor(found, off, 64);
    if (lane == 0) {
        if (n) atomicAdd(&status[0], (uint32_t)n);
        if (found) atomicAdd(&status[1], found);
        if (ground) atomicAdd(&status[3], 1u);
    }
    if (out_planes && lane < 8) {
        // (a choice between scalars, not between addresses: the record stays in registers)
        double v = plane[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) v = lane == k ? plane[k] : v;
        out_planes[8 * (size_t)bin + lane] = v;
    }
    if (out_info && lane < 4) {
        int32_t v = info[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) v = lane == k ? info[k] : v;
        out_info[4 * (size_t)bin + lane] = v;
    }
}

// scratch layout (all 256-byte aligned)
struct GroundScratch {
    uint32_t *hdr;
    uint64_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp;
    float4 *rows;
    void *sort;
    size_t sort_bytes, total;
};

constexpr int kGroundKeyBits = 41;      // 32 of the ordered z + 9 of the bin (SLS_GROUND_BINS = 504 < 512, "no bin" included)
static_assert(SLS_GROUND_BINS < (1 << (kGroundKeyBits - 32)), "the bin field of the key");

static GroundScratch ground_layout(int M, void *base)
{
    GroundScratch s;
    Arena a(base);
    const size_t n = (size_t)M;
    s.hdr = a.take<uint32_t>(16);
    s.keys = a.take<uint64_t>(n);
    s.keys_tmp = a.take<uint64_t>(n);
    s.vals = a.take<uint32_t>(n);
    s.vals_tmp = a.take<uint32_t>(n);
    s.rows = a.take<float4>(n);
    s.sort_bytes = sort_scratch_bytes((uint64_t)M);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t ground_scratch_bytes(int M) { return M > 0 ? ground_layout(M, nullptr).total : 0; }

int launch_ground_segment(int M, const float *xyz, const SlsGroundParams &prm, uint8_t *out_label, int32_t *out_bin,
                          double *out_planes, int32_t *out_info, uint32_t *out_status, void *scratch, hipStream_t st)
{
    if (M == 0) {
        hipLaunchKernelGGL(ground_init_kernel, dim3(1), dim3(64), 0, st, (uint32_t *)nullptr, out_status, 0u);
        SLS_LAUNCH_CHECK("ground_init_kernel");
        return SLS_OK;
    }
    const GroundScratch s = ground_layout(M, scratch);
    const uint32_t Mu = (uint32_t)M;
    const dim3 grid = grid_for((size_t)M, kGroundThreads);
    hipLaunchKernelGGL(ground_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, out_status, Mu);
    SLS_LAUNCH_CHECK("ground_init_kernel");
    hipLaunchKernelGGL(ground_keys_kernel, grid, dim3(kGroundThreads), 0, st, M, xyz, prm, s.keys, s.vals, out_label, out_bin,
                       out_status);
    SLS_LAUNCH_CHECK("ground_keys_kernel");
    int which = 0;
    const int rc = radix_sort_pairs_u64(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + GH_COUNT, Mu, kGroundKeyBits, s.sort,
                                        s.sort_bytes, &which, st);
    if (rc) return rc;
    const uint64_t *keys = which ? s.keys_tmp : s.keys;
    const uint32_t *order = which ? s.vals_tmp : s.vals;
    hipLaunchKernelGGL(ground_gather_kernel, grid, dim3(kGroundThreads), 0, st, Mu, xyz, order, s.rows);
    SLS_LAUNCH_CHECK("ground_gather_kernel");
    hipLaunchKernelGGL(ground_fit_kernel, dim3(SLS_GROUND_BINS), dim3(64), 0, st, Mu, keys, (const float4 *)s.rows, prm, out_label,
                       out_bin, out_planes, out_info, out_status);
    SLS_LAUNCH_CHECK("ground_fit_kernel");
    return SLS_OK;
}

}  // namespace sls
