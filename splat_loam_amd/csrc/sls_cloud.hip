// sls_cloud.hip — what the reference's evaluate_recon does to its inputs before the metric block
// (utils/eval_utils.py:96-120): voxel down-sampling of a cloud (sls_voxel_downsample) and area-weighted sampling of a
// triangle mesh (sls_mesh_sample).  include/sls_cloud_math.h states the arithmetic, tests/cloud_ref.py restates it in
// NumPy.  Built EXACT (-ffp-contract=off): voxel indices, weights and drawn faces are integers of the contract.
//
// sls_voxel_downsample, launches ordered by the stream alone:
//   voxel_init / voxel_bbox     float32 minimum per axis (integer atomicMin in the ordered domain: order-free) and
//                               the count of points with a non-finite coordinate, which take no part in the minimum
//   voxel_keys                  key = ix | iy << 21 | iz << 42 and the identity permutation; a non-finite point, or one
//                               with an index >= 2^21, gets key 0 (and is counted): nothing a key holds is an address
//   the stable LSD sort         63 key bits = six passes of 11-bit digits over (u64 key, u32 index) pairs
//                               (sls_radix.hip: radix_sort_pairs_u64) — stable, so a voxel's points stay in input order
//   voxel_heads / _scan / _segments   head flags of the sorted keys, their scan in chunks of 1024 positions:
//                               seg_start[v] = first sorted position of voxel v, seg_start[n_voxels] = M, the status words
//   voxel_sum                   a lane per voxel adds its points in sorted (= input) order; a voxel of more than 64
//                               points is left to the whole wave afterwards: lane l adds the points l, l + 64, ... and a
//                               fixed xor butterfly adds the lanes.  No floating-point atomics anywhere.
//
// sls_mesh_sample:
//   mesh_init / mesh_area       float64 area per face (0 for a dropped face), the largest area as an integer atomicMax
//                               of its bits (areas are >= 0: the bits order like the values), the bad-index count
//   mesh_weight_sums / mesh_scan / mesh_prefix   w = floor(A / A_max 2^32), inclusive prefix C in chunks of 1024 faces
//                               (64-bit integers: exact in any order), W and the status words
//   mesh_sample                 a thread per sample: Philox words, t = mulhi64(., W), bisection of C, the point
#include "sls_geom.hpp"
#include "sls_scan.hpp"
#include "../../include/sls_cloud_math.h"

namespace sls {

constexpr int kCloudThreads = 256;
using CloudChunks = Chunks<kCloudThreads, 4>;                // the chunked scans: 1024 items per workgroup
constexpr uint32_t kVoxelLong = 64;                          // a voxel of more points is summed by 64 lanes
constexpr int kVoxelKeyBits = 3 * SLS_VOXEL_INDEX_BITS;      // 63

// hdr words of the voxel scratch
enum { VH_MIN = 0, VH_NONFINITE = 3, VH_BIG = 4, VH_COUNT = 5, VH_NVOX = 6 };
// 64-bit hdr words of the mesh scratch
enum { MH_AMAX = 0, MH_BAD = 1, MH_W = 2 };

// ---------------------------------------------------------------------------------------------------------------------
// voxel down-sampling
// ---------------------------------------------------------------------------------------------------------------------
__global__ void voxel_init_kernel(uint32_t *hdr, uint32_t M)
{
    if (threadIdx.x < 3) hdr[threadIdx.x] = 0xFFFFFFFFu;        // min (ordered domain)
    else if (threadIdx.x == VH_COUNT) hdr[VH_COUNT] = M;        // item count for the sorter
    else if (threadIdx.x < 8) hdr[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kCloudThreads) void voxel_bbox_kernel(int M, const float *__restrict__ xyz, uint32_t *hdr)
{
    bbox_min<kCloudThreads>((uint32_t)M, xyz, nullptr, hdr + VH_MIN, hdr + VH_NONFINITE);
}

__global__ __launch_bounds__(kCloudThreads) void voxel_keys_kernel(int M, const float *__restrict__ xyz, double voxel_size,
                                                                   uint32_t *hdr, uint64_t *__restrict__ keys,
                                                                   uint32_t *__restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * kCloudThreads + threadIdx.x;
    bool big = false;
    if (i < (size_t)M) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        uint64_t key = 0u;
        if (finite_f32(x) && finite_f32(y) && finite_f32(z)) {    // (then the minima are finite too)
            const double ox = sls_voxel_origin(ord2f(hdr[VH_MIN + 0]), voxel_size),
                         oy = sls_voxel_origin(ord2f(hdr[VH_MIN + 1]), voxel_size),
                         oz = sls_voxel_origin(ord2f(hdr[VH_MIN + 2]), voxel_size);
            big = !sls_voxel_key(x, y, z, ox, oy, oz, voxel_size, &key);
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    const uint64_t m = __ballot(big);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&hdr[VH_BIG], (uint32_t)__popcll(m));
}

// the head flags of this thread's four consecutive sorted positions, as a bit mask
__device__ __forceinline__ uint32_t voxel_head_mask(uint32_t M, const uint64_t *__restrict__ keys, uint32_t p0)
{
    return CloudChunks::head_mask(M, p0, [&](uint32_t p) { return keys[p]; });
}

__global__ __launch_bounds__(kCloudThreads) void voxel_heads_kernel(uint32_t M, const uint64_t *__restrict__ keys,
                                                                    uint32_t *__restrict__ blk)
{
    CloudChunks::total((uint32_t)__popc(voxel_head_mask(M, keys, CloudChunks::first())), blk);
}

__global__ __launch_bounds__(kCloudThreads) void voxel_scan_kernel(uint32_t M, int nblk, uint32_t *__restrict__ blk,
                                                                   uint32_t *__restrict__ hdr, uint32_t *__restrict__ seg_start,
                                                                   uint32_t *__restrict__ status)
{
    const uint32_t nv = CloudChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) {
        hdr[VH_NVOX] = nv;
        seg_start[nv <= M ? nv : M] = M;       // (nv <= M always: a head per position at most)
        status[0] = nv; status[1] = hdr[VH_NONFINITE]; status[2] = hdr[VH_BIG]; status[3] = 0u;
    }
}

__global__ __launch_bounds__(kCloudThreads) void voxel_segments_kernel(uint32_t M, const uint64_t *__restrict__ keys,
                                                                       const uint32_t *__restrict__ blk,
                                                                       uint32_t *__restrict__ seg_start)
{
    const uint32_t p0 = CloudChunks::first();
    const uint32_t mask = voxel_head_mask(M, keys, p0);
    uint32_t id = CloudChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < CloudChunks::kPer; ++j)
        if ((mask >> j) & 1u) {
            if (id < M) seg_start[id] = p0 + (uint32_t)j;       // (always: voxel ids are below the number of heads <= M)
            ++id;
        }
}

__global__ __launch_bounds__(kCloudThreads) void voxel_sum_kernel(uint32_t M, const float *__restrict__ xyz,
                                                                  const uint32_t *__restrict__ order,
                                                                  const uint32_t *__restrict__ seg_start,
                                                                  const uint32_t *__restrict__ hdr, float *__restrict__ out_xyz,
                                                                  int32_t *__restrict__ out_count)
{
    const uint32_t nv = min(hdr[VH_NVOX], M);
    const uint32_t v = blockIdx.x * (uint32_t)kCloudThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (v - (uint32_t)lane >= nv) return;                       // (wave-uniform: the whole wave lies beyond the voxels)
    const bool active = v < nv;
    uint32_t s = 0u, e = 0u;
    if (active) {
        e = min(seg_start[v + 1], M);
        s = min(seg_start[v], e);
    }
    const uint32_t len = e - s;
    if (active && len <= kVoxelLong) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (uint32_t p = s; p < e; ++p) {
            const size_t i = min(order[p], M - 1u);             // (a permutation of [0, M): the clamp never bites)
            sx += (double)xyz[3 * i]; sy += (double)xyz[3 * i + 1]; sz += (double)xyz[3 * i + 2];
        }
        if (len) {
            out_xyz[3 * (size_t)v] = sls_voxel_centroid(sx, len);
            out_xyz[3 * (size_t)v + 1] = sls_voxel_centroid(sy, len);
            out_xyz[3 * (size_t)v + 2] = sls_voxel_centroid(sz, len);
            if (out_count) out_count[v] = (int32_t)len;
        }
    }
    uint64_t longs = __ballot(active && len > kVoxelLong);
    while (longs) {                                             // (wave-uniform)
        const int src = (int)__builtin_ctzll(longs);
        longs &= longs - 1ull;
        const uint32_t s0 = (uint32_t)__shfl((int)s, src, 64), e0 = (uint32_t)__shfl((int)e, src, 64);
        double part[3] = { 0.0, 0.0, 0.0 };
        for (uint32_t p = s0 + (uint32_t)lane; p < e0; p += 64u) {
            const size_t i = min(order[p], M - 1u);
            part[0] += (double)xyz[3 * i]; part[1] += (double)xyz[3 * i + 1]; part[2] += (double)xyz[3 * i + 2];
        }
        xor_butterfly<3>(part);
        if (lane == src) {
            out_xyz[3 * (size_t)v] = sls_voxel_centroid(part[0], len);
            out_xyz[3 * (size_t)v + 1] = sls_voxel_centroid(part[1], len);
            out_xyz[3 * (size_t)v + 2] = sls_voxel_centroid(part[2], len);
            if (out_count) out_count[v] = (int32_t)len;
        }
    }
}

// scratch layout (all 256-byte aligned)
struct VoxelScratch {
    uint32_t *hdr;
    uint64_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp, *seg_start, *blk;
    void *sort;
    size_t sort_bytes, total;
    int nblk;
};

static VoxelScratch voxel_layout(int M, void *base)
{
    VoxelScratch s;
    Arena a(base);
    const size_t n = (size_t)M;
    s.nblk = CloudChunks::count(n);
    s.hdr = a.take<uint32_t>(16);
    s.keys = a.take<uint64_t>(n);
    s.keys_tmp = a.take<uint64_t>(n);
    s.vals = a.take<uint32_t>(n);
    s.vals_tmp = a.take<uint32_t>(n);
    s.seg_start = a.take<uint32_t>(n + 1);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.sort_bytes = sort_scratch_bytes((uint64_t)M);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t voxel_scratch_bytes(int M) { return M > 0 ? voxel_layout(M, nullptr).total : 0; }

int launch_voxel_downsample(int M, const float *xyz, double voxel_size, float *out_xyz, int32_t *out_count, uint32_t *out_status,
                            void *scratch, hipStream_t st)
{
    const VoxelScratch s = voxel_layout(M, scratch);
    const uint32_t Mu = (uint32_t)M;
    const int nb = (int)grid_for((size_t)M, kCloudThreads).x;
    hipLaunchKernelGGL(voxel_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, Mu);
    SLS_LAUNCH_CHECK("voxel_init_kernel");
    hipLaunchKernelGGL(voxel_bbox_kernel, dim3(nb < 1024 ? nb : 1024), dim3(kCloudThreads), 0, st, M, xyz, s.hdr);
    SLS_LAUNCH_CHECK("voxel_bbox_kernel");
    hipLaunchKernelGGL(voxel_keys_kernel, dim3(nb), dim3(kCloudThreads), 0, st, M, xyz, voxel_size, s.hdr, s.keys, s.vals);
    SLS_LAUNCH_CHECK("voxel_keys_kernel");
    int which = 0;
    int rc = radix_sort_pairs_u64(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + VH_COUNT, Mu, kVoxelKeyBits, s.sort,
                                  s.sort_bytes, &which, st);
    if (rc) return rc;
    const uint64_t *keys = which ? s.keys_tmp : s.keys;
    const uint32_t *order = which ? s.vals_tmp : s.vals;
    hipLaunchKernelGGL(voxel_heads_kernel, dim3(s.nblk), dim3(kCloudThreads), 0, st, Mu, keys, s.blk);
    SLS_LAUNCH_CHECK("voxel_heads_kernel");
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(kCloudThreads), 0, st, Mu, s.nblk, s.blk, s.hdr, s.seg_start, out_status);
    SLS_LAUNCH_CHECK("voxel_scan_kernel");
    hipLaunchKernelGGL(voxel_segments_kernel, dim3(s.nblk), dim3(kCloudThreads), 0, st, Mu, keys, (const uint32_t *)s.blk,
                       s.seg_start);
    SLS_LAUNCH_CHECK("voxel_segments_kernel");
    hipLaunchKernelGGL(voxel_sum_kernel, dim3(nb), dim3(kCloudThreads), 0, st, Mu, xyz, order, (const uint32_t *)s.seg_start,
                       (const uint32_t *)s.hdr, out_xyz, out_count);
    SLS_LAUNCH_CHECK("voxel_sum_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// mesh sampling
// ---------------------------------------------------------------------------------------------------------------------
__global__ void mesh_init_kernel(unsigned long long *hdr)
{
    if (threadIdx.x < 8) hdr[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kCloudThreads) void mesh_area_kernel(int V, int F, const float *__restrict__ vertices,
                                                                  const int32_t *__restrict__ faces, const float *__restrict__ crop_box,
                                                                  double *__restrict__ area, unsigned long long *hdr)
{
    const size_t f = (size_t)blockIdx.x * kCloudThreads + threadIdx.x;
    double A = 0.0;
    bool bad = false;
    if (f < (size_t)F) {
        const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        bad = i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V;
        if (!bad) {
            float v0[3], v1[3], v2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v0[k] = vertices[3 * (size_t)i0 + k]; v1[k] = vertices[3 * (size_t)i1 + k]; v2[k] = vertices[3 * (size_t)i2 + k];
            }
            A = sls_mesh_face_area(v0, v1, v2);
            if (!(A <= DBL_MAX)) A = 0.0;                       // not finite (a NaN included)
            if (crop_box) {
                float box[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) box[k] = crop_box[k];
                if (!(sls_mesh_inside(v0, box) && sls_mesh_inside(v1, box) && sls_mesh_inside(v2, box))) A = 0.0;
            }
        }
        area[f] = A;
    }
    unsigned long long bits = (unsigned long long)__double_as_longlong(A);      // A >= +0: the bits order like the values
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(bits, off, 64);
        bits = o > bits ? o : bits;
    }
    const uint64_t nbad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        if (bits) atomicMax(&hdr[MH_AMAX], bits);
        if (nbad) atomicAdd(&hdr[MH_BAD], (unsigned long long)__popcll(nbad));
    }
}

// the weights of this thread's four consecutive faces
__device__ __forceinline__ void mesh_weights(uint32_t F, const double *__restrict__ area, double amax, uint32_t f0,
                                             unsigned long long w[CloudChunks::kPer])
{
#pragma unroll
    for (int j = 0; j < CloudChunks::kPer; ++j) {
        const uint32_t f = f0 + (uint32_t)j;
        w[j] = f < F ? (unsigned long long)sls_mesh_weight(area[f], amax) : 0ull;
    }
}

__global__ __launch_bounds__(kCloudThreads) void mesh_weight_sums_kernel(uint32_t F, const double *__restrict__ area,
                                                                         const unsigned long long *__restrict__ hdr,
                                                                         unsigned long long *__restrict__ blk)
{
    const double amax = __longlong_as_double((long long)hdr[MH_AMAX]);
    unsigned long long w[CloudChunks::kPer];
    mesh_weights(F, area, amax, CloudChunks::first(), w);
    CloudChunks::total((w[0] + w[1]) + (w[2] + w[3]), blk);
}

__global__ __launch_bounds__(kCloudThreads) void mesh_scan_kernel(int nblk, unsigned long long *__restrict__ blk,
                                                                  unsigned long long *__restrict__ hdr, uint32_t n_samples,
                                                                  uint32_t *__restrict__ status)
{
    const unsigned long long W = CloudChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) {
        hdr[MH_W] = W;
        const unsigned long long nbad = hdr[MH_BAD];
        status[0] = W ? n_samples : 0u;
        status[1] = nbad > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nbad;
        status[2] = W ? 0u : 1u;
        status[3] = 0u;
    }
}

__global__ __launch_bounds__(kCloudThreads) void mesh_prefix_kernel(uint32_t F, const double *__restrict__ area,
                                                                    const unsigned long long *__restrict__ hdr,
                                                                    const unsigned long long *__restrict__ blk,
                                                                    unsigned long long *__restrict__ C)
{
    const double amax = __longlong_as_double((long long)hdr[MH_AMAX]);
    const uint32_t f0 = CloudChunks::first();
    unsigned long long w[CloudChunks::kPer];
    mesh_weights(F, area, amax, f0, w);
    unsigned long long run = CloudChunks::rank((w[0] + w[1]) + (w[2] + w[3]), blk);
#pragma unroll
    for (int j = 0; j < CloudChunks::kPer; ++j) {
        run += w[j];
        if (f0 + (uint32_t)j < F) C[f0 + (uint32_t)j] = run;    // inclusive
    }
}

__global__ __launch_bounds__(kCloudThreads) void mesh_sample_kernel(uint32_t V, uint32_t F, const float *__restrict__ vertices,
                                                                    const int32_t *__restrict__ faces,
                                                                    const unsigned long long *__restrict__ C,
                                                                    const unsigned long long *__restrict__ hdr, uint32_t n_samples,
                                                                    uint64_t seed, float *__restrict__ out_xyz,
                                                                    int32_t *__restrict__ out_face)
{
    const uint32_t i = blockIdx.x * (uint32_t)kCloudThreads + threadIdx.x;
    const uint64_t W = hdr[MH_W];
    if (W == 0u || F == 0u || i >= n_samples) return;           // (no face has weight: nothing is written)
    uint32_t r[4];
    sls_mesh_words(i, seed, r);
    const uint64_t t = sls_mesh_target(r, W);
    uint32_t lo = 0u, hi = F - 1u;                              // the first f with C[f] > t; t < W = C[F - 1]: it is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (C[mid] > t) hi = mid; else lo = mid + 1u;
    }
    const uint32_t i0 = (uint32_t)faces[3 * (size_t)lo], i1 = (uint32_t)faces[3 * (size_t)lo + 1], i2 = (uint32_t)faces[3 * (size_t)lo + 2];
    if (i0 >= V || i1 >= V || i2 >= V) return;                  // (never: a face with a bad index has weight 0 and is not found)
    float v0[3], v1[3], v2[3], p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v0[k] = vertices[3 * (size_t)i0 + k]; v1[k] = vertices[3 * (size_t)i1 + k]; v2[k] = vertices[3 * (size_t)i2 + k];
    }
    sls_mesh_point(r, v0, v1, v2, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) out_xyz[3 * (size_t)i + k] = p[k];
    if (out_face) out_face[i] = (int32_t)lo;
}

struct MeshScratch {
    unsigned long long *hdr, *C, *blk;
    double *area;
    size_t total;
    int nblk;
};

static MeshScratch mesh_layout(int F, void *base)
{
    MeshScratch s;
    Arena a(base);
    s.nblk = CloudChunks::count((size_t)F);
    s.hdr = a.take<unsigned long long>(8);
    s.area = a.take<double>((size_t)F);
    s.C = a.take<unsigned long long>((size_t)F);
    s.blk = a.take<unsigned long long>((size_t)s.nblk);
    s.total = a.off;
    return s;
}

// (the vertices and the samples need no scratch of their own: the size depends on F alone)
size_t mesh_sample_scratch_bytes(int V, int F, int n_samples)
{
    return (V >= 0 && F >= 0 && n_samples >= 0) ? mesh_layout(F, nullptr).total : 0;
}

int launch_mesh_sample(int V, const float *vertices, int F, const int32_t *faces, const float *crop_box, int n_samples,
                       uint64_t seed, float *out_xyz, int32_t *out_face, uint32_t *out_status, void *scratch, hipStream_t st)
{
    const MeshScratch s = mesh_layout(F, scratch);
    const uint32_t Fu = (uint32_t)F, nu = (uint32_t)n_samples;
    hipLaunchKernelGGL(mesh_init_kernel, dim3(1), dim3(64), 0, st, s.hdr);
    SLS_LAUNCH_CHECK("mesh_init_kernel");
    if (F > 0) {
        hipLaunchKernelGGL(mesh_area_kernel, grid_for((size_t)F, kCloudThreads), dim3(kCloudThreads), 0, st, V, F, vertices, faces, crop_box, s.area, s.hdr);
        SLS_LAUNCH_CHECK("mesh_area_kernel");
        hipLaunchKernelGGL(mesh_weight_sums_kernel, dim3(s.nblk), dim3(kCloudThreads), 0, st, Fu, (const double *)s.area,
                           (const unsigned long long *)s.hdr, s.blk);
        SLS_LAUNCH_CHECK("mesh_weight_sums_kernel");
    }
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kCloudThreads), 0, st, s.nblk, s.blk, s.hdr, nu, out_status);
    SLS_LAUNCH_CHECK("mesh_scan_kernel");
    if (F > 0) {
        hipLaunchKernelGGL(mesh_prefix_kernel, dim3(s.nblk), dim3(kCloudThreads), 0, st, Fu, (const double *)s.area,
                           (const unsigned long long *)s.hdr, (const unsigned long long *)s.blk, s.C);
        SLS_LAUNCH_CHECK("mesh_prefix_kernel");
        hipLaunchKernelGGL(mesh_sample_kernel, grid_for(nu, kCloudThreads), dim3(kCloudThreads), 0, st, (uint32_t)V,
                           Fu, vertices, faces, (const unsigned long long *)s.C, (const unsigned long long *)s.hdr, nu, seed, out_xyz,
                           out_face);
        SLS_LAUNCH_CHECK("mesh_sample_kernel");
    }
    return SLS_OK;
}

}  // namespace sls
