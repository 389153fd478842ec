// sls_tsdf.hip — a sparse truncated signed distance volume on the device: which 8x8x8 blocks a point set names
// (sls_tsdf_blocks), one rendered keyframe fused into the volume (sls_tsdf_integrate) and the zero surface as a
// triangle soup by marching tetrahedra (sls_tsdf_extract_count / _emit).  include/sls_tsdf_math.h states the
// arithmetic, tests/tsdf_ref.py restates it in NumPy; DESIGN.md section 2, "TSDF volume", states the contract.
// Built EXACT (-ffp-contract=off): block keys, pixels and vertex bits are part of the contract.
//
// sls_tsdf_blocks, launches ordered by the stream alone:
//   tsdf_init / tsdf_keys       27 candidate keys per point (0 where the point names nothing), the identity permutation,
//                               the counts of non-finite and out-of-range points (integer atomics: order-free)
//   the stable LSD sort         63 key bits over (u64 key, u32 index) pairs (sls_radix.hip: radix_sort_pairs_u64)
//   tsdf_heads / _scan / _write head flags of the sorted keys (a non-zero key that differs from its predecessor), their
//                               scan in chunks of 2048 positions, the block coordinates and the status words
//
// sls_tsdf_integrate            one workgroup of 512 threads per block, thread l owns voxel l = slot 512 k + l: loads
//                               and stores of tsdf / weight coalesce, four planes of allmap are gathered at one pixel
//
// sls_tsdf_extract_count / _emit  one workgroup per block, thread l owns the cube at voxel l.  The seven +x/+y/+z
//                               neighbour blocks are found by bisection of the sorted block list, the 9^3 corner tile
//                               of tsdf / weight is staged in LDS (5832 B), a cube all of whose corners are observed
//                               runs sls_tsdf_cube.  count: the workgroup's sum -> counts[k]; tsdf_prefix: one workgroup
//                               scans counts -> prefix, the total -> status.  emit: the workgroup's exclusive scan of
//                               the cubes' counts (wave scans of 64 lanes, then the eight wave sums) fixes the position
//                               of every triangle: ascending block, cube, tetrahedron, triangle.  No atomics.
#include "sls_geom.hpp"
#include "sls_scan.hpp"
#include "../../include/sls_tsdf_math.h"

namespace sls {

constexpr int kTsdfThreads = SLS_TSDF_BLOCK_VOXELS;         // 512: a thread per voxel of a block
using TsdfChunks = Chunks<kTsdfThreads, 4>;                 // the head scan: chunks of 2048 sorted positions
constexpr int kTsdfTile = 9 * 9 * 9;

enum { TH_COUNT = 0, TH_NONFINITE = 1, TH_RANGE = 2 };      // hdr words of the block scratch

// ---------------------------------------------------------------------------------------------------------------------
// which blocks exist
// ---------------------------------------------------------------------------------------------------------------------
struct TsdfGrid { double origin[3], voxel_size; };

__global__ void tsdf_init_kernel(uint32_t *hdr, uint32_t n_keys)
{
    if (threadIdx.x < 8) hdr[threadIdx.x] = threadIdx.x == TH_COUNT ? n_keys : 0u;
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_keys_kernel(int M, const float *__restrict__ xyz, TsdfGrid g, double margin,
                                                                 uint32_t *hdr, uint64_t *__restrict__ keys,
                                                                 uint32_t *__restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * kTsdfThreads + threadIdx.x;
    bool nonfinite = false, range = false;
    if (i < (size_t)M) {
        const float p[3] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
        uint64_t k[SLS_TSDF_POINT_KEYS];
#pragma unroll
        for (int j = 0; j < SLS_TSDF_POINT_KEYS; ++j) k[j] = 0u;
        if (finite_f32(p[0]) && finite_f32(p[1]) && finite_f32(p[2])) range = !sls_tsdf_point_keys(p, g.origin, g.voxel_size, margin, k);
        else nonfinite = true;
#pragma unroll
        for (int j = 0; j < SLS_TSDF_POINT_KEYS; ++j) {
            keys[SLS_TSDF_POINT_KEYS * i + j] = k[j];
            vals[SLS_TSDF_POINT_KEYS * i + j] = (uint32_t)(SLS_TSDF_POINT_KEYS * i + j);
        }
    }
    const uint64_t mn = __ballot(nonfinite), mr = __ballot(range);
    if ((threadIdx.x & 63) == 0) {
        if (mn) atomicAdd(&hdr[TH_NONFINITE], (uint32_t)__popcll(mn));
        if (mr) atomicAdd(&hdr[TH_RANGE], (uint32_t)__popcll(mr));
    }
}

// the head flags of this thread's four consecutive sorted positions, as a bit mask (key 0: no block; the zeros sort to the front)
__device__ __forceinline__ uint32_t tsdf_head_mask(uint32_t n, const uint64_t *__restrict__ keys, uint32_t p0)
{
    return TsdfChunks::head_mask(n, p0, [&](uint32_t p) { return keys[p]; }, 0u);
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_heads_kernel(uint32_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ blk)
{
    TsdfChunks::total((uint32_t)__popc(tsdf_head_mask(n, keys, TsdfChunks::first())), blk);
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_scan_kernel(int nblk, uint32_t *__restrict__ blk, const uint32_t *__restrict__ hdr,
                                                                 uint32_t *__restrict__ status)
{
    const uint32_t nb = TsdfChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) {
        status[0] = nb; status[1] = hdr[TH_NONFINITE]; status[2] = hdr[TH_RANGE]; status[3] = 1u;
    }
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_write_kernel(uint32_t n, const uint64_t *__restrict__ keys,
                                                                  const uint32_t *__restrict__ blk, uint32_t capacity,
                                                                  int32_t *__restrict__ out_blocks)
{
    const uint32_t p0 = TsdfChunks::first();
    const uint32_t mask = tsdf_head_mask(n, keys, p0);
    uint32_t id = TsdfChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < TsdfChunks::kPer; ++j)
        if ((mask >> j) & 1u) {
            if (id < capacity) {
                int32_t b[3];
                sls_tsdf_key_block(keys[p0 + (uint32_t)j], b);
                out_blocks[3 * (size_t)id] = b[0]; out_blocks[3 * (size_t)id + 1] = b[1]; out_blocks[3 * (size_t)id + 2] = b[2];
            }
            ++id;
        }
}

// scratch layout (all 256-byte aligned)
struct TsdfBlockScratch {
    uint32_t *hdr;
    uint64_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp, *blk;
    void *sort;
    size_t sort_bytes, total;
    int nblk;
};

static TsdfBlockScratch tsdf_block_layout(int M, void *base)
{
    TsdfBlockScratch s;
    Arena a(base);
    const size_t n = SLS_TSDF_POINT_KEYS * (size_t)M;
    s.nblk = TsdfChunks::count(n);
    s.hdr = a.take<uint32_t>(16);
    s.keys = a.take<uint64_t>(n);
    s.keys_tmp = a.take<uint64_t>(n);
    s.vals = a.take<uint32_t>(n);
    s.vals_tmp = a.take<uint32_t>(n);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.sort_bytes = sort_scratch_bytes((uint64_t)n);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t tsdf_blocks_scratch_bytes(int M) { return (M > 0 && M <= SLS_TSDF_MAX_POINTS) ? tsdf_block_layout(M, nullptr).total : 0; }

int launch_tsdf_blocks(int M, const float *xyz, double voxel_size, double trunc, const double *origin, int capacity,
                       int32_t *out_blocks, uint32_t *out_status, void *scratch, hipStream_t st)
{
    const TsdfBlockScratch s = tsdf_block_layout(M, scratch);
    const uint32_t n = (uint32_t)SLS_TSDF_POINT_KEYS * (uint32_t)M;
    TsdfGrid g;
    g.origin[0] = origin[0]; g.origin[1] = origin[1]; g.origin[2] = origin[2]; g.voxel_size = voxel_size;
    hipLaunchKernelGGL(tsdf_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, n);
    SLS_LAUNCH_CHECK("tsdf_init_kernel");
    hipLaunchKernelGGL(tsdf_keys_kernel, grid_for((size_t)M, kTsdfThreads), dim3(kTsdfThreads), 0, st, M, xyz, g,
                       trunc + voxel_size, s.hdr, s.keys, s.vals);
    SLS_LAUNCH_CHECK("tsdf_keys_kernel");
    int which = 0;
    int rc = radix_sort_pairs_u64(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + TH_COUNT, n, SLS_TSDF_KEY_BITS, s.sort,
                                  s.sort_bytes, &which, st);
    if (rc) return rc;
    const uint64_t *keys = which ? s.keys_tmp : s.keys;
    hipLaunchKernelGGL(tsdf_heads_kernel, dim3(s.nblk), dim3(kTsdfThreads), 0, st, n, keys, s.blk);
    SLS_LAUNCH_CHECK("tsdf_heads_kernel");
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(kTsdfThreads), 0, st, s.nblk, s.blk, (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("tsdf_scan_kernel");
    hipLaunchKernelGGL(tsdf_write_kernel, dim3(s.nblk), dim3(kTsdfThreads), 0, st, n, keys, (const uint32_t *)s.blk,
                       (uint32_t)capacity, out_blocks);
    SLS_LAUNCH_CHECK("tsdf_write_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// one keyframe into the volume
// ---------------------------------------------------------------------------------------------------------------------
struct TsdfIntegrateArgs {
    int H, W, wrap;
    float fx, fy, cx, cy, near_cut;
    float R[9], t[3];
    float min_opacity, max_depth_dist, depth_ratio, trunc;
    TsdfGrid g;
    const int32_t *blocks;
    const float *allmap;
    float *tsdf, *weight;
};

__global__ __launch_bounds__(kTsdfThreads) void tsdf_integrate_kernel(TsdfIntegrateArgs a)
{
    const int k = blockIdx.x;                       // (the grid is B workgroups)
    const int l = threadIdx.x;
    const int32_t bx = a.blocks[3 * (size_t)k], by = a.blocks[3 * (size_t)k + 1], bz = a.blocks[3 * (size_t)k + 2];
    float c[3], q[3];
    c[0] = sls_tsdf_centre(8 * bx + (l & 7), a.g.origin[0], a.g.voxel_size);
    c[1] = sls_tsdf_centre(8 * by + ((l >> 3) & 7), a.g.origin[1], a.g.voxel_size);
    c[2] = sls_tsdf_centre(8 * bz + (l >> 6), a.g.origin[2], a.g.voxel_size);
    const float rho = sls_tsdf_view(a.R, a.t, c, q);
    if (!(rho >= a.near_cut) || !(rho > 0.0f) || !(rho <= FLT_MAX)) return;
    const int32_t px = sls_tsdf_pixel(q, rho, a.fx, a.fy, a.cx, a.cy, a.H, a.W, a.wrap);
    const size_t P = (size_t)a.H * (size_t)a.W;
    if (px < 0 || (size_t)px >= P) return;
    const float D = a.allmap[SLS_CH_DEPTH * P + px], al = a.allmap[SLS_CH_ALPHA * P + px];
    const float med = a.allmap[SLS_CH_MEDIAN * P + px], dist = a.allmap[SLS_CH_DIST * P + px];
    const size_t slot = (size_t)k * SLS_TSDF_BLOCK_VOXELS + l;
    float tv = a.tsdf[slot], w = a.weight[slot];
    if (sls_tsdf_update(D, al, med, dist, rho, a.min_opacity, a.max_depth_dist, a.depth_ratio, a.trunc, &tv, &w)) {
        a.tsdf[slot] = tv;
        a.weight[slot] = w;
    }
}

int launch_tsdf_integrate(const SlsCamera &cam, int B, const int32_t *blocks, float *tsdf, float *weight, const float *allmap,
                          double voxel_size, double trunc, const double *origin, float min_opacity, float max_depth_dist,
                          float depth_ratio, hipStream_t st)
{
    TsdfIntegrateArgs a;
    a.H = cam.H; a.W = cam.W; a.wrap = cam.wrap;
    a.fx = cam.fx; a.fy = cam.fy; a.cx = cam.cx; a.cy = cam.cy; a.near_cut = cam.near_cut;
    for (int i = 0; i < 9; ++i) a.R[i] = cam.Rvw[i];
    for (int i = 0; i < 3; ++i) { a.t[i] = cam.tvw[i]; a.g.origin[i] = origin[i]; }
    a.g.voxel_size = voxel_size;
    a.min_opacity = min_opacity; a.max_depth_dist = max_depth_dist; a.depth_ratio = depth_ratio; a.trunc = (float)trunc;
    a.blocks = blocks; a.allmap = allmap; a.tsdf = tsdf; a.weight = weight;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(B), dim3(kTsdfThreads), 0, st, a);
    SLS_LAUNCH_CHECK("tsdf_integrate_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the zero surface
// ---------------------------------------------------------------------------------------------------------------------
struct TsdfExtractArgs {
    int B;
    float min_weight;
    TsdfGrid g;
    const int32_t *blocks;
    const float *tsdf, *weight;
};

// index of block (bx, by, bz) in the sorted list, -1 when it is absent
__device__ __forceinline__ int tsdf_find_block(int B, const int32_t *__restrict__ blocks, int32_t bx, int32_t by, int32_t bz)
{
    const uint64_t want = sls_tsdf_key(bx, by, bz);
    int lo = 0, hi = B;                             // the first k with key(k) >= want lies in [lo, hi]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const uint64_t key = sls_tsdf_key(blocks[3 * (size_t)mid], blocks[3 * (size_t)mid + 1], blocks[3 * (size_t)mid + 2]);
        if (key < want) lo = mid + 1; else hi = mid;
    }
    if (lo >= B) return -1;
    return (blocks[3 * (size_t)lo] == bx && blocks[3 * (size_t)lo + 1] == by && blocks[3 * (size_t)lo + 2] == bz) ? lo : -1;
}

// Stages the 9^3 corner tile of block k (every thread of the workgroup must call this: it synchronises), then hands this
// thread's cube its eight corner values f and the centres c0 / c1 of the global voxel coordinates g and g + 1.  Returns
// whether all eight corners are observed.
__device__ __forceinline__ bool tsdf_cube_corners(const TsdfExtractArgs &a, int k, float *s_t, float *s_w, int *s_nb, float f[8],
                                                  float c0[3], float c1[3])
{
    const int l = threadIdx.x;
    const int32_t bx = a.blocks[3 * (size_t)k], by = a.blocks[3 * (size_t)k + 1], bz = a.blocks[3 * (size_t)k + 2];
    if (l < 8) s_nb[l] = l == 0 ? k : tsdf_find_block(a.B, a.blocks, bx + (l & 1), by + ((l >> 1) & 1), bz + (l >> 2));
    __syncthreads();
    for (int i = l; i < kTsdfTile; i += kTsdfThreads) {
        const int x = i % 9, y = (i / 9) % 9, z = i / 81;
        const int nb = s_nb[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
        float t = 0.0f, w = -1.0f;                  // an absent block: unobserved corners
        if (nb >= 0) {
            const size_t slot = (size_t)nb * SLS_TSDF_BLOCK_VOXELS + ((x & 7) | ((y & 7) << 3) | ((z & 7) << 6));
            t = a.tsdf[slot]; w = a.weight[slot];
        }
        s_t[i] = t; s_w[i] = w;
    }
    __syncthreads();
    const int x = l & 7, y = (l >> 3) & 7, z = l >> 6;
    bool observed = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = (x + (j & 1)) + 9 * (y + ((j >> 1) & 1)) + 81 * (z + (j >> 2));
        f[j] = s_t[i];
        observed = observed && (s_w[i] >= a.min_weight) && (f[j] == f[j]);     // (a NaN weight or value: unobserved)
    }
    const int32_t g[3] = { 8 * bx + x, 8 * by + y, 8 * bz + z };
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        c0[d] = sls_tsdf_centre(g[d], a.g.origin[d], a.g.voxel_size);
        c1[d] = sls_tsdf_centre(g[d] + 1, a.g.origin[d], a.g.voxel_size);
    }
    return observed;
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_count_kernel(TsdfExtractArgs a, uint32_t *__restrict__ counts)
{
    __shared__ float s_t[kTsdfTile], s_w[kTsdfTile];
    __shared__ int s_nb[8];
    float f[8], c0[3], c1[3];
    const bool observed = tsdf_cube_corners(a, (int)blockIdx.x, s_t, s_w, s_nb, f, c0, c1);
    TsdfChunks::total(observed ? (uint32_t)sls_tsdf_cube(f, c0, c1, nullptr) : 0u, counts);
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_prefix_kernel(int B, const uint32_t *__restrict__ counts, uint32_t *__restrict__ prefix,
                                                                   uint32_t *__restrict__ status)
{
    const uint32_t total = TsdfChunks::scan_totals(counts, prefix, B);
    if (threadIdx.x == 0) { status[0] = total; status[1] = (uint32_t)B; status[2] = 0u; status[3] = 1u; }
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_emit_kernel(TsdfExtractArgs a, const uint32_t *__restrict__ prefix, uint32_t T,
                                                                 float *__restrict__ triangles)
{
    __shared__ float s_t[kTsdfTile], s_w[kTsdfTile];
    __shared__ int s_nb[8];
    float f[8], c0[3], c1[3];
    const bool observed = tsdf_cube_corners(a, (int)blockIdx.x, s_t, s_w, s_nb, f, c0, c1);
    const uint32_t n = observed ? (uint32_t)sls_tsdf_cube(f, c0, c1, nullptr) : 0u;
    const uint32_t pos = TsdfChunks::rank(n, prefix);
    if (n == 0u || pos >= T || n > T - pos) return;     // (never past the array the caller sized from the count call)
    sls_tsdf_cube(f, c0, c1, triangles + 9 * (size_t)pos);
}

int launch_tsdf_extract_count(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                              uint32_t *counts, uint32_t *prefix, uint32_t *status, hipStream_t st)
{
    TsdfExtractArgs a;
    a.B = B; a.min_weight = min_weight; a.blocks = blocks; a.tsdf = tsdf; a.weight = weight;
    a.g.origin[0] = a.g.origin[1] = a.g.origin[2] = 0.0; a.g.voxel_size = 1.0;       // (positions play no part in the count)
    if (B > 0) {
        hipLaunchKernelGGL(tsdf_count_kernel, dim3(B), dim3(kTsdfThreads), 0, st, a, counts);
        SLS_LAUNCH_CHECK("tsdf_count_kernel");
    }
    hipLaunchKernelGGL(tsdf_prefix_kernel, dim3(1), dim3(kTsdfThreads), 0, st, B, (const uint32_t *)counts, prefix, status);
    SLS_LAUNCH_CHECK("tsdf_prefix_kernel");
    return SLS_OK;
}

int launch_tsdf_extract_emit(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight,
                             double voxel_size, const double *origin, const uint32_t *prefix, uint32_t T, float *triangles,
                             hipStream_t st)
{
    TsdfExtractArgs a;
    a.B = B; a.min_weight = min_weight; a.blocks = blocks; a.tsdf = tsdf; a.weight = weight;
    for (int i = 0; i < 3; ++i) a.g.origin[i] = origin[i];
    a.g.voxel_size = voxel_size;
    hipLaunchKernelGGL(tsdf_emit_kernel, dim3(B), dim3(kTsdfThreads), 0, st, a, prefix, T, triangles);
    SLS_LAUNCH_CHECK("tsdf_emit_kernel");
    return SLS_OK;
}

}  // namespace sls
