// sls_surface.hip — oriented surface points sampled from a rendered keyframe (sls_surface_samples): steps 3-4 of the
// reference's mesh_poisson (scene/postprocessing.py:164-188) without its boolean gather, its two host copies and its
// unseeded np.random.choice.  DESIGN.md section 2, "Surface samples", states the contract; tests/surface_ref.py
// restates it in NumPy.  Built EXACT (-ffp-contract=off): the selected pixels are integers of the contract.
//
//   valid(p) = !(alpha < min_opacity) && !(dist > max_depth_dist)                      planes 1 and 6 of allmap
//   sample j = the valid pixel of rank floor(r_j n_valid / 2^32) in row-major order,  r_j = sls_sample_word(j, seed, frame_id)
//   point    = M (depth ray),  depth = (1 - ratio) D/alpha + ratio median,  ray at (c - .5, r - .5)
//   normal   = R(M) (N / alpha)                                                        (alpha > 0; as they are elsewhere)
//
// Launches, ordered by the stream alone (no workgroup ever waits for another):
//   surface_valid_kernel    one 64-bit validity word per wave (__ballot), bits past the image clear: H W / 64 words,
//                           at most 4096 = 32 KB.  Reads 2 planes (8 B per pixel), writes 1/8 B per pixel.
//   surface_sample_kernel   ceil(n_samples / 256) workgroups.  Each scans the words' popcounts itself (4096 counts ->
//                           16 KB of exclusive prefix in LDS; 32 KB read from L2 per workgroup), so nobody depends on
//                           another workgroup's result; workgroup 0 writes the status.  A thread then draws its rank,
//                           bisects the prefix for the word, picks the rank-th set bit, gathers the seven planes at
//                           that one pixel (28 B) and writes its two rows (24 B) and its pixel (4 B).
#include "sls_launch.hpp"
#include "../../include/sls_draw_math.h"

namespace sls {

constexpr int kSurfThreads = 256;
constexpr int kSurfMaxWords = SLS_SURFACE_MAX_PIXELS / 64;           // 4096
constexpr int kSurfPer = kSurfMaxWords / kSurfThreads;               // words per thread in the scan: 16

static inline uint32_t surface_words(int H, int W) { return (uint32_t)(((size_t)H * (size_t)W + 63) / 64); }

size_t surface_scratch_bytes(int H, int W) { return (size_t)surface_words(H, W) * sizeof(uint64_t); }

__global__ __launch_bounds__(kSurfThreads) void surface_valid_kernel(uint32_t n, const float *__restrict__ alpha, const float *__restrict__ dist,
                                                                     float min_opacity, float max_depth_dist, uint64_t *__restrict__ words)
{
    const uint32_t p = blockIdx.x * (uint32_t)kSurfThreads + threadIdx.x;      // (the grid covers whole words: ceil(n / 64) of them)
    bool ok = false;
    if (p < n) ok = !(alpha[p] < min_opacity) && !(dist[p] > max_depth_dist);    // (a NaN alpha stays valid, as in invalid_mask)
    const uint64_t word = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && p < n) words[p >> 6] = word;
}

// position of the rank-th (0-based) set bit of x; rank < popcount(x)
__device__ __forceinline__ uint32_t select_bit(uint64_t x, uint32_t rank)
{
    uint32_t pos = 0u;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t below = (uint32_t)__popcll((x >> pos) & ((1ull << s) - 1ull));
        if (rank >= below) { rank -= below; pos += (uint32_t)s; }
    }
    return pos;
}

struct SurfaceArgs {
    uint32_t n, n_words, W, n_samples;
    float depth_ratio;
    uint64_t seed;
    uint32_t frame_id;
    const float *allmap;
    const float2 *col_h, *row_h;
    const float *M;                  // 3x4 row-major
    const uint64_t *words;
    float *points, *normals;
    int32_t *pixels;                 // optional
    uint32_t *status;
};

__global__ __launch_bounds__(kSurfThreads) void surface_sample_kernel(SurfaceArgs a)
{
    __shared__ uint32_t s_prefix[kSurfMaxWords];      // exclusive prefix of the words' popcounts
    __shared__ uint32_t s_w[kSurfThreads / 64];
    // this thread's run of words, their counts and the workgroup-wide scan of the runs' sums
    const uint32_t w0 = threadIdx.x * (uint32_t)kSurfPer;
    uint32_t cnt[kSurfPer], sum = 0u;
#pragma unroll
    for (int j = 0; j < kSurfPer; ++j) {
        const uint32_t w = w0 + (uint32_t)j;
        cnt[j] = w < a.n_words ? (uint32_t)__popcll(a.words[w]) : 0u;
        sum += cnt[j];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t before = 0u, n_valid = 0u;
#pragma unroll
    for (int j = 0; j < kSurfThreads / 64; ++j) {
        const uint32_t t = s_w[j];
        before += j < wv ? t : 0u;
        n_valid += t;
    }
    uint32_t run = before + incl - sum;
#pragma unroll
    for (int j = 0; j < kSurfPer; ++j) { s_prefix[w0 + j] = run; run += cnt[j]; }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.status[0] = n_valid; a.status[1] = n_valid ? a.n_samples : 0u; a.status[2] = 0u; a.status[3] = 1u;
    }
    const uint32_t j = blockIdx.x * (uint32_t)kSurfThreads + threadIdx.x;
    if (n_valid == 0u || j >= a.n_samples) return;     // (an empty keyframe writes no row)
    const uint32_t idx = sls_sample_index(sls_sample_word(j, a.seed, a.frame_id), n_valid);
    // the last word whose prefix is <= idx: it is not empty (the next prefix is larger) and holds the idx-th valid pixel
    uint32_t lo = 0u, hi = a.n_words;                   // invariant: s_prefix[lo] <= idx, the answer is in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_prefix[mid] <= idx) lo = mid; else hi = mid;
    }
    const uint64_t word = a.words[lo];
    const uint32_t rank = idx - s_prefix[lo];
    if (rank >= (uint32_t)__popcll(word)) return;       // (never: idx < n_valid = the sum of the counts; keeps every index inside the image)
    const uint32_t px = lo * 64u + select_bit(word, rank);
    if (px >= a.n) return;                              // (never: the bits past the image are clear)
    const uint32_t r = px / a.W, c = px - r * a.W;
    const size_t P = a.n;
    const float D = a.allmap[SLS_CH_DEPTH * P + px], al = a.allmap[SLS_CH_ALPHA * P + px];
    const float N0 = a.allmap[(SLS_CH_NORMAL + 0) * P + px], N1 = a.allmap[(SLS_CH_NORMAL + 1) * P + px],
                N2 = a.allmap[(SLS_CH_NORMAL + 2) * P + px];
    const float med = a.allmap[SLS_CH_MEDIAN * P + px];
    const bool hit = al > 0.0f;
    const float Dh = hit ? D / al : D;
    const float s = Dh * (1.0f - a.depth_ratio) + med * a.depth_ratio;        // (surf_depth_of, sls_consumer_dev.hpp)
    const float2 cc = a.col_h[c], rr = a.row_h[r];
    const float x = s * cc.x * rr.x, y = s * cc.y * rr.x, z = s * rr.y;       // (surf_point's products)
    const float n0 = hit ? N0 / al : N0, n1 = hit ? N1 / al : N1, n2 = hit ? N2 / al : N2;
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = a.M[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.points[3 * (size_t)j + k] = ((m[4 * k + 0] * x + m[4 * k + 1] * y) + m[4 * k + 2] * z) + m[4 * k + 3];
        a.normals[3 * (size_t)j + k] = (m[4 * k + 0] * n0 + m[4 * k + 1] * n1) + m[4 * k + 2] * n2;
    }
    if (a.pixels) a.pixels[j] = (int32_t)px;
}

int launch_surface_samples(int H, int W, const float *allmap, const float *col_h, const float *row_h, const float *M,
                           float min_opacity, float max_depth_dist, float depth_ratio, int n_samples, uint64_t seed,
                           uint32_t frame_id, float *points, float *normals, int32_t *pixels, uint32_t *status, void *scratch,
                           hipStream_t st)
{
    const uint32_t n = (uint32_t)H * (uint32_t)W, n_words = surface_words(H, W);
    uint64_t *words = reinterpret_cast<uint64_t *>(scratch);
    hipLaunchKernelGGL(surface_valid_kernel, dim3((n_words * 64u + kSurfThreads - 1) / kSurfThreads), dim3(kSurfThreads), 0, st, n,
                       allmap + (size_t)SLS_CH_ALPHA * n, allmap + (size_t)SLS_CH_DIST * n, min_opacity, max_depth_dist, words);
    SLS_LAUNCH_CHECK("surface_valid_kernel");
    SurfaceArgs a;
    a.n = n; a.n_words = n_words; a.W = (uint32_t)W; a.n_samples = (uint32_t)n_samples;
    a.depth_ratio = depth_ratio; a.seed = seed; a.frame_id = frame_id;
    a.allmap = allmap; a.col_h = (const float2 *)col_h; a.row_h = (const float2 *)row_h; a.M = M; a.words = words;
    a.points = points; a.normals = normals; a.pixels = pixels; a.status = status;
    hipLaunchKernelGGL(surface_sample_kernel, dim3(((uint32_t)n_samples + kSurfThreads - 1) / kSurfThreads), dim3(kSurfThreads), 0, st, a);
    SLS_LAUNCH_CHECK("surface_sample_kernel");
    return SLS_OK;
}

}  // namespace sls
