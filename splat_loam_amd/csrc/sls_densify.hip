// sls_densify.hip — Mapper.densify's draw on the device (sls_densify_draw): which candidate pixels become surfels.
//
// Weighted sampling without replacement as an exponential race (include/sls_draw_math.h): key = -ln(u) / w with u a
// pure function of (pixel, seed, draw index), the k smallest (key bits, pixel) are drawn and leave in ascending pixel
// order — the list nonzero() gave sls_densify_rows before.  Built EXACT (-ffp-contract=off): the keys are integers of
// the contract ("Deterministic integers"); tests/densify_draw_ref.py restates them in NumPy.
//
// Launches, ordered by the stream alone (no workgroup ever waits for another):
//   densify_weights_kernel (sls_consumer.hip, unchanged)   weights + [#candidates, max gradient, weight sum]
//   densify_keys_kernel                                    one key per pixel, whole grid
//   densify_select_kernel, ONE workgroup of 1024           k and the no-draw verdict -> status (+ pinned mirror, at
//       once: the host reads n_drawn while the selection runs), a 12 + 10 + 10 bit radix select of the k-th key
//       (LDS histograms, the keys stay in L2: <= 1 MB), the tie on the pixel index, an ordered compaction.
#include "sls_launch.hpp"
#include "../../include/sls_draw_math.h"

namespace sls {

constexpr int kSelThreads = 1024;
constexpr int kSelTile = 4 * kSelThreads;        // keys per compaction tile: one uint4 per thread
constexpr uint32_t kKeyInf = 0x7F800000u;

static inline size_t padded_keys(int H, int W)
{
    const size_t n = (size_t)H * (size_t)W;
    return (n + kSelTile - 1) / kSelTile * kSelTile;
}

size_t densify_draw_scratch_bytes(int H, int W) { return padded_keys(H, W) * sizeof(uint32_t); }

// keys[p] = bits of E(p) / w[p] at w > 0, +inf elsewhere and in the padding up to a whole compaction tile
__global__ __launch_bounds__(256) void densify_keys_kernel(uint32_t n, uint32_t n_pad, const float *__restrict__ w, uint64_t seed,
                                                           uint32_t draw_index, uint32_t *__restrict__ keys)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pad) return;
    uint32_t key = kKeyInf;
    if (p < n) {
        const float wp = w[p];
        if (wp > 0.0f) key = sls_draw_float_bits(sls_draw_key(wp, sls_draw_word(p, seed, draw_index)));
    }
    keys[p] = key;
}

// exclusive prefix of v over the 1024 threads in thread order; *total: the sum.  s_w: 16 words of LDS, free on return
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int j = 0; j < kSelThreads / 64; ++j) {
        const uint32_t t = s_w[j];
        before += j < wv ? t : 0u;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// One pass of the radix select: among the keys whose bits above `shift + bits` equal those of *s_prefix, the digit
// (key >> shift) & (2^bits - 1) that holds the (*s_rank)-th smallest (0-based); *s_prefix gains the digit, *s_rank
// becomes the rank inside it.  Non-candidates (+inf) never count: k <= #candidates, whose keys are all finite.
template <int SHIFT, int BITS>
__device__ __forceinline__ void select_pass(const uint4 *__restrict__ keys4, uint32_t n_vec, uint32_t *hist, uint32_t *s_w,
                                            uint32_t *s_prefix, uint32_t *s_rank)
{
    constexpr uint32_t kBins = 1u << BITS;
    constexpr uint32_t kPer = (kBins + kSelThreads - 1) / kSelThreads;       // bins per thread in the search
    constexpr uint32_t kAbove = (SHIFT + BITS >= 32) ? 0u : ~0u << ((SHIFT + BITS) & 31);
    for (uint32_t b = threadIdx.x; b < kBins; b += kSelThreads) hist[b] = 0u;
    __syncthreads();
    const uint32_t prefix = *s_prefix, rank = *s_rank;
    for (uint32_t i = threadIdx.x; i < n_vec; i += kSelThreads) {
        const uint4 q = keys4[i];
        const uint32_t k4[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k4[j] != kKeyInf && (k4[j] & kAbove) == prefix) atomicAdd(&hist[(k4[j] >> SHIFT) & (kBins - 1u)], 1u);
    }
    __syncthreads();
    uint32_t mine[kPer], sum = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t b = threadIdx.x * kPer + j;
        mine[j] = b < kBins ? hist[b] : 0u;
        sum += mine[j];
    }
    uint32_t total;
    uint32_t below = block_exclusive_scan(sum, s_w, &total);
    if (rank >= below && rank < below + sum) {          // exactly one thread
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            if (rank >= below && rank < below + mine[j]) {
                *s_prefix = prefix | ((threadIdx.x * kPer + j) << SHIFT);
                *s_rank = rank - below;
            }
            below += mine[j];
        }
    }
    __syncthreads();
}

// stats: [#candidates, max gradient bits, weight sum bits] on entry (densify_weights_kernel); on exit also
// [3] n_drawn, [4] k, [5] the k-th key's bits, [6] how many pixels of exactly that key are drawn, [7] 1.
__global__ __launch_bounds__(kSelThreads) void densify_select_kernel(uint32_t n_pad, double percentage, const uint32_t *__restrict__ keys,
                                                                     int64_t *__restrict__ pixels_out, uint32_t *stats,
                                                                     uint32_t *stats_mirror)
{
    __shared__ uint32_t hist[4096];
    __shared__ uint32_t s_w[kSelThreads / 64];
    __shared__ uint32_t s_prefix, s_rank, s_k;
    if (threadIdx.x == 0) {
        const uint32_t n_cand = stats[0];
        const float gmax = __uint_as_float(stats[1]), total = __uint_as_float(stats[2]);
        uint32_t k = (uint32_t)(percentage * (double)n_cand);
        if (k < 2u || !(gmax > 0.0f) || (double)total / (double)gmax <= 1e-5) k = 0u;      // slam_rules.densify_sample's rules
        stats[3] = k;
        stats[4] = (uint32_t)(percentage * (double)n_cand);
        stats[5] = 0u; stats[6] = 0u; stats[7] = 1u;
        if (stats_mirror) mirror_status_block(stats, stats_mirror);
        s_k = k; s_prefix = 0u; s_rank = k ? k - 1u : 0u;
    }
    __syncthreads();
    const uint32_t k = s_k;
    if (k == 0u) return;
    const uint4 *keys4 = reinterpret_cast<const uint4 *>(keys);
    const uint32_t n_vec = n_pad / 4u;
    select_pass<20, 12>(keys4, n_vec, hist, s_w, &s_prefix, &s_rank);
    select_pass<10, 10>(keys4, n_vec, hist, s_w, &s_prefix, &s_rank);
    select_pass<0, 10>(keys4, n_vec, hist, s_w, &s_prefix, &s_rank);
    const uint32_t T = s_prefix, ties = s_rank + 1u;      // the k-th key; the first `ties` pixels that carry it are drawn
    if (threadIdx.x == 0) { stats[5] = T; stats[6] = ties; }
    // ordered compaction: a drawn pixel's place = the drawn pixels before it = (#keys < T before it) + min(#keys == T before it, ties)
    uint32_t run_lt = 0u, run_eq = 0u;
    for (uint32_t base = 0u; base < n_pad; base += kSelTile) {
        const uint32_t p0 = base + 4u * threadIdx.x;
        const uint4 q = keys4[p0 / 4u];
        const uint32_t k4[4] = { q.x, q.y, q.z, q.w };
        uint32_t packed = 0u;                              // #less in the low half, #equal in the high half (<= 4096 each per tile)
#pragma unroll
        for (int j = 0; j < 4; ++j) packed += (k4[j] < T ? 1u : 0u) + (k4[j] == T ? 0x10000u : 0u);
        uint32_t total;
        const uint32_t before = block_exclusive_scan(packed, s_w, &total);
        uint32_t lt = run_lt + (before & 0xFFFFu), eq = run_eq + (before >> 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (place < k always — k finite keys exist, one per candidate; the test keeps a write inside the list whatever the keys)
            if (k4[j] < T) { const uint32_t at = lt + min(eq, ties); if (at < k) pixels_out[at] = (int64_t)(p0 + j); ++lt; }
            else if (k4[j] == T) { if (eq < ties && lt + eq < k) pixels_out[lt + eq] = (int64_t)(p0 + j); ++eq; }
        }
        run_lt += total & 0xFFFFu;
        run_eq += total >> 16;
        if (run_lt + min(run_eq, ties) >= k) break;        // (uniform: every thread holds the same totals)
    }
}

int launch_densify_draw(int H, int W, const float *depth, const uint8_t *valid, const float *alpha, float thr, double percentage,
                        uint64_t seed, uint32_t draw_index, float *w_out, int64_t *pixels_out, uint32_t *stats,
                        uint32_t *stats_mirror, void *scratch, hipStream_t st)
{
    const uint32_t n = (uint32_t)H * (uint32_t)W, n_pad = (uint32_t)padded_keys(H, W);
    uint32_t *keys = reinterpret_cast<uint32_t *>(scratch);
    const int rc = launch_densify_weights(H, W, depth, valid, alpha, thr, w_out, stats, st);
    if (rc != SLS_OK) return rc;
    hipLaunchKernelGGL(densify_keys_kernel, dim3(n_pad / 256u), dim3(256), 0, st, n, n_pad, w_out, seed, draw_index, keys);
    SLS_LAUNCH_CHECK("densify_keys_kernel");
    hipLaunchKernelGGL(densify_select_kernel, dim3(1), dim3(kSelThreads), 0, st, n_pad, percentage, keys, pixels_out, stats,
                       stats_mirror);
    SLS_LAUNCH_CHECK("densify_select_kernel");
    return SLS_OK;
}

}  // namespace sls
