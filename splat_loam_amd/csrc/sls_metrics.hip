// sls_metrics.hip — what is made of an array of distances, unsigned (sls_nn_query's, sls_mesh_distance's squared ones) or
// signed (sls_mesh_signed_distance's): the counts and the float64 sum (sls_nn_stats, sls_signed_stats) and the error
// colours (sls_error_colors, sls_signed_error_colors).  One body each; the two flavours differ in the header function
// that judges an entry (include/sls_nn_math.h, sls_meshdist_math.h, sls_signdist_math.h).  Built EXACT.
//
// The stats: the entries that count, those of them that are flagged (below the threshold; negative) and the float64 sum of
// their values, in a FIXED order: block b of a grid that depends on M alone sums its entries b*256 + t, + grid*256, ... per
// thread, the 64 lanes by the xor butterfly 32 .. 1, the 4 waves in order; one block then adds the partials the same way,
// thread t the partials t, t + 256, ...  No atomics: the same bits every run, and tests/nn_ref.py (device_sum) restates
// them.  The order is the contract of both entry points.
#include "sls_launch.hpp"
#include "../../include/sls_nn_math.h"
#include "../../include/sls_meshdist_math.h"
#include "../../include/sls_signdist_math.h"

namespace sls {

constexpr int kNnStatsMaxBlocks = SLS_NN_STATS_SCRATCH_BYTES / 32;     // 32 bytes per partial: n, flagged, sum, pad

struct StatsPartial { unsigned long long n, flagged; double sum; };

// an entry's term: does it count and with which value (kept), and is a counted value flagged
struct NnStatsTerm {        // sls_nn_stats: the distance, below the threshold
    float truncation, threshold;
    int include_truncated;
    __device__ __forceinline__ int kept(float d2, float *value) const { return sls_nn_stats_term(d2, truncation, include_truncated, value); }
    __device__ __forceinline__ bool flag(float value) const { return value < threshold; }
};
struct SignedStatsTerm {    // sls_signed_stats: the signed distance, negative
    float truncation;
    __device__ __forceinline__ int kept(float sd, float *value) const { *value = sd; return sls_sd_stats_term(sd, truncation); }
    __device__ __forceinline__ bool flag(float value) const { return value < 0.0f; }
};

__device__ __forceinline__ StatsPartial stats_block_sum(StatsPartial v)
{   // valid in thread 0
    __shared__ unsigned long long s_n[4], s_b[4];
    __shared__ double s_s[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v.n += __shfl_xor(v.n, off, 64);
        v.flagged += __shfl_xor(v.flagged, off, 64);
        v.sum += __shfl_xor(v.sum, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_n[threadIdx.x >> 6] = v.n; s_b[threadIdx.x >> 6] = v.flagged; s_s[threadIdx.x >> 6] = v.sum; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) { v.n += s_n[w]; v.flagged += s_b[w]; v.sum += s_s[w]; }
    return v;
}

template <class Term>
__global__ __launch_bounds__(256) void stats_partial_kernel(int M, const float *__restrict__ in, Term term,
                                                            unsigned long long *__restrict__ partials)
{
    StatsPartial v = { 0ull, 0ull, 0.0 };
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)M; i += (size_t)gridDim.x * 256) {
        float value;
        if (term.kept(in[i], &value)) {
            v.n += 1ull;
            v.flagged += term.flag(value) ? 1ull : 0ull;
            v.sum += (double)value;
        }
    }
    v = stats_block_sum(v);
    if (threadIdx.x == 0) {
        partials[4 * blockIdx.x] = v.n;
        partials[4 * blockIdx.x + 1] = v.flagged;
        partials[4 * blockIdx.x + 2] = (unsigned long long)__double_as_longlong(v.sum);
    }
}

__global__ __launch_bounds__(256) void stats_final_kernel(int M, int nblocks, const unsigned long long *__restrict__ partials,
                                                          unsigned long long *__restrict__ out)
{
    StatsPartial v = { 0ull, 0ull, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        v.n += partials[4 * b];
        v.flagged += partials[4 * b + 1];
        v.sum += __longlong_as_double((long long)partials[4 * b + 2]);
    }
    v = stats_block_sum(v);
    if (threadIdx.x == 0) {
        out[0] = v.n;
        out[1] = v.flagged;
        out[2] = (unsigned long long)__double_as_longlong(v.sum);
        out[3] = (unsigned long long)M;
    }
}

// scratch: SLS_NN_STATS_SCRATCH_BYTES.  M == 0: the final kernel alone, which writes [0, 0, 0.0, 0]
template <class Term>
static int launch_stats(int M, const float *in, const Term &term, uint64_t *out_words, void *scratch, hipStream_t st)
{
    int nblocks = (M + 255) / 256;
    if (nblocks > kNnStatsMaxBlocks) nblocks = kNnStatsMaxBlocks;
    unsigned long long *partials = (unsigned long long *)scratch;
    if (nblocks > 0) {
        hipLaunchKernelGGL(stats_partial_kernel<Term>, dim3(nblocks), dim3(256), 0, st, M, in, term, partials);
        SLS_LAUNCH_CHECK("stats_partial_kernel");
    }
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(256), 0, st, M, nblocks, (const unsigned long long *)partials,
                       (unsigned long long *)out_words);
    SLS_LAUNCH_CHECK("stats_final_kernel");
    return SLS_OK;
}

int launch_nn_stats(int M, const float *dist2, float truncation, float threshold, int include_truncated, uint64_t *out_stats,
                    void *scratch, hipStream_t st)
{
    return launch_stats(M, dist2, NnStatsTerm{ truncation, threshold, include_truncated }, out_stats, scratch, st);
}

int launch_signed_stats(int M, const float *sdist, float truncation, uint64_t *out_words, void *scratch, hipStream_t st)
{
    return launch_stats(M, sdist, SignedStatsTerm{ truncation }, out_words, scratch, st);
}

// out_rgb[i] = Color(in[i], truncation)
template <void (*Color)(float, float, uint8_t *)>
__global__ __launch_bounds__(256) void colors_kernel(int M, const float *__restrict__ in, float truncation,
                                                     uint8_t *__restrict__ out_rgb)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M) return;
    uint8_t rgb[3];
    Color(in[i], truncation, rgb);
    out_rgb[3 * i] = rgb[0];
    out_rgb[3 * i + 1] = rgb[1];
    out_rgb[3 * i + 2] = rgb[2];
}

template <void (*Color)(float, float, uint8_t *)>
static int launch_colors(int M, const float *in, float truncation, uint8_t *out_rgb, hipStream_t st)
{
    if (M == 0) return SLS_OK;
    hipLaunchKernelGGL(colors_kernel<Color>, dim3((M + 255) / 256), dim3(256), 0, st, M, in, truncation, out_rgb);
    SLS_LAUNCH_CHECK("colors_kernel");
    return SLS_OK;
}

int launch_error_colors(int M, const float *dist2, float truncation, uint8_t *out_rgb, hipStream_t st)
{
    return launch_colors<sls_error_color>(M, dist2, truncation, out_rgb, st);
}

int launch_signed_error_colors(int M, const float *sdist, float truncation, uint8_t *out_rgb, hipStream_t st)
{
    return launch_colors<sls_signed_error_color>(M, sdist, truncation, out_rgb, st);
}

}  // namespace sls
