// sls_scan.hpp — workgroup-wide exclusive scans shared by sls_cloud.hip and sls_tsdf.hip: wave scans of 64 lanes, then
// the wave sums through LDS.  Integer types only (the order of the additions then does not matter).
#pragma once
#include "sls_common.hpp"

namespace sls {

// exclusive scan of one value per thread over the workgroup's THREADS threads (one use per kernel: s_wave, THREADS / 64
// entries of LDS, is not protected against a second use); *total: the sum of all
template <typename T, int THREADS>
__device__ __forceinline__ T block_scan(T v, T *s_wave, T *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    T before = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < THREADS / 64; ++j) {
        const T t = s_wave[j];
        before += j < wv ? t : (T)0;
        tot += t;
    }
    *total = tot;
    return before + incl - v;
}

// One workgroup: out[0 .. n) <- the exclusive scan of in[0 .. n) (out may be in), thread t owning ceil(n / THREADS)
// consecutive entries; returns the total
template <typename T, int THREADS>
__device__ __forceinline__ T scan_in_place(const T *in, T *out, int n, T *s_wave)
{
    const int P = (n + THREADS - 1) / THREADS;
    const int i0 = min((int)threadIdx.x * P, n), i1 = min(i0 + P, n);
    T sum = 0;
    for (int i = i0; i < i1; ++i) sum += in[i];
    T total;
    T run = block_scan<T, THREADS>(sum, s_wave, &total);
    for (int i = i0; i < i1; ++i) { const T v = in[i]; out[i] = run; run += v; }
    return total;
}

}  // namespace sls
