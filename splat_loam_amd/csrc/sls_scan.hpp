// sls_scan.hpp — what the device geometry ops (sls_cloud, sls_tsdf, sls_mesh, sls_simplify, sls_smooth, sls_fill, sls_outlier,
// sls_cluster) share of their scans.  block_scan / scan_in_place: workgroup-wide exclusive scans, wave scans of 64 lanes, then
// the wave sums through LDS.  Chunks<THREADS, PER>: the chunked layer on top — an array is cut into chunks of THREADS * PER positions,
// a workgroup per chunk, thread t owning PER consecutive positions — with the three launches of an ordered compaction:
//   total      every workgroup's sum of its threads' values (popc of a head or flag mask, or any integer sum) -> blk[chunk]
//   scan_totals  one workgroup: blk <- its exclusive scan, the caller's epilogue stores the grand total
//   rank       the values recomputed: blk[chunk] + the scan inside the workgroup = this thread's rank in the whole array
// and write_rows, the third launch's body where the compacted thing is a cloud: rows of xyz, normals and the row index.
// Integer types only (the order of the additions then does not matter).
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

// The chunk geometry and the per-chunk steps.  total / scan_totals / rank own their LDS wave array: one of them per kernel.
template <int THREADS, int PER>
struct Chunks {
    static constexpr int kThreads = THREADS, kPer = PER, kChunk = THREADS * PER;

    static int count(size_t n) { return (int)((n + kChunk - 1) / kChunk); }     // host: the chunks (= workgroups) of n positions
    static __device__ __forceinline__ uint32_t first() { return blockIdx.x * (uint32_t)kChunk + threadIdx.x * (uint32_t)PER; }

    // The head flags of the sorted positions p0 .. p0 + PER - 1 below n as a bit mask: a position whose key differs from its
    // predecessor's (position 0 has none and is a head).  key(p) loads the key of position p: any type with != and a value
    // initialisation.  A run of the key `reserved` has no head.
    template <bool RESERVED, typename Load, typename K>
    static __device__ __forceinline__ uint32_t head_mask_of(uint32_t n, uint32_t p0, Load key, K reserved)
    {
        uint32_t mask = 0u;
        if (p0 < n) {
            K prev = K();
            if (p0) prev = key(p0 - 1u);
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const uint32_t p = p0 + (uint32_t)j;
                if (p < n) {
                    const K k = key(p);
                    if ((p == 0u || k != prev) && (!RESERVED || k != reserved)) mask |= 1u << j;
                    prev = k;
                }
            }
        }
        return mask;
    }
    template <typename Load>
    static __device__ __forceinline__ uint32_t head_mask(uint32_t n, uint32_t p0, Load key)
    {
        return head_mask_of<false>(n, p0, key, decltype(key(0u))());
    }
    template <typename Load, typename K>
    static __device__ __forceinline__ uint32_t head_mask(uint32_t n, uint32_t p0, Load key, K reserved)
    {
        return head_mask_of<true>(n, p0, key, (decltype(key(0u)))reserved);
    }

    // the non-zero flags of the positions i0 .. i0 + PER - 1 below n as a bit mask
    static __device__ __forceinline__ uint32_t flag_mask(uint32_t n, const uint32_t *__restrict__ flag, uint32_t i0)
    {
        uint32_t mask = 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (i0 + (uint32_t)j < n && flag[i0 + (uint32_t)j]) mask |= 1u << j;
        return mask;
    }

    // blk[this chunk] <- the sum of v over the workgroup
    template <typename T>
    static __device__ __forceinline__ void total(T v, T *__restrict__ blk)
    {
        __shared__ T s_wave[THREADS / 64];
        T sum;
        block_scan<T, THREADS>(v, s_wave, &sum);
        if (threadIdx.x == 0) blk[blockIdx.x] = sum;
    }

    // one workgroup: out[0 .. nblk) <- the exclusive scan of the chunk totals in[0 .. nblk) (out may be in); returns their sum
    template <typename T>
    static __device__ __forceinline__ T scan_totals(const T *in, T *out, int nblk)
    {
        __shared__ T s_wave[THREADS / 64];
        return scan_in_place<T, THREADS>(in, out, nblk, s_wave);
    }

    // the sum of v over every thread in front of this one in the whole array (blk: the scanned chunk totals)
    template <typename T>
    static __device__ __forceinline__ T rank(T v, const T *__restrict__ blk)
    {
        __shared__ T s_wave[THREADS / 64];
        T sum;
        return blk[blockIdx.x] + block_scan<T, THREADS>(v, s_wave, &sum);
    }

    // The kept rows of a cloud in their order (mask: the keep flags of this thread's positions first() .. + PER - 1, blk: the
    // scanned chunk totals): row i goes to row rank(i) of out_xyz, out_normals and out_index, each written where it is given
    static __device__ __forceinline__ void write_rows(uint32_t mask, const uint32_t *__restrict__ blk, const float *__restrict__ xyz,
                                                      const float *__restrict__ normals, float *__restrict__ out_xyz,
                                                      float *__restrict__ out_normals, int32_t *__restrict__ out_index)
    {
        const uint32_t i0 = first();
        uint32_t id = rank((uint32_t)__popc(mask), blk);
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if ((mask >> j) & 1u) {                 // (id <= i < the rows of the cloud: the outputs hold as many)
                const size_t i = i0 + (uint32_t)j, o = id;
                if (out_xyz) { out_xyz[3 * o] = xyz[3 * i]; out_xyz[3 * o + 1] = xyz[3 * i + 1]; out_xyz[3 * o + 2] = xyz[3 * i + 2]; }
                if (out_normals) {
                    out_normals[3 * o] = normals[3 * i]; out_normals[3 * o + 1] = normals[3 * i + 1];
                    out_normals[3 * o + 2] = normals[3 * i + 2];
                }
                if (out_index) out_index[o] = (int32_t)i;
                ++id;
            }
    }
};

}  // namespace sls
