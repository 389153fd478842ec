// sls_radix.hip — the project's radix sorter: stable LSD sort of (key, u32 value) pairs, 32- or 64-bit keys.  The
// rasterizer's depth order and tile sort (sls_sort.hip) and every geometry op (weld, clusters, simplify, adjacency,
// fill, voxel, TSDF blocks, Poisson, ground, the NN index, ICP) call it through the functions of sls_launch.hpp.
//
// Radix sort building block (wave64-native, no vendor library):
//   * 8..11-bit digits (sort_plan); the unit of work is ONE WAVE owning kSortWaveItems =
//     1024 consecutive items (16 rounds of 64): no workgroup barrier inside a pass, each
//     wave keeps its 2^BITS running bucket cursors in a private LDS slice; a workgroup is
//     SortBlock<BITS>::kWaves waves (8 up to 10-bit digits, 4 for 11) so that the count
//     table is written and read back in runs of that many chunks per digit;
//   * stable ranking inside a round by BITS ballots (the set of lanes holding my
//     digit), rank = popcount(peers below me): wave_digit_rank, sls_common.hpp;
//   * per pass: histogram -> per-digit row scan over chunks -> scatter;
//   * the item count is read from DEVICE memory (count_ptr), grids are sized for
//     a host-side capacity, so a whole iteration can be enqueued without a
//     device->host sync (sls_mapping_step).
#include "sls_common.hpp"
#include "sls_launch.hpp"

namespace sls {

// (build-time knobs for A/B runs; measured on the bench scene, A/B inside one box, iteration time with
//  rounds x waves per block = 16x16: 0.2652 ms, 16x8: 0.2613 (scatter 18.6 -> 15.8 us: twice the workgroups for
//  the 1260 wave chunks of the tile sort), 16x4: 0.266 (the stray-word table access), 24x8: 0.2618, 32x8: 0.264,
//  8x16: 0.268 and 8x8: 0.269 (row scan +4 us), 4x16: 0.280)
#ifndef SLS_SORT_ROUNDS
#define SLS_SORT_ROUNDS 16
#endif
#ifndef SLS_SORT_WAVES
#define SLS_SORT_WAVES 8
#endif
constexpr int kSortRounds = SLS_SORT_ROUNDS;
constexpr int kSortWaveItems = kWave * kSortRounds;  // 1024 items per wave

// ---------------------------------------------------------------------------
// step 1 of a pass: per-wave-chunk digit histogram -> cnt[digit][chunk]
// ---------------------------------------------------------------------------
// A block is WAVES chunks: the count table cnt[digit][chunk] is written (and read back by the scatter)
// in runs of WAVES consecutive chunks per digit — 32 contiguous bytes with 8 waves — instead of one
// stray word per (digit, wave).  The LDS rows are padded by one word so that the transposed access
// (lanes = consecutive waves of one digit) spreads over the banks.
template <int BITS> struct SortBlock { static constexpr int kWaves = BITS <= 9 ? SLS_SORT_WAVES : (BITS == 10 ? (SLS_SORT_WAVES < 8 ? SLS_SORT_WAVES : 8) : 4); };

template <typename KeyT, int BITS>
__global__ __launch_bounds__(64 * SortBlock<BITS>::kWaves) void sort_hist_kernel(
    const KeyT *__restrict__ keys, const uint32_t *__restrict__ count_ptr, uint32_t cap, int shift,
    uint32_t *__restrict__ cnt, int nchunks_cap)
{
    constexpr int BINS = 1 << BITS, WAVES = SortBlock<BITS>::kWaves, STR = BINS + 1;
    __shared__ uint32_t s_hist[WAVES * STR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk0 = blockIdx.x * WAVES, chunk = chunk0 + wave;
    const uint32_t R = load_count(count_ptr, cap);
    const int nchunks = (int)((R + kSortWaveItems - 1) / kSortWaveItems);
    if (chunk0 >= nchunks) return;             // whole block beyond the data
#pragma unroll
    for (int k = 0; k < BINS / 64; ++k) s_hist[wave * STR + lane + 64 * k] = 0;
    __builtin_amdgcn_wave_barrier();
    if (chunk < nchunks) {
        const uint32_t base = (uint32_t)chunk * kSortWaveItems + lane;
        KeyT k[kSortRounds];
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) k[r] = keys[min(base + (uint32_t)r * 64, R - 1u)];   // (chunk < nchunks: R >= 1)
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) {
            const uint32_t idx = base + (uint32_t)r * 64;
            if (idx < R) atomicAdd(&s_hist[wave * STR + ((uint32_t)(k[r] >> shift) & (uint32_t)(BINS - 1))], 1u);
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < BINS * WAVES; idx += 64 * WAVES) {
        const int d = idx / WAVES, w = idx % WAVES;
        if (chunk0 + w < nchunks_cap) cnt[(size_t)d * nchunks_cap + chunk0 + w] = s_hist[w * STR + d];
    }
}

// step 2: block d scans row d of cnt[][] exclusively in place, writes the row total.
// Thread t owns P = ceil(nchunks / 256) CONSECUTIVE entries: one pass to sum them, one wave scan + one barrier for
// the 256 partial sums, one pass to write the running prefix (a loop over 256-entry slabs with two barriers each
// cost 2 us more on the 1260-chunk rows of the tile sort: the kernel is nothing but its chain of latencies).
// nchunks_fixed > 0: the rows have that many entries (chunks of the emission, see emit_tiles_kernel)
__global__ __launch_bounds__(256) void sort_rowscan_kernel(uint32_t *__restrict__ cnt,
                                                           const uint32_t *__restrict__ count_ptr, uint32_t cap,
                                                           int nchunks_cap, uint32_t *__restrict__ totals,
                                                           int nchunks_fixed)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t R = nchunks_fixed > 0 ? 0u : load_count(count_ptr, cap);
    const int nchunks = nchunks_fixed > 0 ? nchunks_fixed : (int)((R + kSortWaveItems - 1) / kSortWaveItems);
    uint32_t *row = cnt + (size_t)blockIdx.x * nchunks_cap;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = (nchunks + 255) / 256, i0 = (int)threadIdx.x * P, i1 = min(i0 + P, nchunks);
    constexpr int kKeep = 8;                 // entries kept in registers between the two passes (P <= 8 up to 2 M items)
    uint32_t keep[kKeep];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kKeep; ++j) { keep[j] = (i0 + j < i1) ? row[i0 + j] : 0u; sum += keep[j]; }
    for (int i = i0 + kKeep; i < i1; ++i) sum += row[i];
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
#pragma unroll
    for (int j = 0; j < kKeep; ++j) {
        if (i0 + j < i1) row[i0 + j] = run;
        run += keep[j];
    }
    for (int i = i0 + kKeep; i < i1; ++i) { const uint32_t v = row[i]; row[i] = run; run += v; }
    if (threadIdx.x == 255) totals[blockIdx.x] = run;
}

// ---------------------------------------------------------------------------
// step 3: stable scatter.  Two kernels — fixed 1024-item chunks, the emission's chunks — that differ in where a wave's
// items begin and end; what follows is what both do, each part written once.
// ---------------------------------------------------------------------------
// (The loads stay in the kernels, where each requests them.  The rows of the count table too, though both kernels
//  spell that loop alike: moved into a function it compiled to 20 VGPRs more at 11-bit digits and a wave less per
//  SIMD at 9 and 10.)
// exclusive scan of the BINS digit totals (PER consecutive ones per thread, first 256 threads) into s_digit_base;
// every thread of the workgroup, two barriers
template <int BITS>
__device__ __forceinline__ void scatter_digit_bases(const uint32_t (&tot)[(1 << BITS) / 256], uint32_t *s_wave,
                                                    uint32_t *s_digit_base, uint2 *ranges_out, int nranges)
{
    constexpr int PER = (1 << BITS) / 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool scanner = threadIdx.x < 256;
    uint32_t loc[PER];
    uint32_t sum = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { loc[q] = sum; sum += tot[q]; }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (scanner && lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (scanner) {
        uint32_t wave_prefix = 0;
        for (int w = 0; w < wave; ++w) wave_prefix += s_wave[w];
#pragma unroll
        for (int q = 0; q < PER; ++q) s_digit_base[threadIdx.x * PER + q] = wave_prefix + incl - sum + loc[q];
        // single-pass sort by tile id: the digit bases ARE the tile ranges (A5)
        if (ranges_out && blockIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int d = threadIdx.x * PER + q;
                const uint32_t b0 = wave_prefix + incl - sum + loc[q], c = tot[q];
                if (d < nranges) ranges_out[d] = c ? make_uint2(b0, b0 + c) : make_uint2(0u, 0u);
            }
        }
    }
    __syncthreads();
}

// cursors of the block's WAVES chunks: runs of WAVES consecutive counts per digit (see sort_hist_kernel)
template <int BITS>
__device__ __forceinline__ void scatter_fill_cursors(const uint32_t (&my_cnt)[(1 << BITS) / 64], const uint32_t *s_digit_base,
                                                     uint32_t *s_cursor)
{
    constexpr int WAVES = SortBlock<BITS>::kWaves, STR = (1 << BITS) + 1;
#pragma unroll
    for (int q = 0; q < (1 << BITS) / 64; ++q) {
        const int idx = threadIdx.x + q * 64 * WAVES, d = idx / WAVES, w = idx % WAVES;
        s_cursor[w * STR + d] = s_digit_base[d] + my_cnt[q];
    }
}

// one round of 64 items: rank among the lanes of my digit, take the digit's cursor (the wave's slice `cursor`), store,
// the last peer moves the cursor on.  Wave-uniform control flow.
template <typename KeyT, int BITS>
__device__ __forceinline__ void scatter_round(bool valid, KeyT key, uint32_t val, int shift, uint64_t lt_mask,
                                              uint32_t *cursor, KeyT *keys_out,
                                              uint32_t *vals_out, const BlockMaskArgs &bm)
{
    const uint32_t digit = (uint32_t)(key >> shift) & (uint32_t)((1 << BITS) - 1);
    uint32_t rank, count;
    wave_digit_rank<BITS>(valid, digit, lt_mask, rank, count);
    uint32_t pos = 0;
    if (valid) pos = cursor[digit] + rank;
    __builtin_amdgcn_wave_barrier();
    if (valid) {
        if (keys_out) keys_out[pos] = key;      // (a caller that only wants the permutation passes null in the last pass)
        if (sizeof(KeyT) == 8 && bm.out) bm.out[pos] = make_uint2(val, block_mask_of(bm, digit, (uint32_t)((uint64_t)key >> 32)));
        else vals_out[pos] = val;
        if (rank == count - 1) cursor[digit] = pos + 1;
    }
    __builtin_amdgcn_wave_barrier();
}

template <typename KeyT, int BITS>
__global__ __launch_bounds__(64 * SortBlock<BITS>::kWaves) void sort_scatter_kernel(const KeyT *__restrict__ keys_in,
                                                           const uint32_t *__restrict__ vals_in,
                                                           KeyT *__restrict__ keys_out,
                                                           uint32_t *__restrict__ vals_out,
                                                           const uint32_t *__restrict__ count_ptr, uint32_t cap,
                                                           int shift, const uint32_t *__restrict__ cnt,
                                                           const uint32_t *__restrict__ totals, int nchunks_cap,
                                                           uint2 *__restrict__ ranges_out, int nranges,
                                                           uint32_t packed_val_mask, BlockMaskArgs bm)
{
    constexpr int BINS = 1 << BITS, PER = BINS / 256;   // digit totals handled per thread (of the first 256)
    constexpr int WAVES = SortBlock<BITS>::kWaves, STR = BINS + 1;
    __shared__ uint32_t s_cursor[WAVES * STR];
    __shared__ uint32_t s_digit_base[BINS];
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk0 = blockIdx.x * WAVES, chunk = chunk0 + wave;
    // Everything the block needs from memory is requested up front — its items, its rows of the count
    // table, the digit totals, the item count — so the waits below overlap into ONE round trip (with one
    // wave per SIMD nothing else would hide them).  Loads are guarded by the buffers' capacity, validity
    // (idx < R) is applied afterwards.
    const uint32_t base = (uint32_t)chunk * kSortWaveItems + lane;
    KeyT k[kSortRounds];
    uint32_t v[kSortRounds];
    // (clamped addresses instead of predicated loads: a conditional load per round compiles into a branch
    //  and a full wait per round — sixteen serialised round trips)
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) k[r] = keys_in[min(base + (uint32_t)r * 64, cap - 1u)];
    if (vals_in) {
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) v[r] = vals_in[min(base + (uint32_t)r * 64, cap - 1u)];
    } else {   // packed mode: the value is the low part of the key
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) v[r] = (uint32_t)k[r] & packed_val_mask;
    }
    constexpr int CPT = BINS / 64;             // count-table entries per thread: BINS * WAVES / (64 * WAVES)
    uint32_t my_cnt[CPT];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int idx = threadIdx.x + q * 64 * WAVES, d = idx / WAVES, w = idx % WAVES;
        my_cnt[q] = (chunk0 + w < nchunks_cap) ? cnt[(size_t)d * nchunks_cap + chunk0 + w] : 0u;
    }
    uint32_t tot[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) tot[q] = threadIdx.x < 256 ? totals[threadIdx.x * PER + q] : 0u;
    const uint32_t R = load_count(count_ptr, cap);
    const int nchunks = (int)((R + kSortWaveItems - 1) / kSortWaveItems);
    if (chunk0 >= nchunks) return;   // whole block beyond the data
    scatter_digit_bases<BITS>(tot, s_wave, s_digit_base, ranges_out, nranges);
    scatter_fill_cursors<BITS>(my_cnt, s_digit_base, s_cursor);
    __syncthreads();
    if (chunk >= nchunks) return;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r)
        scatter_round<KeyT, BITS>(base + (uint32_t)r * 64 < R, k[r], v[r], shift, lt_mask, s_cursor + wave * STR, keys_out,
                                  vals_out, bm);
}

// step 3 when the chunks are the EMISSION's (emit_tiles_kernel counted the digits of the instances each of its
// workgroups wrote: no histogram launch): chunk c = instances [chunk_start[c], chunk_start[c + 1]), a few hundred
// to a few thousand; one wave per chunk, 16 rounds of 64 in registers at a time.  Same positions as the pass over
// fixed 1024-item chunks: a stable partition does not care where the chunk boundaries are.
template <typename KeyT, int BITS>
__global__ __launch_bounds__(64 * SortBlock<BITS>::kWaves) void sort_scatter_chunks_kernel(
    const KeyT *__restrict__ keys_in, const uint32_t *__restrict__ vals_in, KeyT *__restrict__ keys_out,
    uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ chunk_start, uint32_t cap, int shift,
    const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ totals, int nchunks,
    uint2 *__restrict__ ranges_out, int nranges, uint32_t packed_val_mask, BlockMaskArgs bm)
{
    constexpr int BINS = 1 << BITS, PER = BINS / 256;
    constexpr int WAVES = SortBlock<BITS>::kWaves, STR = BINS + 1;
    __shared__ uint32_t s_cursor[WAVES * STR];
    __shared__ uint32_t s_digit_base[BINS];
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk0 = blockIdx.x * WAVES, chunk = chunk0 + wave;
    // (the chunk's bounds, its rows of the count table and the digit totals travel together; the items follow)
    const uint32_t cs = min(chunk_start[min(chunk, nchunks)], cap), ce = min(chunk_start[min(chunk + 1, nchunks)], cap);
    KeyT k[kSortRounds];
    uint32_t v[kSortRounds];
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) k[r] = keys_in[min(cs + (uint32_t)(r * 64 + lane), cap - 1u)];
    if (vals_in) {
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) v[r] = vals_in[min(cs + (uint32_t)(r * 64 + lane), cap - 1u)];
    }
    constexpr int CPT = BINS / 64;
    uint32_t my_cnt[CPT];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int idx = threadIdx.x + q * 64 * WAVES, d = idx / WAVES, w = idx % WAVES;
        my_cnt[q] = (chunk0 + w < nchunks) ? cnt[(size_t)d * nchunks + chunk0 + w] : 0u;
    }
    uint32_t tot[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) tot[q] = threadIdx.x < 256 ? totals[threadIdx.x * PER + q] : 0u;
    scatter_digit_bases<BITS>(tot, s_wave, s_digit_base, ranges_out, nranges);
    scatter_fill_cursors<BITS>(my_cnt, s_digit_base, s_cursor);
    __syncthreads();
    if (chunk >= nchunks) return;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    for (uint32_t b0 = cs; b0 < ce; b0 += (uint32_t)kSortWaveItems) {
        if (b0 != cs) {     // (a chunk of more than 1024 instances: the next 16 rounds)
#pragma unroll
            for (int r = 0; r < kSortRounds; ++r) k[r] = keys_in[min(b0 + (uint32_t)(r * 64 + lane), cap - 1u)];
            if (vals_in) {
#pragma unroll
                for (int r = 0; r < kSortRounds; ++r) v[r] = vals_in[min(b0 + (uint32_t)(r * 64 + lane), cap - 1u)];
            }
        }
        if (!vals_in) {     // packed mode: the value is the low part of the key
#pragma unroll
            for (int r = 0; r < kSortRounds; ++r) v[r] = (uint32_t)k[r] & packed_val_mask;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) {
            if (b0 + (uint32_t)(r * 64) >= ce) break;       // (wave-uniform)
            scatter_round<KeyT, BITS>(b0 + (uint32_t)(r * 64 + lane) < ce, k[r], v[r], shift, lt_mask, s_cursor + wave * STR,
                                      keys_out, vals_out, bm);
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
size_t sort_core_bytes(uint64_t cap)
{
    const uint64_t nchunks = (cap + kSortWaveItems - 1) / kSortWaveItems;
    return (size_t)(kSortMaxBins * (nchunks ? nchunks : 1) + kSortMaxBins) * sizeof(uint32_t);
}
// (count table + digit totals, and behind them the list of (surfel, block mask) pairs and the 64-bit instances it
//  is sorted from: sort_bmask_buffer, sort_wide_buffer)
size_t sort_scratch_bytes(uint64_t cap) { return sort_core_bytes(cap) + 2 * sizeof(uint64_t) * (size_t)cap + 64; }
uint2 *sort_bmask_buffer(void *scratch, uint64_t cap) { return (uint2 *)((char *)scratch + ((sort_core_bytes(cap) + 15) & ~(size_t)15)); }
uint64_t *sort_wide_buffer(void *scratch, uint64_t cap) { return (uint64_t *)(sort_bmask_buffer(scratch, cap) + cap); }

// digit width: as few passes as 11-bit digits allow, then the narrowest digit that still fits
static void sort_plan(int nbits, int &npasses, int &bits)
{
    npasses = (nbits + 10) / 11;
    bits = (nbits + npasses - 1) / npasses;
    if (bits < 8) bits = 8;
}
int sort_passes(int nbits)
{
    int np, b;
    sort_plan(nbits, np, b);
    return np;
}

int sort_rowscan_rows(uint32_t *cnt, int rows, int nchunks, uint32_t *totals, uint32_t cap, hipStream_t st)
{
    ScopedTimer tm(T_SORT_ROWSCAN, st);
    hipLaunchKernelGGL(sort_rowscan_kernel, dim3(rows), dim3(256), 0, st, cnt, (const uint32_t *)nullptr, cap, nchunks, totals,
                       nchunks);
    tm.end_now();
    SLS_LAUNCH_CHECK("sort_rowscan_kernel");
    return SLS_OK;
}

// rows of the emission's count table + scatter over its chunks (the histogram was the emission's)
template <typename KeyT, int BITS>
static int tile_sort_emit_chunks(const KeyT *kin, const EmitChunkSort &a, hipStream_t st)
{
    if (int rc = sort_rowscan_rows(a.cnt, 1 << BITS, a.nchunks, a.totals, a.cap, st)) return rc;
    {
        ScopedTimer tm(T_SORT_SCATTER, st);
        const int nblocks = (a.nchunks + SortBlock<BITS>::kWaves - 1) / SortBlock<BITS>::kWaves;
        hipLaunchKernelGGL((sort_scatter_chunks_kernel<KeyT, BITS>), dim3(nblocks), dim3(64 * SortBlock<BITS>::kWaves), 0, st,
                           kin, a.vals, (KeyT *)nullptr, a.vals_out, a.chunk_start, a.cap, a.shift, (const uint32_t *)a.cnt,
                           (const uint32_t *)a.totals, a.nchunks, a.ranges_out, a.nranges, a.packed_val_mask, a.bm);
    }
    SLS_LAUNCH_CHECK("sort_scatter_chunks_kernel");
    return SLS_OK;
}
template <typename KeyT>
static int tile_sort_emit_chunks_t(const KeyT *kin, const EmitChunkSort &a, hipStream_t st)
{
    switch (a.bits) {
    case 8: return tile_sort_emit_chunks<KeyT, 8>(kin, a, st);
    case 9: return tile_sort_emit_chunks<KeyT, 9>(kin, a, st);
    case 10: return tile_sort_emit_chunks<KeyT, 10>(kin, a, st);
    default: return tile_sort_emit_chunks<KeyT, 11>(kin, a, st);
    }
}
int tile_sort_emit_chunks_u32(const uint32_t *keys, const EmitChunkSort &a, hipStream_t st) { return tile_sort_emit_chunks_t(keys, a, st); }
int tile_sort_emit_chunks_u64(const uint64_t *keys, const EmitChunkSort &a, hipStream_t st) { return tile_sort_emit_chunks_t(keys, a, st); }

template <typename KeyT, int BITS>
static int radix_pass(const KeyT *kin, const uint32_t *vin, KeyT *kout, uint32_t *vout, const uint32_t *count_ptr,
                      uint32_t cap, int shift, uint32_t *cnt, uint32_t *totals, int nchunks,
                      uint2 *ranges_out, int nranges, uint32_t packed_val_mask, hipStream_t st,
                      const BlockMaskArgs &bm)
{
    const int nblocks = (nchunks + SortBlock<BITS>::kWaves - 1) / SortBlock<BITS>::kWaves;
    {
        ScopedTimer tm(T_SORT_HIST, st);
        hipLaunchKernelGGL((sort_hist_kernel<KeyT, BITS>), dim3(nblocks), dim3(64 * SortBlock<BITS>::kWaves), 0, st, kin,
                           count_ptr, cap, shift, cnt, nchunks);
    }
    SLS_LAUNCH_CHECK("sort_hist_kernel");
    {
        ScopedTimer tm(T_SORT_ROWSCAN, st);
        hipLaunchKernelGGL(sort_rowscan_kernel, dim3(1 << BITS), dim3(256), 0, st, cnt, count_ptr, cap, nchunks, totals, 0);
    }
    SLS_LAUNCH_CHECK("sort_rowscan_kernel");
    {
        ScopedTimer tm(T_SORT_SCATTER, st);
        hipLaunchKernelGGL((sort_scatter_kernel<KeyT, BITS>), dim3(nblocks), dim3(64 * SortBlock<BITS>::kWaves), 0, st, kin, vin, kout, vout,
                           count_ptr, cap, shift, (const uint32_t *)cnt, (const uint32_t *)totals, nchunks, ranges_out,
                           nranges, packed_val_mask, bm);
    }
    SLS_LAUNCH_CHECK("sort_scatter_kernel");
    return SLS_OK;
}

// Stable LSD radix sort of (key, u32 value) pairs on the low `nbits` key bits.
// Item count = min(*count_ptr, cap), read on the device.  Ping-pongs between
// (keys, vals) and (keys_tmp, vals_tmp); *result_in_tmp says where the sorted
// data ended up.  The options: RadixOptions, sls_launch.hpp.
// (Counting the next pass's digits inside the scatter / the producer with global
// atomics was measured and is slower than the histogram kernel: +35 us per pass.)
template <typename KeyT>
static int radix_sort_pairs_t(KeyT *keys, uint32_t *vals, KeyT *keys_tmp, uint32_t *vals_tmp,
                              const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch,
                              size_t scratch_bytes, int *result_in_tmp, hipStream_t st, const RadixOptions &opt)
{
    *result_in_tmp = 0;
    if (cap == 0 || nbits <= 0) return SLS_OK;
    if (scratch_bytes < sort_scratch_bytes(cap)) {
        set_error("sort scratch too small: %zu < %zu", scratch_bytes, sort_scratch_bytes(cap));
        return SLS_E_SCRATCH;
    }
    const int nchunks = (int)(((uint64_t)cap + kSortWaveItems - 1) / kSortWaveItems);
    uint32_t *cnt = (uint32_t *)scratch;
    int npasses, bits;
    sort_plan(nbits, npasses, bits);
    if (opt.ranges_out && npasses != 1) {
        set_error("internal: ranges need a single-pass sort");
        return SLS_E_ARG;
    }
    uint32_t *totals = cnt + ((size_t)1 << bits) * nchunks;
    KeyT *kb[2] = { keys, keys_tmp };
    uint32_t *vb[2] = { vals, vals_tmp };
    for (int p = 0; p < npasses; ++p) {
        const int shift = opt.base_shift + bits * p;
        const int src = p & 1, dst = src ^ 1;
        // packed single-pass sort (vals == null): the value travels in the key's low base_shift bits
        const uint32_t packed_val_mask = (vals == nullptr && opt.base_shift > 0) ? ((1u << opt.base_shift) - 1u) : 0u;
        int rc;
        KeyT *kout = (opt.drop_sorted_keys && p + 1 == npasses) ? nullptr : kb[dst];
#define SLS_PASS(B) radix_pass<KeyT, B>(kb[src], vb[src], kout, vb[dst], count_ptr, cap, shift, cnt, totals, nchunks, \
                                        opt.ranges_out, opt.nranges, packed_val_mask, st,                      \
                                        (npasses == 1 ? opt.bm : kNoRadixOptions.bm))
        switch (bits) {
        case 8: rc = SLS_PASS(8); break;
        case 9: rc = SLS_PASS(9); break;
        case 10: rc = SLS_PASS(10); break;
        default: rc = SLS_PASS(11); break;
        }
#undef SLS_PASS
        if (rc) return rc;
    }
    *result_in_tmp = npasses & 1;
    return SLS_OK;
}

int radix_sort_options_u32(uint32_t *keys, uint32_t *vals, uint32_t *keys_tmp, uint32_t *vals_tmp,
                           const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                           int *result_in_tmp, hipStream_t st, const RadixOptions &opt)
{
    return radix_sort_pairs_t(keys, vals, keys_tmp, vals_tmp, count_ptr, cap, nbits, scratch, scratch_bytes, result_in_tmp, st, opt);
}
int radix_sort_options_u64(uint64_t *keys, uint32_t *vals, uint64_t *keys_tmp, uint32_t *vals_tmp,
                           const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                           int *result_in_tmp, hipStream_t st, const RadixOptions &opt)
{
    return radix_sort_pairs_t(keys, vals, keys_tmp, vals_tmp, count_ptr, cap, nbits, scratch, scratch_bytes, result_in_tmp, st, opt);
}
int radix_sort_pairs_u32(uint32_t *keys, uint32_t *vals, uint32_t *keys_tmp, uint32_t *vals_tmp,
                         const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                         int *result_in_tmp, hipStream_t st)
{
    return radix_sort_pairs_t(keys, vals, keys_tmp, vals_tmp, count_ptr, cap, nbits, scratch, scratch_bytes, result_in_tmp, st, kNoRadixOptions);
}
int radix_sort_pairs_u64(uint64_t *keys, uint32_t *vals, uint64_t *keys_tmp, uint32_t *vals_tmp,
                         const uint32_t *count_ptr, uint32_t cap, int nbits, void *scratch, size_t scratch_bytes,
                         int *result_in_tmp, hipStream_t st)
{
    return radix_sort_pairs_t(keys, vals, keys_tmp, vals_tmp, count_ptr, cap, nbits, scratch, scratch_bytes, result_in_tmp, st, kNoRadixOptions);
}

}  // namespace sls

