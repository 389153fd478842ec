// sls_fill.hip — filling the small holes of a mesh on the device (sls_mesh_boundary_loops, sls_mesh_fill_holes): the boundary
// half-edges of a mesh, the closed loops they form, and a fan over the centroid of every loop that is small enough.
// include/sls_fill_math.h states every rule, tests/fill_ref.py restates it in NumPy; DESIGN.md section 2, "Mesh hole
// filling", states the contract.  Built EXACT (-ffp-contract=off): the bits of the new vertices are part of the contract.
// No floating-point atomics, no hash table, nothing read back: the live counts, B, the number of loops and the verdict on
// the room are device words, and every launch is sized by the capacity.
//
// Launches ordered by the stream alone:
//   fill_init / fill_keys + two stable sorts   the three half-edges (a, b) of every non-degenerate live triangle ((0, 0) for
//                               any other row: sorted in front of every pair) as two u32 arrays, sorted by b, then by a
//   fill_mark + scan + fill_compact   a pair is a boundary half-edge iff it stands alone in its run and a lower-bound
//                               search finds no (b, a); the survivors leave in key order: half-edge h = (ha[h], hb[h])
//   fill_degrees / _union / _complex   the half-edges that leave and enter every vertex (integer atomics), the one that
//                               leaves it, the union-find of sls_unionfind.hpp over h and next(h) where the head is simple
//   fill_roots / _rootkeys + one stable sort   root[h] (the lowest half-edge of the component), the components that touch a
//                               complex vertex poisoned, then sorted by root: every loop a segment in ascending tail
//   fill_heads + scan + fill_segments   the number of every loop, where it starts, out_loop
//   fill_verdict_short / _long  a lane per loop of at most 64 edges (and every loop above max_edges), a wave per longer
//                               loop (lane l adds l, l + 64, ..., then a fixed xor butterfly): verdict, centroid, needs
//   scan + fill_decide          where every loop's vertex and triangles go; the needs against the room; the status
//   fill_copy / fill_write      the live rows and the -1 padding; the fans (skipped on overflow: a device word)
// The chunked scans (fill_totals / _blkscan / _apply) work in place over 2048 entries per workgroup.
#include "sls_geom.hpp"
#include "sls_scan.hpp"
#include "sls_unionfind.hpp"
#include "../../include/sls_fill_math.h"

namespace sls {

constexpr int kFillThreads = 512;
using FillChunks = Chunks<kFillThreads, 4>;                 // the chunked scans: 2048 entries per workgroup
constexpr int kFillLongBlocks = 2048;                       // the long-loop kernel strides over the loops
constexpr int kFillLongThreads = 256;

// hdr words
enum { FH_N3 = 0, FH_VL, FH_TL, FH_B, FH_LOOPS, FH_OPEN, FH_COMPLEX, FH_DEGENERATE, FH_RANGE, FH_FILLED, FH_SKIP_EDGES, FH_SKIP_SIZE,
       FH_SKIP_NONFINITE, FH_OVERFLOW, FH_NEW_V, FH_NEW_T, FH_WORDS };

__global__ void fill_init_kernel(uint32_t *hdr, uint32_t n3, int V, int T, const uint32_t *__restrict__ in_counts)
{
    const uint32_t i = threadIdx.x;
    if (i >= 32) return;
    uint32_t v = 0u;
    if (i == FH_N3) v = n3;
    if (i == FH_VL) v = (uint32_t)(in_counts ? sls_fill_live(in_counts[0], V) : V);
    if (i == FH_TL) v = (uint32_t)(in_counts ? sls_fill_live(in_counts[1], T) : T);
    hdr[i] = v;
}

__global__ __launch_bounds__(kFillThreads) void fill_keys_kernel(int T, const int32_t *__restrict__ faces, uint32_t *hdr,
                                                                 uint32_t *__restrict__ ka, uint32_t *__restrict__ kb)
{
    const size_t t = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    const int32_t VL = (int32_t)hdr[FH_VL];
    int deg = 0;
    if (t < (size_t)T) {
        const bool live = t < (size_t)hdr[FH_TL];
        const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
        deg = live ? sls_mesh_degenerate(f, VL) : 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            int32_t a = 0, b = 0;
            if (live && !deg) sls_fill_half_edge(f, e, &a, &b);
            ka[3 * t + e] = (uint32_t)a;
            kb[3 * t + e] = (uint32_t)b;
        }
    }
    count_degenerate(deg, &hdr[FH_DEGENERATE], &hdr[FH_RANGE]);
}

// flag[p] = 1 iff the sorted pair at p is a boundary half-edge: alone in its run, and no (b, a) anywhere
__global__ __launch_bounds__(kFillThreads) void fill_mark_kernel(uint32_t n, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                                 uint32_t *__restrict__ flag)
{
    const size_t p = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t a = sa[p], b = sb[p];
    uint32_t is = 0u;
    if (a != b) {                                                   // (not the (0, 0) of a row that takes no part)
        const uint64_t k = ((uint64_t)a << 32) | b;
        const bool alone = (p == 0 || pair_key(sa, sb, (uint32_t)p - 1u) != k) && (p + 1 >= n || pair_key(sa, sb, (uint32_t)p + 1u) != k);
        if (alone) {
            const uint64_t target = ((uint64_t)b << 32) | a;
            uint32_t lo = 0u, hi = n;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (pair_key(sa, sb, mid) < target) lo = mid + 1u; else hi = mid; }
            is = (lo < n && pair_key(sa, sb, lo) == target) ? 0u : 1u;
        }
    }
    flag[p] = is;
}

// ---- the chunked exclusive scan of arr[0 .. n) in place; *total: the sum ----------------------------------------------
template <typename W>
__global__ __launch_bounds__(kFillThreads) void fill_totals_kernel(uint32_t n, const W *__restrict__ arr, W *__restrict__ blk)
{
    const uint32_t p0 = FillChunks::first();
    W sum = 0;
#pragma unroll
    for (int j = 0; j < FillChunks::kPer; ++j)
        if (p0 + (uint32_t)j < n) sum += arr[p0 + (uint32_t)j];
    FillChunks::total(sum, blk);
}

template <typename W>
__global__ __launch_bounds__(kFillThreads) void fill_blkscan_kernel(int nblk, W *blk, W *__restrict__ total)
{
    const W sum = FillChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) *total = sum;
}

template <typename W>
__global__ __launch_bounds__(kFillThreads) void fill_apply_kernel(uint32_t n, W *__restrict__ arr, const W *__restrict__ blk)
{
    const uint32_t p0 = FillChunks::first();
    W v[FillChunks::kPer], sum = 0;
#pragma unroll
    for (int j = 0; j < FillChunks::kPer; ++j) {
        v[j] = p0 + (uint32_t)j < n ? arr[p0 + (uint32_t)j] : (W)0;
        sum += v[j];
    }
    W run = FillChunks::rank(sum, blk);
#pragma unroll
    for (int j = 0; j < FillChunks::kPer; ++j)
        if (p0 + (uint32_t)j < n) { arr[p0 + (uint32_t)j] = run; run += v[j]; }
}

template <typename W>
static int fill_scan(uint32_t n, W *arr, W *blk, W *total, hipStream_t st)
{
    const int nblk = FillChunks::count(n);
    hipLaunchKernelGGL((fill_totals_kernel<W>), dim3(nblk), dim3(kFillThreads), 0, st, n, (const W *)arr, blk);
    SLS_LAUNCH_CHECK("fill_totals_kernel");
    hipLaunchKernelGGL((fill_blkscan_kernel<W>), dim3(1), dim3(kFillThreads), 0, st, nblk, blk, total);
    SLS_LAUNCH_CHECK("fill_blkscan_kernel");
    hipLaunchKernelGGL((fill_apply_kernel<W>), dim3(nblk), dim3(kFillThreads), 0, st, n, arr, (const W *)blk);
    SLS_LAUNCH_CHECK("fill_apply_kernel");
    return SLS_OK;
}

// rank: the exclusive scan of the flags (hdr[FH_B]: their sum); half-edge rank[p] = the flagged pair at p
__global__ __launch_bounds__(kFillThreads) void fill_compact_kernel(uint32_t n, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                                    const uint32_t *__restrict__ rank, const uint32_t *__restrict__ hdr,
                                                                    uint32_t *__restrict__ ha, uint32_t *__restrict__ hb, uint32_t *__restrict__ parent,
                                                                    int32_t *__restrict__ out_halfedges)
{
    const size_t p = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = rank[p], next = p + 1 < n ? rank[p + 1] : hdr[FH_B];
    if (next == r || r >= n) return;                                // (r < n always: a flag per position at most)
    ha[r] = sa[p];
    hb[r] = sb[p];
    parent[r] = r;
    if (out_halfedges) { out_halfedges[2 * (size_t)r] = (int32_t)sa[p]; out_halfedges[2 * (size_t)r + 1] = (int32_t)sb[p]; }
}

__global__ __launch_bounds__(kFillThreads) void fill_degrees_kernel(uint32_t n, uint32_t V, const uint32_t *__restrict__ hdr,
                                                                    const uint32_t *__restrict__ ha, const uint32_t *__restrict__ hb,
                                                                    uint32_t *outdeg, uint32_t *indeg, uint32_t *first_out)
{
    const size_t h = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (h >= min(hdr[FH_B], n)) return;
    const uint32_t a = ha[h], b = hb[h];
    if (a >= V || b >= V) return;                                   // (never: both lie inside the live vertices)
    atomicAdd(&outdeg[a], 1u);
    atomicAdd(&indeg[b], 1u);
    first_out[a] = (uint32_t)h;                                     // (read only where exactly one half-edge leaves a)
}

__global__ __launch_bounds__(kFillThreads) void fill_union_kernel(uint32_t n, uint32_t V, const uint32_t *__restrict__ hdr,
                                                                  const uint32_t *__restrict__ hb, const uint32_t *__restrict__ outdeg,
                                                                  const uint32_t *__restrict__ indeg, const uint32_t *__restrict__ first_out,
                                                                  uint32_t *parent)
{
    const size_t h = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    const uint32_t B = min(hdr[FH_B], n);
    if (h >= B) return;
    const uint32_t b = hb[h];
    if (b >= V || !sls_fill_simple(outdeg[b], indeg[b])) return;
    const uint32_t next = first_out[b];
    if (next < B) uf_unite(parent, (uint32_t)h, next);
}

__global__ __launch_bounds__(kFillThreads) void fill_complex_kernel(uint32_t V, const uint32_t *__restrict__ outdeg,
                                                                    const uint32_t *__restrict__ indeg, uint32_t *hdr)
{
    const size_t v = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    bool is = false;
    if (v < V) {
        const uint32_t o = outdeg[v], i = indeg[v];
        is = (o | i) != 0u && !sls_fill_simple(o, i);
    }
    const uint64_t m = __ballot(is);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&hdr[FH_COMPLEX], (uint32_t)__popcll(m));
}

// root[h] (a launch of its own: parent is only read); a half-edge with a complex end poisons its component
__global__ __launch_bounds__(kFillThreads) void fill_roots_kernel(uint32_t n, uint32_t V, const uint32_t *__restrict__ hdr,
                                                                  const uint32_t *__restrict__ parent, const uint32_t *__restrict__ ha,
                                                                  const uint32_t *__restrict__ hb, const uint32_t *__restrict__ outdeg,
                                                                  const uint32_t *__restrict__ indeg, uint32_t *__restrict__ root, uint8_t *bad)
{
    const size_t h = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    const uint32_t B = min(hdr[FH_B], n);
    if (h >= B) return;
    uint32_t x = (uint32_t)h, p = parent[x];
    while (p != x && p < B) { x = p; p = parent[x]; }
    root[h] = x;
    const uint32_t a = min(ha[h], V - 1u), b = min(hb[h], V - 1u);  // (inside [0, V): the clamps never bite)
    if (!sls_fill_simple(outdeg[a], indeg[a]) || !sls_fill_simple(outdeg[b], indeg[b])) bad[x] = 1;
}

// the sort key of half-edge h: its root, or n (behind every root) where its component is open
__global__ __launch_bounds__(kFillThreads) void fill_rootkeys_kernel(uint32_t n, uint32_t *hdr, const uint32_t *__restrict__ root,
                                                                     const uint8_t *__restrict__ bad, uint32_t *__restrict__ rk,
                                                                     uint32_t *__restrict__ rv)
{
    const size_t h = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    bool open = false;
    if (h < min(hdr[FH_B], n)) {
        const uint32_t r = min(root[h], n - 1u);
        open = bad[r] != 0;
        rk[h] = open ? n : r;
        rv[h] = (uint32_t)h;
    }
    const uint64_t m = __ballot(open);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&hdr[FH_OPEN], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(kFillThreads) void fill_heads_kernel(uint32_t n, const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ sr,
                                                                  uint32_t *__restrict__ flag)
{
    const size_t p = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (p >= n) return;
    flag[p] = Chunks<kFillThreads, 1>::head_mask(hdr[FH_B], (uint32_t)p, [&](uint32_t q) { return sr[q]; }, n);     // (key n: open, no loop)
}

// rank: the exclusive scan of the head flags (hdr[FH_LOOPS]: their sum); ploop[p]: the loop of sorted position p or -1
__global__ __launch_bounds__(kFillThreads) void fill_segments_kernel(uint32_t n, uint32_t max_loops, const uint32_t *__restrict__ hdr,
                                                                     const uint32_t *__restrict__ sr, const uint32_t *__restrict__ sv,
                                                                     const uint32_t *__restrict__ rank, uint32_t *__restrict__ loop_start,
                                                                     int32_t *__restrict__ ploop, int32_t *__restrict__ out_loop)
{
    const size_t p = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    const uint32_t B = min(hdr[FH_B], n), loops = min(hdr[FH_LOOPS], max_loops);
    if (p == 0) loop_start[loops] = B - min(hdr[FH_OPEN], B);       // the end of the last loop: the open half-edges follow
    if (p >= B) return;
    int32_t id = -1;
    if (sr[p] != n) {
        const uint32_t r = rank[p];
        const bool head = p == 0 || sr[p - 1] != sr[p];
        id = head ? (int32_t)r : (int32_t)r - 1;
        if (head && r < max_loops) loop_start[r] = (uint32_t)p;     // (r < max_loops always: a loop holds three half-edges)
    }
    ploop[p] = id;
    const uint32_t h = sv[p];
    if (out_loop && h < n) out_loop[h] = id;
}

__global__ __launch_bounds__(kFillThreads) void fill_lengths_kernel(uint32_t max_loops, const uint32_t *__restrict__ hdr,
                                                                    const uint32_t *__restrict__ loop_start, int32_t *__restrict__ out_loop_edges)
{
    const size_t k = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (k < min(hdr[FH_LOOPS], max_loops)) out_loop_edges[k] = (int32_t)(loop_start[k + 1] - loop_start[k]);
}

struct VerdictArgs {
    uint32_t n, V, max_loops, max_edges;
    double max_size;
    const uint32_t *loop_start, *sv, *ha;
    const float *xyz;
    uint32_t *verdict;
    float *centroid;                // 3 floats per loop
    uint64_t *needs;                // new vertices << 32 | new triangles, per loop; 0 behind the last loop
};

__device__ __forceinline__ const float *fill_vertex(const VerdictArgs &a, uint32_t p)
{
    const uint32_t h = min(a.sv[p], a.n - 1u);
    return a.xyz + 3 * (size_t)min(a.ha[h], a.V - 1u);              // (inside [0, V): the clamps never bite)
}

__device__ __forceinline__ void fill_verdict_store(const VerdictArgs &a, uint32_t k, uint32_t L, int verdict, const double acc[3], uint32_t *hdr)
{
    a.verdict[k] = (uint32_t)verdict;
    if (sls_fill_new_vertices(L, verdict)) sls_fill_centroid(acc, L, a.centroid + 3 * (size_t)k);
    a.needs[k] = ((uint64_t)sls_fill_new_vertices(L, verdict) << 32) | (uint64_t)sls_fill_new_triangles(L, verdict);
    atomicAdd(&hdr[verdict == SLS_FILL_FILLED ? FH_FILLED : verdict == SLS_FILL_SKIP_EDGES ? FH_SKIP_EDGES
                   : verdict == SLS_FILL_SKIP_SIZE ? FH_SKIP_SIZE : FH_SKIP_NONFINITE], 1u);
}

// a lane per loop: loops of at most 64 edges, and those above max_edges (no vertex is read); the others are left to
// fill_verdict_long
__global__ __launch_bounds__(kFillThreads) void fill_verdict_short_kernel(VerdictArgs a, uint32_t *hdr)
{
    const size_t k = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (k >= a.max_loops) return;
    if (k >= hdr[FH_LOOPS]) { a.needs[k] = 0u; return; }
    const uint32_t e = min(a.loop_start[k + 1], a.n), s = min(a.loop_start[k], e), L = e - s;
    double acc[3] = { 0.0, 0.0, 0.0 };
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    int finite = 1;
    if (L <= a.max_edges) {
        if (L > (uint32_t)SLS_FILL_LONG) return;
        for (uint32_t p = s; p < e; ++p) {
            const float *q = fill_vertex(a, p);
            const float v[3] = { q[0], q[1], q[2] };
            finite &= sls_fill_finite3(v);
            sls_fill_box(lo, hi, v);
            sls_fill_add(acc, v);
        }
    }
    fill_verdict_store(a, (uint32_t)k, L, sls_fill_verdict(L, finite, lo, hi, a.max_edges, a.max_size), acc, hdr);
}

// a wave per loop of more than 64 edges (and at most max_edges)
__global__ __launch_bounds__(kFillLongThreads) void fill_verdict_long_kernel(VerdictArgs a, uint32_t *hdr)
{
    const int lane = threadIdx.x & 63;
    const uint32_t loops = min(hdr[FH_LOOPS], a.max_loops);
    const uint32_t waves = gridDim.x * (uint32_t)(kFillLongThreads / 64);
    for (uint32_t k = blockIdx.x * (uint32_t)(kFillLongThreads / 64) + (threadIdx.x >> 6); k < loops; k += waves) {      // (wave-uniform)
        const uint32_t e = min(a.loop_start[k + 1], a.n), s = min(a.loop_start[k], e), L = e - s;
        if (L <= (uint32_t)SLS_FILL_LONG || L > a.max_edges) continue;
        double part[3] = { 0.0, 0.0, 0.0 };
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        int finite = 1;
        for (uint32_t p = s + (uint32_t)lane; p < e; p += 64u) {
            const float *q = fill_vertex(a, p);
            const float v[3] = { q[0], q[1], q[2] };
            finite &= sls_fill_finite3(v);
            sls_fill_box(lo, hi, v);
            sls_fill_add(part, v);
        }
        finite = __all(finite);
        xor_butterfly<3>(part);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float l2 = __shfl_xor(lo[c], off, 64), h2 = __shfl_xor(hi[c], off, 64);
                lo[c] = l2 < lo[c] ? l2 : lo[c];
                hi[c] = h2 > hi[c] ? h2 : hi[c];
            }
        }
        if (lane == 0) fill_verdict_store(a, k, L, sls_fill_verdict(L, finite, lo, hi, a.max_edges, a.max_size), part, hdr);
    }
}

// the needs against the room, and the status words; *total: new vertices << 32 | new triangles
__global__ void fill_decide_kernel(uint32_t *hdr, const uint64_t *__restrict__ total, uint32_t cap_vertices, uint32_t cap_triangles,
                                   int fills, uint32_t *__restrict__ status)
{
    if (threadIdx.x != 0) return;
    const uint64_t new_v = fills ? (*total >> 32) : 0u, new_t = fills ? (*total & 0xFFFFFFFFu) : 0u;
    const uint64_t need_v = fills ? (uint64_t)hdr[FH_VL] + new_v : 0u, need_t = fills ? (uint64_t)hdr[FH_TL] + new_t : 0u;
    const uint32_t over = (need_v > cap_vertices || need_t > cap_triangles) ? 1u : 0u;      // (the loops alone: no room is asked for)
    hdr[FH_OVERFLOW] = over;
    hdr[FH_NEW_V] = over ? 0u : (uint32_t)new_v;
    hdr[FH_NEW_T] = over ? 0u : (uint32_t)new_t;
    status[SLS_FILL_W_VERTICES] = fills ? hdr[FH_VL] + hdr[FH_NEW_V] : 0u;
    status[SLS_FILL_W_TRIANGLES] = fills ? hdr[FH_TL] + hdr[FH_NEW_T] : 0u;
    status[SLS_FILL_W_HALFEDGES] = hdr[FH_B];
    status[SLS_FILL_W_LOOPS] = hdr[FH_LOOPS];
    status[SLS_FILL_W_FILLED] = over ? 0u : hdr[FH_FILLED];
    status[SLS_FILL_W_SKIP_EDGES] = hdr[FH_SKIP_EDGES];
    status[SLS_FILL_W_SKIP_SIZE] = hdr[FH_SKIP_SIZE];
    status[SLS_FILL_W_SKIP_NONFINITE] = hdr[FH_SKIP_NONFINITE];
    status[SLS_FILL_W_OPEN] = hdr[FH_OPEN];
    status[SLS_FILL_W_COMPLEX] = hdr[FH_COMPLEX];
    status[SLS_FILL_W_DEGENERATE] = hdr[FH_DEGENERATE];
    status[SLS_FILL_W_RANGE] = hdr[FH_RANGE];
    status[SLS_FILL_W_NEED_VERTICES] = (uint32_t)need_v;            // (both fit: V + T and 4 T stay below 2^32)
    status[SLS_FILL_W_NEED_TRIANGLES] = (uint32_t)need_t;
    status[SLS_FILL_W_OVERFLOW] = over;
    status[SLS_FILL_W_WRITTEN] = 1u;
}

// the live rows word by word, and -1 behind the last triangle; counts: [V_live, T_live, new triangles] (hdr + FH_VL ..., or
// the words of the call without a triangle)
__global__ __launch_bounds__(kFillThreads) void fill_copy_kernel(uint32_t V, uint32_t T, uint32_t cap_triangles, uint32_t vl, uint32_t tl,
                                                                 const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ in_counts,
                                                                 const uint32_t *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                                 uint32_t *__restrict__ out_vertices, int32_t *__restrict__ out_faces)
{
    const size_t i = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    uint32_t new_t = 0u;
    if (hdr) { vl = hdr[FH_VL]; tl = hdr[FH_TL]; new_t = hdr[FH_NEW_T]; }
    else if (in_counts) { vl = (uint32_t)sls_fill_live(in_counts[0], (int32_t)V); tl = (uint32_t)sls_fill_live(in_counts[1], (int32_t)T); }
    vl = min(vl, V); tl = min(tl, T);
    if (i < 3 * (size_t)vl) out_vertices[i] = vertices[i];
    if (i < 3 * (size_t)cap_triangles) {
        const size_t row = i / 3;
        if (row < tl) out_faces[i] = faces[i];
        else if (row >= (size_t)tl + new_t) out_faces[i] = -1;
    }
}

struct WriteArgs {
    uint32_t n, V, max_loops, cap_vertices, cap_triangles;
    const uint32_t *hdr, *loop_start, *sv, *ha, *hb, *first_out, *verdict;
    const int32_t *ploop;
    const float *centroid;
    const uint64_t *offsets;        // the exclusive scan of the needs
    float *out_vertices;
    int32_t *out_faces;
};

// a lane per half-edge of a loop, in the sorted order: the triangle of a fan, or the one triangle of a loop of three
__global__ __launch_bounds__(kFillThreads) void fill_write_kernel(WriteArgs a)
{
    const size_t p = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (a.hdr[FH_OVERFLOW]) return;
    const uint32_t loops = min(a.hdr[FH_LOOPS], a.max_loops);
    if (p >= min(a.loop_start[loops], a.n)) return;
    const int32_t id = a.ploop[p];
    if (id < 0 || (uint32_t)id >= loops) return;                    // (never: the open half-edges lie behind)
    const uint32_t k = (uint32_t)id;
    if (a.verdict[k] != (uint32_t)SLS_FILL_FILLED) return;
    const uint32_t s = a.loop_start[k], L = a.loop_start[k + 1] - s, j = (uint32_t)p - s;
    const uint64_t off = a.offsets[k];
    const uint32_t h = min(a.sv[p], a.n - 1u);
    const uint32_t va = a.ha[h], vb = a.hb[h];
    const size_t row = (size_t)a.hdr[FH_TL] + (uint32_t)(off & 0xFFFFFFFFu) + (L > 3u ? j : 0u);
    if (row >= a.cap_triangles) return;                             // (never: the room was checked)
    int32_t *f = a.out_faces + 3 * row;
    if (L == 3u) {
        if (j != 0u) return;
        const uint32_t h1 = min(a.first_out[min(vb, a.V - 1u)], a.n - 1u);     // the half-edge that leaves n1 = vb
        f[0] = (int32_t)va; f[1] = (int32_t)a.hb[h1]; f[2] = (int32_t)vb;
        return;
    }
    const size_t c = (size_t)a.hdr[FH_VL] + (uint32_t)(off >> 32);
    if (c >= a.cap_vertices) return;                                // (never)
    f[0] = (int32_t)vb; f[1] = (int32_t)va; f[2] = (int32_t)c;
    if (j == 0u) {
        a.out_vertices[3 * c] = a.centroid[3 * (size_t)k];
        a.out_vertices[3 * c + 1] = a.centroid[3 * (size_t)k + 1];
        a.out_vertices[3 * c + 2] = a.centroid[3 * (size_t)k + 2];
    }
}

// the call without a vertex or without a triangle: no half-edge; with V == 0 every live row is out of range
__global__ void fill_empty_status_kernel(uint32_t V, uint32_t T, const uint32_t *__restrict__ in_counts, int fills, uint32_t *__restrict__ status)
{
    const uint32_t i = threadIdx.x;
    if (i >= 16) return;
    const uint32_t vl = in_counts ? (uint32_t)sls_fill_live(in_counts[0], (int32_t)V) : V;
    const uint32_t tl = in_counts ? (uint32_t)sls_fill_live(in_counts[1], (int32_t)T) : T;
    uint32_t w = 0u;
    if (fills && (i == SLS_FILL_W_VERTICES || i == SLS_FILL_W_NEED_VERTICES)) w = vl;
    if (fills && (i == SLS_FILL_W_TRIANGLES || i == SLS_FILL_W_NEED_TRIANGLES)) w = tl;
    if (i == SLS_FILL_W_DEGENERATE || i == SLS_FILL_W_RANGE) w = tl;       // (T == 0: none; V == 0: all of them)
    if (i == SLS_FILL_W_WRITTEN) w = 1u;
    status[i] = w;
}

// ---------------------------------------------------------------------------------------------------------------------
// scratch layout (all 256-byte aligned) and the launchers
// ---------------------------------------------------------------------------------------------------------------------
struct FillScratch {
    uint32_t *hdr, *k[4], *scan, *ha, *hb, *parent, *root, *outdeg, *indeg, *first_out, *loop_start, *verdict;
    int32_t *ploop;
    uint8_t *bad;
    float *centroid;
    uint64_t *needs, *blk, *total;
    void *sort;
    size_t sort_bytes, total_bytes;
};

static FillScratch fill_layout(size_t V, size_t T, void *base)
{
    FillScratch s;
    Arena a(base);
    const size_t n = 3 * T;
    s.hdr = a.take<uint32_t>(32);
    s.total = a.take<uint64_t>(1);
    for (int i = 0; i < 4; ++i) s.k[i] = a.take<uint32_t>(n);
    s.scan = a.take<uint32_t>(n);
    s.ha = a.take<uint32_t>(n);
    s.hb = a.take<uint32_t>(n);
    s.parent = a.take<uint32_t>(n);
    s.root = a.take<uint32_t>(n);
    s.ploop = a.take<int32_t>(n);
    s.bad = a.take<uint8_t>(n);
    s.outdeg = a.take<uint32_t>(V);
    s.indeg = a.take<uint32_t>(V);
    s.first_out = a.take<uint32_t>(V);
    s.loop_start = a.take<uint32_t>(T + 1);
    s.verdict = a.take<uint32_t>(T);
    s.centroid = a.take<float>(3 * T);
    s.needs = a.take<uint64_t>(T);
    s.blk = a.take<uint64_t>((size_t)FillChunks::count(n));
    s.sort_bytes = sort_scratch_bytes((uint64_t)n);
    s.sort = a.take<char>(s.sort_bytes);
    s.total_bytes = a.off;
    return s;
}

size_t mesh_fill_scratch_bytes(int V, int T)
{
    return mesh_sizes_ok(V, T) ? fill_layout((size_t)V, (size_t)T, nullptr).total_bytes : 0;
}

// what both calls share: half-edges, loops, out_loop; afterwards s.k[*sorted] holds the sorted roots and s.k[*sorted + 1] the
// half-edge of every sorted position
static int fill_loops(int V, int T, const int32_t *faces, const uint32_t *in_counts, int32_t *out_halfedges, int32_t *out_loop,
                      const FillScratch &s, int *sorted, hipStream_t st)
{
    const uint32_t Vu = (uint32_t)V, n = 3u * (uint32_t)T;
    const int bits = sls_mesh_index_bits(V);
    hipLaunchKernelGGL(fill_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, n, V, T, in_counts);
    SLS_LAUNCH_CHECK("fill_init_kernel");
    hipLaunchKernelGGL(fill_keys_kernel, grid_for((size_t)T, kFillThreads), dim3(kFillThreads), 0, st, T, faces, s.hdr, s.k[0], s.k[2]);
    SLS_LAUNCH_CHECK("fill_keys_kernel");
    uint32_t *a2[2] = { s.k[0], s.k[1] }, *b2[2] = { s.k[2], s.k[3] };
    int which = 0, cur = 0;
    int rc = sort_pairs_ab(a2, b2, s.hdr + FH_N3, n, bits, s.sort, s.sort_bytes, &cur, st);
    if (rc) return rc;
    const uint32_t *sa = a2[cur], *sb = b2[cur];
    hipLaunchKernelGGL(fill_mark_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, sa, sb, s.scan);
    SLS_LAUNCH_CHECK("fill_mark_kernel");
    rc = fill_scan<uint32_t>(n, s.scan, (uint32_t *)s.blk, s.hdr + FH_B, st);
    if (rc) return rc;
    hipLaunchKernelGGL(fill_compact_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, sa, sb, (const uint32_t *)s.scan,
                       (const uint32_t *)s.hdr, s.ha, s.hb, s.parent, out_halfedges);
    SLS_LAUNCH_CHECK("fill_compact_kernel");
    SLS_HIP_CHECK(hipMemsetAsync(s.outdeg, 0, sizeof(uint32_t) * (size_t)V, st));
    SLS_HIP_CHECK(hipMemsetAsync(s.indeg, 0, sizeof(uint32_t) * (size_t)V, st));
    SLS_HIP_CHECK(hipMemsetAsync(s.bad, 0, (size_t)n, st));
    hipLaunchKernelGGL(fill_degrees_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, Vu, (const uint32_t *)s.hdr, (const uint32_t *)s.ha,
                       (const uint32_t *)s.hb, s.outdeg, s.indeg, s.first_out);
    SLS_LAUNCH_CHECK("fill_degrees_kernel");
    hipLaunchKernelGGL(fill_union_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, Vu, (const uint32_t *)s.hdr, (const uint32_t *)s.hb,
                       (const uint32_t *)s.outdeg, (const uint32_t *)s.indeg, (const uint32_t *)s.first_out, s.parent);
    SLS_LAUNCH_CHECK("fill_union_kernel");
    hipLaunchKernelGGL(fill_complex_kernel, grid_for((size_t)V, kFillThreads), dim3(kFillThreads), 0, st, Vu, (const uint32_t *)s.outdeg,
                       (const uint32_t *)s.indeg, s.hdr);
    SLS_LAUNCH_CHECK("fill_complex_kernel");
    hipLaunchKernelGGL(fill_roots_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, Vu, (const uint32_t *)s.hdr, (const uint32_t *)s.parent,
                       (const uint32_t *)s.ha, (const uint32_t *)s.hb, (const uint32_t *)s.outdeg, (const uint32_t *)s.indeg, s.root, s.bad);
    SLS_LAUNCH_CHECK("fill_roots_kernel");
    // the sorted pairs are spent: their four arrays hold the sort by root
    hipLaunchKernelGGL(fill_rootkeys_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, s.hdr, (const uint32_t *)s.root, (const uint8_t *)s.bad,
                       s.k[0], s.k[1]);
    SLS_LAUNCH_CHECK("fill_rootkeys_kernel");
    rc = radix_sort_pairs_u32(s.k[0], s.k[1], s.k[2], s.k[3], s.hdr + FH_B, n, sls_mesh_index_bits((int32_t)n + 1), s.sort, s.sort_bytes,
                              &which, st);
    if (rc) return rc;
    *sorted = which ? 2 : 0;
    const uint32_t *sr = s.k[*sorted], *sv = s.k[*sorted + 1];
    hipLaunchKernelGGL(fill_heads_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, (const uint32_t *)s.hdr, sr, s.scan);
    SLS_LAUNCH_CHECK("fill_heads_kernel");
    rc = fill_scan<uint32_t>(n, s.scan, (uint32_t *)s.blk, s.hdr + FH_LOOPS, st);
    if (rc) return rc;
    hipLaunchKernelGGL(fill_segments_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, n, (uint32_t)T, (const uint32_t *)s.hdr, sr, sv,
                       (const uint32_t *)s.scan, s.loop_start, s.ploop, out_loop);
    SLS_LAUNCH_CHECK("fill_segments_kernel");
    return SLS_OK;
}

int launch_mesh_boundary_loops(int V, int T, const int32_t *faces, const uint32_t *in_counts, int32_t *out_halfedges, int32_t *out_loop,
                               int32_t *out_loop_edges, uint32_t *out_status, void *scratch, hipStream_t st)
{
    const FillScratch s = fill_layout((size_t)V, (size_t)T, scratch);
    int sorted = 0;
    const int rc = fill_loops(V, T, faces, in_counts, out_halfedges, out_loop, s, &sorted, st);
    if (rc) return rc;
    hipLaunchKernelGGL(fill_lengths_kernel, grid_for((size_t)T, kFillThreads), dim3(kFillThreads), 0, st, (uint32_t)T, (const uint32_t *)s.hdr,
                       (const uint32_t *)s.loop_start, out_loop_edges);
    SLS_LAUNCH_CHECK("fill_lengths_kernel");
    hipLaunchKernelGGL(fill_decide_kernel, dim3(1), dim3(64), 0, st, s.hdr, (const uint64_t *)s.total, 0u, 0u, 0, out_status);
    SLS_LAUNCH_CHECK("fill_decide_kernel");
    return SLS_OK;
}

int launch_mesh_fill_holes(int V, const float *vertices, int T, const int32_t *faces, const uint32_t *in_counts, int max_edges,
                           double max_size, int cap_vertices, float *out_vertices, int cap_triangles, int32_t *out_faces,
                           uint32_t *out_status, void *scratch, hipStream_t st)
{
    const FillScratch s = fill_layout((size_t)V, (size_t)T, scratch);
    const uint32_t n = 3u * (uint32_t)T;
    int sorted = 0;
    int rc = fill_loops(V, T, faces, in_counts, nullptr, nullptr, s, &sorted, st);
    if (rc) return rc;
    VerdictArgs v;
    v.n = n; v.V = (uint32_t)V; v.max_loops = (uint32_t)T; v.max_edges = (uint32_t)max_edges; v.max_size = max_size;
    v.loop_start = s.loop_start; v.sv = s.k[sorted + 1]; v.ha = s.ha; v.xyz = vertices;
    v.verdict = s.verdict; v.centroid = s.centroid; v.needs = s.needs;
    hipLaunchKernelGGL(fill_verdict_short_kernel, grid_for((size_t)T, kFillThreads), dim3(kFillThreads), 0, st, v, s.hdr);
    SLS_LAUNCH_CHECK("fill_verdict_short_kernel");
    const size_t long_blocks = ((size_t)T / (SLS_FILL_LONG + 1) + kFillLongThreads / 64) / (kFillLongThreads / 64);    // a long loop takes 65 half-edges at least
    hipLaunchKernelGGL(fill_verdict_long_kernel, dim3((unsigned)(long_blocks < (size_t)kFillLongBlocks ? long_blocks : (size_t)kFillLongBlocks)),
                       dim3(kFillLongThreads), 0, st, v, s.hdr);
    SLS_LAUNCH_CHECK("fill_verdict_long_kernel");
    rc = fill_scan<uint64_t>((uint32_t)T, s.needs, s.blk, s.total, st);
    if (rc) return rc;
    hipLaunchKernelGGL(fill_decide_kernel, dim3(1), dim3(64), 0, st, s.hdr, (const uint64_t *)s.total, (uint32_t)cap_vertices,
                       (uint32_t)cap_triangles, 1, out_status);
    SLS_LAUNCH_CHECK("fill_decide_kernel");
    const size_t words = 3 * (size_t)(cap_triangles > V ? cap_triangles : V);
    hipLaunchKernelGGL(fill_copy_kernel, grid_for(words, kFillThreads), dim3(kFillThreads), 0, st, (uint32_t)V, (uint32_t)T, (uint32_t)cap_triangles, 0u, 0u,
                       (const uint32_t *)s.hdr, (const uint32_t *)nullptr, (const uint32_t *)vertices, faces, (uint32_t *)out_vertices, out_faces);
    SLS_LAUNCH_CHECK("fill_copy_kernel");
    WriteArgs w;
    w.n = n; w.V = (uint32_t)V; w.max_loops = (uint32_t)T; w.cap_vertices = (uint32_t)cap_vertices; w.cap_triangles = (uint32_t)cap_triangles;
    w.hdr = s.hdr; w.loop_start = s.loop_start; w.sv = s.k[sorted + 1]; w.ha = s.ha; w.hb = s.hb; w.first_out = s.first_out;
    w.verdict = s.verdict; w.ploop = s.ploop; w.centroid = s.centroid; w.offsets = s.needs;
    w.out_vertices = out_vertices; w.out_faces = out_faces;
    hipLaunchKernelGGL(fill_write_kernel, grid_for(n, kFillThreads), dim3(kFillThreads), 0, st, w);
    SLS_LAUNCH_CHECK("fill_write_kernel");
    return SLS_OK;
}

// V == 0 or T == 0: the status alone, and for the fill the live rows and the -1 padding
int launch_mesh_fill_empty(int V, const float *vertices, int T, const int32_t *faces, const uint32_t *in_counts, int fills,
                           float *out_vertices, int cap_triangles, int32_t *out_faces, uint32_t *out_status, hipStream_t st)
{
    if (out_status) {
        hipLaunchKernelGGL(fill_empty_status_kernel, dim3(1), dim3(64), 0, st, (uint32_t)V, (uint32_t)T, in_counts, fills, out_status);
        SLS_LAUNCH_CHECK("fill_empty_status_kernel");
    }
    const size_t words = 3 * (size_t)(cap_triangles > V ? cap_triangles : V);
    if (fills && words) {
        hipLaunchKernelGGL(fill_copy_kernel, grid_for(words, kFillThreads), dim3(kFillThreads), 0, st, (uint32_t)V, (uint32_t)T, (uint32_t)cap_triangles,
                           (uint32_t)V, (uint32_t)T, (const uint32_t *)nullptr, in_counts, (const uint32_t *)vertices, faces,
                           (uint32_t *)out_vertices, out_faces);
        SLS_LAUNCH_CHECK("fill_copy_kernel");
    }
    return SLS_OK;
}

}  // namespace sls
