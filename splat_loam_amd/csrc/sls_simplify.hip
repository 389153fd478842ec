// sls_simplify.hip — simplifying a mesh on the device by vertex clustering (sls_mesh_simplify): the vertices of a voxel
// become one vertex, at their mean or at the minimum of the voxel's error quadric, and the faces are mapped, collapsed and
// de-duplicated.  include/sls_simplify_math.h states every rule, tests/simplify_ref.py restates it in NumPy; DESIGN.md
// section 2, "Mesh simplification", states the contract.  Built EXACT (-ffp-contract=off): the bits of the positions are
// part of the contract.  No floating-point atomics, no hash table, nothing read back.
//
// Launches ordered by the stream alone, every array at the capacity of the input (V vertices, T triangles):
//   simp_init / _mark / _bbox   live flags (a vertex a non-degenerate triangle references; every writer stores 1), the
//                               float32 minimum over the finite live vertices (integer atomicMin in the ordered domain)
//   simp_keys + the stable sort key = ix | iy << 21 | iz << 42 per finite live vertex, bit 63 alone for every other one
//                               (sorted behind all clusters); 64 key bits over (u64 key, u32 vertex) pairs: a cluster's
//                               vertices stay in ascending index
//   simp_vheads / _vscan / _vsegments   head flags of the sorted keys, their scan in chunks of 2048 positions, the
//                               segment of every cluster and cid[v], the cluster of vertex v (-1: none)
//   simp_faces + two stable sorts       the rotated cluster triple of every triangle ((-1,-1,-1): dropped), sorted by its
//                               last entry, then by the first two (u64 keys of bits(V) and 2 bits(V) bits)
//   simp_dedupe                 a triangle whose predecessor in that order holds the same triple is a duplicate (stable
//                               sorts: the lowest input index comes first); kept triangles flag their clusters
//   simp_count x 2 / _scan / _cnew / _fwrite / _vmap    two ordered compactions by chunked scans: surviving clusters,
//                               kept triangles
//   simp_corner_keys + a stable sort    (quadric) corner 3 t + k under the cluster of its vertex, V for a corner that
//                               adds nothing: a cluster's corners in ascending corner id
//   simp_place                  a lane per cluster: the mean over its vertex segment, the quadric sums over its corner
//                               run (found by bisection), the solve; a segment of more than 64 items is left to the
//                               whole wave afterwards (lane l adds l, l + 64, ..., then a fixed xor butterfly)
//   simp_status                 the eight status words
// Timed (sls_timing_enable): the groups simp_cluster, simp_faces, simp_corners, simp_place; the sorts under sort_*.
#include "sls_geom.hpp"
#include "sls_scan.hpp"
#include "../../include/sls_simplify_math.h"

namespace sls {

constexpr int kSimpThreads = 512;
using SimpChunks = Chunks<kSimpThreads, 4>;                 // the chunked scans: 2048 positions per workgroup
constexpr int kSimpPlaceThreads = 256;
constexpr uint64_t kSimpNoKey = 1ull << 63;                 // the key of a vertex that belongs to no cluster
constexpr int kSimpKeyBits = 64;

// hdr words
enum { SH_MIN = 0, SH_NONFINITE = 3, SH_BIG = 4, SH_COLLAPSED = 5, SH_DUPLICATES = 6, SH_FALLBACKS = 7, SH_NV = 8, SH_NT = 9,
       SH_N3T = 10, SH_NC = 11, SH_VOUT = 12, SH_TOUT = 13 };

__global__ void simp_init_kernel(uint32_t *hdr, uint32_t V, uint32_t T)
{
    const uint32_t i = threadIdx.x;
    if (i < 16) hdr[i] = i < 3 ? 0xFFFFFFFFu : i == SH_NV ? V : i == SH_NT ? T : i == SH_N3T ? 3u * T : 0u;
}

__global__ __launch_bounds__(kSimpThreads) void simp_mark_kernel(int T, const int32_t *__restrict__ faces, int V, uint32_t *vlive)
{
    const size_t t = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (t >= (size_t)T) return;
    const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
    if (sls_mesh_degenerate(f, V)) return;
    vlive[f[0]] = 1u; vlive[f[1]] = 1u; vlive[f[2]] = 1u;      // (every writer stores 1; the indices are inside [0, V))
}

__global__ __launch_bounds__(kSimpThreads) void simp_bbox_kernel(uint32_t V, const float *__restrict__ xyz,
                                                                 const uint32_t *__restrict__ vlive, uint32_t *hdr)
{
    bbox_min<kSimpThreads>(V, xyz, vlive, hdr + SH_MIN, hdr + SH_NONFINITE);
}

__global__ __launch_bounds__(kSimpThreads) void simp_keys_kernel(uint32_t V, const float *__restrict__ xyz,
                                                                 const uint32_t *__restrict__ vlive, double voxel_size, uint32_t *hdr,
                                                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    bool big = false;
    if (i < (size_t)V) {
        uint64_t key = kSimpNoKey;
        if (vlive[i] && finite_row(xyz, i)) {                 // (then the minima are finite too)
            const double ox = sls_voxel_origin(ord2f(hdr[SH_MIN + 0]), voxel_size),
                         oy = sls_voxel_origin(ord2f(hdr[SH_MIN + 1]), voxel_size),
                         oz = sls_voxel_origin(ord2f(hdr[SH_MIN + 2]), voxel_size);
            big = !sls_voxel_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ox, oy, oz, voxel_size, &key);
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    const uint64_t m = __ballot(big);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&hdr[SH_BIG], (uint32_t)__popcll(m));
}

// the head flags of this thread's four consecutive sorted positions, as a bit mask (the run of kSimpNoKey has one too)
__device__ __forceinline__ uint32_t simp_head_mask(uint32_t V, const uint64_t *__restrict__ keys, uint32_t p0)
{
    return SimpChunks::head_mask(V, p0, [&](uint32_t p) { return keys[p]; });
}

__global__ __launch_bounds__(kSimpThreads) void simp_vheads_kernel(uint32_t V, const uint64_t *__restrict__ keys, uint32_t *__restrict__ blk)
{
    SimpChunks::total((uint32_t)__popc(simp_head_mask(V, keys, SimpChunks::first())), blk);
}

// seg_start holds V + 1 entries: heads <= V
__global__ __launch_bounds__(kSimpThreads) void simp_vscan_kernel(uint32_t V, int nblk, uint32_t *blk, const uint64_t *__restrict__ keys,
                                                                  uint32_t *__restrict__ hdr, uint32_t *__restrict__ seg_start)
{
    const uint32_t heads = SimpChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) {
        const uint32_t h = heads <= V ? heads : V;              // (always: a head per position at most)
        seg_start[h] = V;
        hdr[SH_NC] = (h > 0u && keys[V - 1u] == kSimpNoKey) ? h - 1u : h;     // (the last run is the one of no cluster)
    }
}

__global__ __launch_bounds__(kSimpThreads) void simp_vsegments_kernel(uint32_t V, const uint64_t *__restrict__ keys,
                                                                      const uint32_t *__restrict__ order, const uint32_t *__restrict__ blk,
                                                                      uint32_t *__restrict__ seg_start, int32_t *__restrict__ cid)
{
    const uint32_t p0 = SimpChunks::first();
    const uint32_t mask = simp_head_mask(V, keys, p0);
    uint32_t id = SimpChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < SimpChunks::kPer; ++j) {
        const uint32_t p = p0 + (uint32_t)j;
        if (p < V) {
            if ((mask >> j) & 1u) {
                if (id < V) seg_start[id] = p;                  // (always: ids are below the number of heads <= V)
                ++id;
            }
            const uint32_t v = min(order[p], V - 1u);           // (a permutation of [0, V): the clamp never bites)
            cid[v] = keys[p] == kSimpNoKey ? -1 : (int32_t)(id - 1u);       // (position 0 is a head: id >= 1 here)
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// faces
// ---------------------------------------------------------------------------------------------------------------------
// rf[t] = the rotated cluster triple, (-1, -1, -1) for a dropped triangle; the first sort's pairs (last entry, t)
__global__ __launch_bounds__(kSimpThreads) void simp_faces_kernel(int T, const int32_t *__restrict__ faces, int V,
                                                                  const int32_t *__restrict__ cid, uint32_t *hdr, int32_t *__restrict__ rf,
                                                                  uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const size_t t = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    bool collapsed = false;
    if (t < (size_t)T) {
        const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
        int32_t r[3] = { -1, -1, -1 };
        if (sls_mesh_degenerate(f, V) == 0) {
            const int32_t c[3] = { cid[f[0]], cid[f[1]], cid[f[2]] };
            if (c[0] >= 0 && c[1] >= 0 && c[2] >= 0) {
                collapsed = sls_simplify_rotate(c, r) != 0;
                if (collapsed) { r[0] = -1; r[1] = -1; r[2] = -1; }
            }
        }
        rf[3 * t] = r[0]; rf[3 * t + 1] = r[1]; rf[3 * t + 2] = r[2];
        keys[t] = r[0] < 0 ? (uint64_t)0 : (uint64_t)(uint32_t)r[2];
        vals[t] = (uint32_t)t;
    }
    const uint64_t m = __ballot(collapsed);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&hdr[SH_COLLAPSED], (uint32_t)__popcll(m));
}

// the second sort's keys: first << bits | second of the triangle at sorted position j (0 for a dropped one: a kept
// triple never has two equal entries, so no kept triangle shares that key)
__global__ __launch_bounds__(kSimpThreads) void simp_face_keys_kernel(uint32_t T, const int32_t *__restrict__ rf,
                                                                      const uint32_t *__restrict__ vals, int bits, uint64_t *__restrict__ keys)
{
    const size_t j = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (j >= T) return;
    const size_t t = min(vals[j], T - 1u);                      // (a permutation of [0, T): the clamp never bites)
    const int32_t a = rf[3 * t], b = rf[3 * t + 1];
    keys[j] = a < 0 ? (uint64_t)0 : (((uint64_t)(uint32_t)a << bits) | (uint64_t)(uint32_t)b);
}

__global__ __launch_bounds__(kSimpThreads) void simp_dedupe_kernel(uint32_t T, uint32_t V, const int32_t *__restrict__ rf,
                                                                   const uint32_t *__restrict__ vals, uint32_t *__restrict__ kept,
                                                                   uint32_t *csurv, uint32_t *hdr)
{
    const size_t j = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    bool dup = false;
    if (j < T) {
        const size_t t = min(vals[j], T - 1u);
        const int32_t r[3] = { rf[3 * t], rf[3 * t + 1], rf[3 * t + 2] };
        uint32_t keep = 0u;
        if (r[0] >= 0) {
            if (j > 0) {
                const size_t u = min(vals[j - 1], T - 1u);
                dup = rf[3 * u] == r[0] && rf[3 * u + 1] == r[1] && rf[3 * u + 2] == r[2];
            }
            keep = dup ? 0u : 1u;
        }
        kept[t] = keep;
        if (keep && (uint32_t)r[0] < V && (uint32_t)r[1] < V && (uint32_t)r[2] < V) {       // (always: cluster ids are below V)
            csurv[r[0]] = 1u; csurv[r[1]] = 1u; csurv[r[2]] = 1u;                          // (every writer stores 1)
        }
    }
    const uint64_t m = __ballot(dup);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&hdr[SH_DUPLICATES], (uint32_t)__popcll(m));
}

// ---------------------------------------------------------------------------------------------------------------------
// the two ordered compactions
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSimpThreads) void simp_count_kernel(uint32_t n, const uint32_t *__restrict__ flag, uint32_t *__restrict__ blk)
{
    SimpChunks::total((uint32_t)__popc(SimpChunks::flag_mask(n, flag, SimpChunks::first())), blk);
}

__global__ __launch_bounds__(kSimpThreads) void simp_scan_kernel(int nblk_t, uint32_t *blk_t, int nblk_v, uint32_t *blk_v,
                                                                 uint32_t *__restrict__ hdr)
{
    __shared__ uint32_t s_wave_t[kSimpThreads / 64], s_wave_v[kSimpThreads / 64];
    const uint32_t nt = scan_in_place<uint32_t, kSimpThreads>(blk_t, blk_t, nblk_t, s_wave_t);
    const uint32_t nv = scan_in_place<uint32_t, kSimpThreads>(blk_v, blk_v, nblk_v, s_wave_v);
    if (threadIdx.x == 0) { hdr[SH_VOUT] = nv; hdr[SH_TOUT] = nt; }
}

// cnew[c] = the output vertex of surviving cluster c (entries of the others stay unwritten and are never read)
__global__ __launch_bounds__(kSimpThreads) void simp_cnew_kernel(uint32_t V, const uint32_t *__restrict__ csurv,
                                                                 const uint32_t *__restrict__ blk, uint32_t *__restrict__ cnew)
{
    const uint32_t c0 = SimpChunks::first();
    const uint32_t mask = SimpChunks::flag_mask(V, csurv, c0);
    uint32_t id = SimpChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < SimpChunks::kPer; ++j)
        if ((mask >> j) & 1u) cnew[c0 + (uint32_t)j] = id++;
}

__global__ __launch_bounds__(kSimpThreads) void simp_fwrite_kernel(uint32_t T, uint32_t V, const uint32_t *__restrict__ kept,
                                                                   const uint32_t *__restrict__ blk, const int32_t *__restrict__ rf,
                                                                   const uint32_t *__restrict__ cnew, int32_t *__restrict__ out_faces)
{
    const uint32_t t0 = SimpChunks::first();
    const uint32_t mask = SimpChunks::flag_mask(T, kept, t0);
    uint32_t id = SimpChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < SimpChunks::kPer; ++j)
        if ((mask >> j) & 1u) {                     // (id < T: the output holds T rows; a kept triple lies inside [0, V))
            const size_t t = t0 + (uint32_t)j;
#pragma unroll
            for (int k = 0; k < 3; ++k) out_faces[3 * (size_t)id + k] = (int32_t)cnew[min((uint32_t)rf[3 * t + k], V - 1u)];
            ++id;
        }
}

__global__ __launch_bounds__(kSimpThreads) void simp_vmap_kernel(uint32_t V, const int32_t *__restrict__ cid,
                                                                 const uint32_t *__restrict__ csurv, const uint32_t *__restrict__ cnew,
                                                                 int32_t *__restrict__ vmap)
{
    const size_t v = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (v >= V) return;
    const int32_t c = cid[v];
    vmap[v] = (c >= 0 && (uint32_t)c < V && csurv[c]) ? (int32_t)cnew[c] : -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// positions
// ---------------------------------------------------------------------------------------------------------------------
// the key of corner 3 t + k: the cluster of its vertex, or V for a corner of a triangle that is degenerate or has a vertex
// without a cluster (sorted behind every cluster)
__global__ __launch_bounds__(kSimpThreads) void simp_corner_keys_kernel(int T, const int32_t *__restrict__ faces, int V,
                                                                        const int32_t *__restrict__ cid, uint32_t *__restrict__ keys,
                                                                        uint32_t *__restrict__ vals)
{
    const size_t t = (size_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (t >= (size_t)T) return;
    const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
    int32_t c[3] = { -1, -1, -1 };
    if (sls_mesh_degenerate(f, V) == 0) { c[0] = cid[f[0]]; c[1] = cid[f[1]]; c[2] = cid[f[2]]; }
    const bool adds = c[0] >= 0 && c[1] >= 0 && c[2] >= 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        keys[3 * t + k] = adds ? (uint32_t)c[k] : (uint32_t)V;
        vals[3 * t + k] = (uint32_t)(3 * t + k);
    }
}

// The sums of include/sls_simplify_math.h, "the order of every float64 sum": every lane owns the segment [s, e) of its
// own cluster (active lanes only) and ends with acc = its N sums.  add(p, acc) adds item p.  Called by whole waves.
template <int N, typename F>
__device__ __forceinline__ void simp_segment_sums(uint32_t s, uint32_t e, bool active, F add, double acc[N])
{
    const int lane = threadIdx.x & 63;
    const uint32_t len = e - s;
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if (active && len <= (uint32_t)SLS_SIMPLIFY_LONG)
        for (uint32_t p = s; p < e; ++p) add(p, acc);
    uint64_t longs = __ballot(active && len > (uint32_t)SLS_SIMPLIFY_LONG);
    while (longs) {                                             // (wave-uniform)
        const int src = (int)__builtin_ctzll(longs);
        longs &= longs - 1ull;
        const uint32_t s0 = (uint32_t)__shfl((int)s, src, 64), e0 = (uint32_t)__shfl((int)e, src, 64);
        double part[N];
#pragma unroll
        for (int k = 0; k < N; ++k) part[k] = 0.0;
        for (uint32_t p = s0 + (uint32_t)lane; p < e0; p += 64u) add(p, part);
        xor_butterfly<N>(part);
        if (lane == src) {
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] = part[k];
        }
    }
}

__global__ __launch_bounds__(kSimpPlaceThreads) void simp_place_kernel(uint32_t V, uint32_t T, const float *__restrict__ xyz,
                                                                       const int32_t *__restrict__ faces, const uint32_t *__restrict__ order,
                                                                       const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ csurv,
                                                                       const uint32_t *__restrict__ cnew, const uint32_t *__restrict__ ckeys,
                                                                       const uint32_t *__restrict__ cvals, int contraction, double lambda,
                                                                       double voxel_size, uint32_t *hdr, float *__restrict__ out_vertices)
{
    const uint32_t nc = min(hdr[SH_NC], V);
    const uint32_t c = blockIdx.x * (uint32_t)kSimpPlaceThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (c - (uint32_t)lane >= nc) return;                       // (wave-uniform: the whole wave lies beyond the clusters)
    const bool active = c < nc && csurv[c] != 0u;
    uint32_t s = 0u, e = 0u;
    if (active) {
        e = min(seg_start[c + 1], V);
        s = min(seg_start[c], e);
    }
    double m[3];
    simp_segment_sums<3>(s, e, active, [&](uint32_t p, double *a) {
        const size_t i = min(order[p], V - 1u);                 // (a permutation of [0, V): the clamp never bites)
        a[0] += (double)xyz[3 * i]; a[1] += (double)xyz[3 * i + 1]; a[2] += (double)xyz[3 * i + 2];
    }, m);
    const uint32_t count = e - s;
    bool fell = false;
    float out[3] = { 0.0f, 0.0f, 0.0f };
    if (active && count) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { m[k] = sls_simplify_mean(m[k], count); out[k] = (float)m[k]; }
    }
    if (contraction == 1) {                                     // (uniform)
        const uint32_t n = 3u * T;
        uint32_t lo = 0u, hi = 0u;
        if (active) {                                           // the run of corners under key c: [lo, hi)
            uint32_t a = 0u, b = n;
            while (a < b) { const uint32_t mid = a + ((b - a) >> 1); if (ckeys[mid] < c) a = mid + 1u; else b = mid; }
            lo = a; b = n;
            while (a < b) { const uint32_t mid = a + ((b - a) >> 1); if (ckeys[mid] <= c) a = mid + 1u; else b = mid; }
            hi = a;
        }
        double q[9];
        simp_segment_sums<9>(lo, hi, active, [&](uint32_t p, double *a) {
            const uint32_t corner = min(cvals[p], n - 1u);      // (a permutation of [0, 3 T))
            const size_t t = corner / 3u;
            const uint32_t i0 = (uint32_t)faces[3 * t], i1 = (uint32_t)faces[3 * t + 1], i2 = (uint32_t)faces[3 * t + 2];
            if (i0 >= V || i1 >= V || i2 >= V) return;          // (never: such a corner carries the key V)
            const float p0[3] = { xyz[3 * (size_t)i0], xyz[3 * (size_t)i0 + 1], xyz[3 * (size_t)i0 + 2] };
            const float p1[3] = { xyz[3 * (size_t)i1], xyz[3 * (size_t)i1 + 1], xyz[3 * (size_t)i1 + 2] };
            const float p2[3] = { xyz[3 * (size_t)i2], xyz[3 * (size_t)i2 + 1], xyz[3 * (size_t)i2 + 2] };
            double w[9];
            if (sls_simplify_quadric(p0, p1, p2, w)) {
#pragma unroll
                for (int k = 0; k < 9; ++k) a[k] += w[k];
            }
        }, q);
        if (active && count) fell = sls_simplify_solve(q, m, lambda, voxel_size, out) != 0;
    }
    if (active && count) {
        const size_t o = min(cnew[c], V - 1u);                  // (the rank of a surviving cluster: below V)
        out_vertices[3 * o] = out[0]; out_vertices[3 * o + 1] = out[1]; out_vertices[3 * o + 2] = out[2];
    }
    const uint64_t mf = __ballot(fell);
    if (mf && lane == 0) atomicAdd(&hdr[SH_FALLBACKS], (uint32_t)__popcll(mf));
}

__global__ void simp_status_kernel(const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    if (threadIdx.x == 0) {
        status[0] = hdr[SH_VOUT]; status[1] = hdr[SH_TOUT]; status[2] = hdr[SH_NONFINITE]; status[3] = hdr[SH_BIG];
        status[4] = hdr[SH_COLLAPSED]; status[5] = hdr[SH_DUPLICATES]; status[6] = hdr[SH_FALLBACKS]; status[7] = 1u;
    }
}

// scratch layout (all 256-byte aligned)
struct SimplifyScratch {
    uint32_t *hdr, *vlive, *vvals, *vvals_tmp, *seg_start, *csurv, *cnew, *fvals, *fvals_tmp, *kept, *ckeys, *ckeys_tmp, *cvals,
        *cvals_tmp, *blk_v, *blk_t;
    uint64_t *vkeys, *vkeys_tmp, *fkeys, *fkeys_tmp;
    int32_t *cid, *rf, *vmap;
    void *sort;
    size_t sort_bytes, total;
    int nblk_v, nblk_t;
};

static SimplifyScratch simplify_layout(size_t V, size_t T, void *base)
{
    SimplifyScratch s;
    Arena a(base);
    s.nblk_v = SimpChunks::count(V); s.nblk_t = SimpChunks::count(T);
    s.hdr = a.take<uint32_t>(16);
    s.vlive = a.take<uint32_t>(V);
    s.vkeys = a.take<uint64_t>(V);
    s.vkeys_tmp = a.take<uint64_t>(V);
    s.vvals = a.take<uint32_t>(V);
    s.vvals_tmp = a.take<uint32_t>(V);
    s.seg_start = a.take<uint32_t>(V + 1);
    s.cid = a.take<int32_t>(V);
    s.vmap = a.take<int32_t>(V);
    s.csurv = a.take<uint32_t>(V);
    s.cnew = a.take<uint32_t>(V);
    s.rf = a.take<int32_t>(3 * T);
    s.fkeys = a.take<uint64_t>(T);
    s.fkeys_tmp = a.take<uint64_t>(T);
    s.fvals = a.take<uint32_t>(T);
    s.fvals_tmp = a.take<uint32_t>(T);
    s.kept = a.take<uint32_t>(T);
    s.ckeys = a.take<uint32_t>(3 * T);
    s.ckeys_tmp = a.take<uint32_t>(3 * T);
    s.cvals = a.take<uint32_t>(3 * T);
    s.cvals_tmp = a.take<uint32_t>(3 * T);
    s.blk_v = a.take<uint32_t>((size_t)s.nblk_v);
    s.blk_t = a.take<uint32_t>((size_t)s.nblk_t);
    s.sort_bytes = sort_scratch_bytes((uint64_t)(V > 3 * T ? V : 3 * T));
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t mesh_simplify_scratch_bytes(int V, int T)
{
    return mesh_sizes_ok(V, T) ? simplify_layout((size_t)V, (size_t)T, nullptr).total : 0;
}

int launch_mesh_simplify(int V, const float *vertices, int T, const int32_t *faces, double voxel_size, int contraction,
                         double regularisation, float *out_vertices, int32_t *out_faces, int32_t *out_vmap, uint32_t *out_status,
                         void *scratch, hipStream_t st)
{
    const SimplifyScratch s = simplify_layout((size_t)V, (size_t)T, scratch);
    const uint32_t Vu = (uint32_t)V, Tu = (uint32_t)T, n3 = 3u * Tu;
    const int bits = sls_mesh_index_bits(V);
    int32_t *vmap = out_vmap ? out_vmap : s.vmap;
    int which = 0, rc;
    ScopedTimer tm_cluster(T_SIMP_CLUSTER, st);
    SLS_HIP_CHECK(hipMemsetAsync(s.vlive, 0, sizeof(uint32_t) * (size_t)V, st));
    SLS_HIP_CHECK(hipMemsetAsync(s.csurv, 0, sizeof(uint32_t) * (size_t)V, st));
    hipLaunchKernelGGL(simp_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, Vu, Tu);
    SLS_LAUNCH_CHECK("simp_init_kernel");
    hipLaunchKernelGGL(simp_mark_kernel, grid_for((size_t)T, kSimpThreads), dim3(kSimpThreads), 0, st, T, faces, V, s.vlive);
    SLS_LAUNCH_CHECK("simp_mark_kernel");
    const unsigned nbv = grid_for((size_t)V, kSimpThreads).x;
    hipLaunchKernelGGL(simp_bbox_kernel, dim3(nbv < 1024u ? nbv : 1024u), dim3(kSimpThreads), 0, st, Vu, vertices,
                       (const uint32_t *)s.vlive, s.hdr);
    SLS_LAUNCH_CHECK("simp_bbox_kernel");
    hipLaunchKernelGGL(simp_keys_kernel, grid_for((size_t)V, kSimpThreads), dim3(kSimpThreads), 0, st, Vu, vertices, (const uint32_t *)s.vlive,
                       voxel_size, s.hdr, s.vkeys, s.vvals);
    SLS_LAUNCH_CHECK("simp_keys_kernel");
    tm_cluster.end_now();
    rc = radix_sort_pairs_u64(s.vkeys, s.vvals, s.vkeys_tmp, s.vvals_tmp, s.hdr + SH_NV, Vu, kSimpKeyBits, s.sort, s.sort_bytes, &which, st);
    if (rc) return rc;
    const uint64_t *vkeys = which ? s.vkeys_tmp : s.vkeys;
    const uint32_t *order = which ? s.vvals_tmp : s.vvals;
    ScopedTimer tm_segments(T_SIMP_CLUSTER, st);
    hipLaunchKernelGGL(simp_vheads_kernel, dim3(s.nblk_v), dim3(kSimpThreads), 0, st, Vu, vkeys, s.blk_v);
    SLS_LAUNCH_CHECK("simp_vheads_kernel");
    hipLaunchKernelGGL(simp_vscan_kernel, dim3(1), dim3(kSimpThreads), 0, st, Vu, s.nblk_v, s.blk_v, vkeys, s.hdr, s.seg_start);
    SLS_LAUNCH_CHECK("simp_vscan_kernel");
    hipLaunchKernelGGL(simp_vsegments_kernel, dim3(s.nblk_v), dim3(kSimpThreads), 0, st, Vu, vkeys, order, (const uint32_t *)s.blk_v,
                       s.seg_start, s.cid);
    SLS_LAUNCH_CHECK("simp_vsegments_kernel");
    tm_segments.end_now();

    ScopedTimer tm_faces(T_SIMP_FACES, st);
    hipLaunchKernelGGL(simp_faces_kernel, grid_for((size_t)T, kSimpThreads), dim3(kSimpThreads), 0, st, T, faces, V, (const int32_t *)s.cid, s.hdr,
                       s.rf, s.fkeys, s.fvals);
    SLS_LAUNCH_CHECK("simp_faces_kernel");
    tm_faces.end_now();
    rc = radix_sort_pairs_u64(s.fkeys, s.fvals, s.fkeys_tmp, s.fvals_tmp, s.hdr + SH_NT, Tu, bits, s.sort, s.sort_bytes, &which, st);
    if (rc) return rc;
    uint64_t *fk[2] = { s.fkeys, s.fkeys_tmp };
    uint32_t *fv[2] = { s.fvals, s.fvals_tmp };
    int cur = which;
    ScopedTimer tm_face_keys(T_SIMP_FACES, st);
    hipLaunchKernelGGL(simp_face_keys_kernel, grid_for((size_t)T, kSimpThreads), dim3(kSimpThreads), 0, st, Tu, (const int32_t *)s.rf,
                       (const uint32_t *)fv[cur], bits, fk[cur]);
    SLS_LAUNCH_CHECK("simp_face_keys_kernel");
    tm_face_keys.end_now();
    rc = radix_sort_pairs_u64(fk[cur], fv[cur], fk[cur ^ 1], fv[cur ^ 1], s.hdr + SH_NT, Tu, 2 * bits, s.sort, s.sort_bytes, &which, st);
    if (rc) return rc;
    cur ^= which;
    ScopedTimer tm_dedupe(T_SIMP_FACES, st);
    hipLaunchKernelGGL(simp_dedupe_kernel, grid_for((size_t)T, kSimpThreads), dim3(kSimpThreads), 0, st, Tu, Vu, (const int32_t *)s.rf,
                       (const uint32_t *)fv[cur], s.kept, s.csurv, s.hdr);
    SLS_LAUNCH_CHECK("simp_dedupe_kernel");

    hipLaunchKernelGGL(simp_count_kernel, dim3(s.nblk_t), dim3(kSimpThreads), 0, st, Tu, (const uint32_t *)s.kept, s.blk_t);
    SLS_LAUNCH_CHECK("simp_count_kernel");
    hipLaunchKernelGGL(simp_count_kernel, dim3(s.nblk_v), dim3(kSimpThreads), 0, st, Vu, (const uint32_t *)s.csurv, s.blk_v);
    SLS_LAUNCH_CHECK("simp_count_kernel");
    hipLaunchKernelGGL(simp_scan_kernel, dim3(1), dim3(kSimpThreads), 0, st, s.nblk_t, s.blk_t, s.nblk_v, s.blk_v, s.hdr);
    SLS_LAUNCH_CHECK("simp_scan_kernel");
    hipLaunchKernelGGL(simp_cnew_kernel, dim3(s.nblk_v), dim3(kSimpThreads), 0, st, Vu, (const uint32_t *)s.csurv,
                       (const uint32_t *)s.blk_v, s.cnew);
    SLS_LAUNCH_CHECK("simp_cnew_kernel");
    hipLaunchKernelGGL(simp_fwrite_kernel, dim3(s.nblk_t), dim3(kSimpThreads), 0, st, Tu, Vu, (const uint32_t *)s.kept,
                       (const uint32_t *)s.blk_t, (const int32_t *)s.rf, (const uint32_t *)s.cnew, out_faces);
    SLS_LAUNCH_CHECK("simp_fwrite_kernel");
    hipLaunchKernelGGL(simp_vmap_kernel, grid_for((size_t)V, kSimpThreads), dim3(kSimpThreads), 0, st, Vu, (const int32_t *)s.cid,
                       (const uint32_t *)s.csurv, (const uint32_t *)s.cnew, vmap);
    SLS_LAUNCH_CHECK("simp_vmap_kernel");
    tm_dedupe.end_now();

    const uint32_t *ckeys = s.ckeys, *cvals = s.cvals;
    if (contraction == 1) {
        ScopedTimer tm_corners(T_SIMP_CORNERS, st);
        hipLaunchKernelGGL(simp_corner_keys_kernel, grid_for((size_t)T, kSimpThreads), dim3(kSimpThreads), 0, st, T, faces, V, (const int32_t *)s.cid,
                           s.ckeys, s.cvals);
        SLS_LAUNCH_CHECK("simp_corner_keys_kernel");
        tm_corners.end_now();
        rc = radix_sort_pairs_u32(s.ckeys, s.cvals, s.ckeys_tmp, s.cvals_tmp, s.hdr + SH_N3T, n3, sls_mesh_index_bits(V + 1), s.sort,
                                  s.sort_bytes, &which, st);
        if (rc) return rc;
        if (which) { ckeys = s.ckeys_tmp; cvals = s.cvals_tmp; }
    }
    ScopedTimer tm_place(T_SIMP_PLACE, st);
    hipLaunchKernelGGL(simp_place_kernel, grid_for(Vu, kSimpPlaceThreads), dim3(kSimpPlaceThreads), 0, st, Vu, Tu,
                       vertices, faces, order, (const uint32_t *)s.seg_start, (const uint32_t *)s.csurv, (const uint32_t *)s.cnew, ckeys,
                       cvals, contraction, regularisation, voxel_size, s.hdr, out_vertices);
    SLS_LAUNCH_CHECK("simp_place_kernel");
    tm_place.end_now();
    hipLaunchKernelGGL(simp_status_kernel, dim3(1), dim3(64), 0, st, (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("simp_status_kernel");
    return SLS_OK;
}

}  // namespace sls
