// sls_smooth.hip — smoothing a mesh on the device over its edge graph (sls_mesh_adjacency, sls_mesh_smooth): the distinct
// neighbours of every vertex in CSR form, then Laplacian, Taubin or simple sweeps that gather them.
// include/sls_smooth_math.h states every rule, tests/smooth_ref.py restates it in NumPy; DESIGN.md section 2, "Mesh
// smoothing", states the contract.  Built EXACT (-ffp-contract=off): the bits of the positions are part of the contract.
// No floating-point atomics, no hash table, nothing read back.
//
// Launches ordered by the stream alone:
//   adj_init / adj_keys + two stable sorts  six directed pairs (a, b) per non-degenerate triangle ((0, 0) for a degenerate
//                               one: sorted in front of every pair), as two u32 arrays: sorted by b with a as the value,
//                               then by a with b as the value (bits(V) key bits each) — the order of a << bits | b at
//                               8 bytes per item and pass instead of 12
//   adj_heads / _scan / _write  head flags of the sorted pairs (a pair that differs from its predecessor), their scan in
//                               chunks of 2048 positions; a head writes its neighbour, flags its row's vertex as a boundary
//                               vertex when its run has length one (every writer stores 1), and every position learns its rank
//   adj_offsets                 offsets[v] = the rank at the lower bound of v in the sorted a
//   adj_rows                    live, boundary and non-finite counts, the largest row, the list of rows above 64 neighbours
//                               (its order is that of an integer atomic and decides nothing: a row's result does not depend
//                               on the other rows)
//   smooth_pack                 positions as float4 (xyz + pad): every gather of a sweep is one 16-byte load
//   smooth_step + smooth_long   one sweep: a lane per vertex for rows of at most 64 neighbours, a wave per row of the
//                               long list (lane l adds l, l + 64, ..., then a fixed xor butterfly); they ping-pong between
//                               two float4 buffers of the scratch, the last sweep writes out_vertices
//   adj_status                  the eight status words
// Timed (sls_timing_enable): the groups smooth_adjacency and smooth_step; the sort under sort_*.
#include "sls_geom.hpp"
#include "sls_scan.hpp"
#include "../../include/sls_smooth_math.h"

namespace sls {

constexpr int kAdjThreads = 512;
using AdjChunks = Chunks<kAdjThreads, 4>;                   // the chunked scan: 2048 positions per workgroup
constexpr int kStepThreads = 256;
constexpr int kLongMaxBlocks = 2048;                        // the long-row kernel strides over the list

// hdr words
enum { AH_N6 = 0, AH_HEADS, AH_LIVE, AH_BOUNDARY, AH_NONFINITE, AH_DEGENERATE, AH_RANGE, AH_MAXROW, AH_NLONG };

// a row above 64 neighbours takes at least 65 of the 6 T directed keys, and there are at most V rows
static size_t adj_long_cap(size_t V, size_t T) { const size_t c = 6 * T / (SLS_SMOOTH_LONG + 1) + 1; return c < V ? c : V; }

__global__ void adj_init_kernel(uint32_t *hdr, uint32_t n6)
{
    const uint32_t i = threadIdx.x;
    if (i < 16) hdr[i] = i == AH_N6 ? n6 : 0u;
}

__global__ __launch_bounds__(kAdjThreads) void adj_keys_kernel(int T, const int32_t *__restrict__ faces, int V, uint32_t *hdr,
                                                               uint32_t *__restrict__ ka, uint32_t *__restrict__ kb)
{
    const size_t t = (size_t)blockIdx.x * kAdjThreads + threadIdx.x;
    int deg = 0;
    if (t < (size_t)T) {
        const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
        deg = sls_mesh_degenerate(f, V);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            int32_t a = 0, b = 0;
            if (!deg) sls_smooth_face_pair(f, j, &a, &b);
            ka[6 * t + j] = (uint32_t)a;
            kb[6 * t + j] = (uint32_t)b;
        }
    }
    count_degenerate(deg, &hdr[AH_DEGENERATE], &hdr[AH_RANGE]);
}

// the head flags of this thread's four consecutive sorted positions, as a bit mask: a pair that differs from its
// predecessor (the zeros of the degenerate triangles come first and form no run)
__device__ __forceinline__ uint32_t adj_head_mask(uint32_t n, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb, uint32_t p0)
{
    return AdjChunks::head_mask(n, p0, [&](uint32_t p) { return pair_key(sa, sb, p); }, 0u);
}

__global__ __launch_bounds__(kAdjThreads) void adj_heads_kernel(uint32_t n, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                                uint32_t *__restrict__ blk)
{
    AdjChunks::total((uint32_t)__popc(adj_head_mask(n, sa, sb, AdjChunks::first())), blk);
}

__global__ __launch_bounds__(kAdjThreads) void adj_scan_kernel(int nblk, uint32_t *blk, uint32_t *__restrict__ hdr)
{
    const uint32_t heads = AdjChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) hdr[AH_HEADS] = heads;
}

// rank[p] = the heads in front of position p; neighbours[rank] = b of every head; boundary[a] = 1 where the head's run ends
// at once (the pair (a, b) appears once: one triangle owns the edge)
__global__ __launch_bounds__(kAdjThreads) void adj_write_kernel(uint32_t n, uint32_t V, const uint32_t *__restrict__ sa,
                                                                const uint32_t *__restrict__ sb, const uint32_t *__restrict__ blk,
                                                                uint32_t *__restrict__ rank, int32_t *__restrict__ neighbours,
                                                                uint8_t *boundary)
{
    const uint32_t p0 = AdjChunks::first();
    const uint32_t mask = adj_head_mask(n, sa, sb, p0);
    uint32_t id = AdjChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < AdjChunks::kPer; ++j) {
        const uint32_t p = p0 + (uint32_t)j;
        if (p < n) {
            rank[p] = id;
            if ((mask >> j) & 1u) {
                const uint64_t k = pair_key(sa, sb, p);
                const uint64_t next = p + 1u < n ? pair_key(sa, sb, p + 1u) : (uint64_t)0;
                if (id < n) neighbours[id] = (int32_t)(uint32_t)k;  // (always: a head per position at most)
                const uint32_t a = (uint32_t)(k >> 32);
                if (next != k && a < V) boundary[a] = 1;            // (a < V always: the pair of a non-degenerate triangle)
                ++id;
            }
        }
    }
}

__global__ __launch_bounds__(kAdjThreads) void adj_offsets_kernel(uint32_t n, uint32_t V, const uint32_t *__restrict__ sa,
                                                                  const uint32_t *__restrict__ rank, const uint32_t *__restrict__ hdr,
                                                                  uint32_t *__restrict__ offsets)
{
    const size_t v = (size_t)blockIdx.x * kAdjThreads + threadIdx.x;
    if (v > V) return;
    const uint32_t heads = min(hdr[AH_HEADS], n);
    uint32_t at = heads;
    if (v < V) {
        const uint32_t target = (uint32_t)v;                    // (the pairs (0, 0) in front are no heads: the rank there is 0)
        uint32_t a = 0u, b = n;
        while (a < b) { const uint32_t mid = a + ((b - a) >> 1); if (sa[mid] < target) a = mid + 1u; else b = mid; }
        if (a < n) at = min(rank[a], heads);
    }
    offsets[v] = at;
}

__global__ __launch_bounds__(kAdjThreads) void adj_rows_kernel(uint32_t V, const uint32_t *__restrict__ offsets,
                                                               const uint8_t *__restrict__ boundary, const float *__restrict__ xyz,
                                                               uint32_t long_cap, uint32_t *hdr, uint32_t *__restrict__ long_rows)
{
    const size_t v = (size_t)blockIdx.x * kAdjThreads + threadIdx.x;
    uint32_t len = 0u;
    bool edge = false, bad = false;
    if (v < V) {
        len = offsets[v + 1] - offsets[v];
        edge = boundary[v] != 0;
        if (xyz && len)
            bad = !(sls_smooth_finite(xyz[3 * v]) && sls_smooth_finite(xyz[3 * v + 1]) && sls_smooth_finite(xyz[3 * v + 2]));
        if (len > (uint32_t)SLS_SMOOTH_LONG) {
            const uint32_t slot = atomicAdd(&hdr[AH_NLONG], 1u);
            if (slot < long_cap) long_rows[slot] = (uint32_t)v;     // (always: adj_long_cap bounds the number of such rows)
        }
    }
    const uint64_t ml = __ballot(len != 0u), me = __ballot(edge), mb = __ballot(bad);
    uint32_t mx = len;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    if ((threadIdx.x & 63) == 0) {
        if (ml) atomicAdd(&hdr[AH_LIVE], (uint32_t)__popcll(ml));
        if (me) atomicAdd(&hdr[AH_BOUNDARY], (uint32_t)__popcll(me));
        if (mb) atomicAdd(&hdr[AH_NONFINITE], (uint32_t)__popcll(mb));
        if (mx) atomicMax(&hdr[AH_MAXROW], mx);
    }
}

__global__ void adj_status_kernel(const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    if (threadIdx.x == 0) {
        status[0] = hdr[AH_LIVE]; status[1] = hdr[AH_HEADS] / 2u; status[2] = hdr[AH_BOUNDARY]; status[3] = hdr[AH_NONFINITE];
        status[4] = hdr[AH_DEGENERATE]; status[5] = hdr[AH_RANGE]; status[6] = hdr[AH_MAXROW]; status[7] = 1u;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the sweeps
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStepThreads) void smooth_pack_kernel(uint32_t V, const float *__restrict__ xyz, float4 *__restrict__ out)
{
    const size_t v = (size_t)blockIdx.x * kStepThreads + threadIdx.x;
    if (v < V) out[v] = make_float4(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], 0.0f);
}

struct StepArgs {
    uint32_t V, n6;                 // vertices; the capacity of the neighbour list
    const float4 *in;
    const uint32_t *offsets;
    const int32_t *neighbours;
    const uint8_t *boundary;
    int simple, weights, fix_boundary;
    double f;
    float4 *out4;                   // the other ping-pong buffer, or null on the last sweep ...
    float *out3;                    // ... which writes packed rows
};

__device__ __forceinline__ void smooth_store(const StepArgs &a, size_t v, const float o[3])
{
    if (a.out4) a.out4[v] = make_float4(o[0], o[1], o[2], 0.0f);
    else { a.out3[3 * v] = o[0]; a.out3[3 * v + 1] = o[1]; a.out3[3 * v + 2] = o[2]; }
}

__device__ __forceinline__ void smooth_item(const StepArgs &a, const float pi[3], uint32_t p, double acc[4])
{
    const size_t nb = min((uint32_t)a.neighbours[p], a.V - 1u);     // (inside [0, V): the clamp never bites)
    const float4 q = a.in[nb];
    const float pn[3] = { q.x, q.y, q.z };
    sls_smooth_add(acc, sls_smooth_weight(pi, pn, a.simple ? SLS_SMOOTH_UNIFORM : a.weights), pn);
}

__device__ __forceinline__ void smooth_result(const StepArgs &a, const float pi[3], const double acc[4], uint32_t len, float o[3])
{
    if (a.simple) sls_smooth_simple(pi, acc, len, o);
    else sls_smooth_step(pi, acc, a.f, o);
}

// a lane per vertex: rows of at most 64 neighbours, and the copies (not live, pinned); longer rows are left to smooth_long
__global__ __launch_bounds__(kStepThreads) void smooth_step_kernel(StepArgs a)
{
    const size_t v = (size_t)blockIdx.x * kStepThreads + threadIdx.x;
    if (v >= a.V) return;
    const float4 p4 = a.in[v];
    const float pi[3] = { p4.x, p4.y, p4.z };
    const uint32_t e = min(a.offsets[v + 1], a.n6), s = min(a.offsets[v], e), len = e - s;
    float o[3] = { pi[0], pi[1], pi[2] };
    if (len && !(a.fix_boundary && a.boundary[v])) {
        if (len > (uint32_t)SLS_SMOOTH_LONG) return;
        double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (uint32_t p = s; p < e; ++p) smooth_item(a, pi, p, acc);
        smooth_result(a, pi, acc, len, o);
    }
    smooth_store(a, v, o);
}

// a wave per row of the long list
__global__ __launch_bounds__(kStepThreads) void smooth_long_kernel(StepArgs a, const uint32_t *__restrict__ hdr,
                                                                   const uint32_t *__restrict__ long_rows, uint32_t long_cap)
{
    const int lane = threadIdx.x & 63;
    const uint32_t nlong = min(hdr[AH_NLONG], long_cap);
    const uint32_t waves = gridDim.x * (uint32_t)(kStepThreads / 64);
    for (uint32_t r = blockIdx.x * (uint32_t)(kStepThreads / 64) + (threadIdx.x >> 6); r < nlong; r += waves) {     // (wave-uniform)
        const size_t v = min(long_rows[r], a.V - 1u);
        if (a.fix_boundary && a.boundary[v]) continue;
        const float4 p4 = a.in[v];
        const float pi[3] = { p4.x, p4.y, p4.z };
        const uint32_t e = min(a.offsets[v + 1], a.n6), s = min(a.offsets[v], e), len = e - s;
        if (len <= (uint32_t)SLS_SMOOTH_LONG) continue;             // (never: the list holds long rows alone)
        double part[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (uint32_t p = s + (uint32_t)lane; p < e; p += 64u) smooth_item(a, pi, p, part);
        xor_butterfly<4>(part);
        if (lane == 0) {
            float o[3];
            smooth_result(a, pi, part, len, o);
            smooth_store(a, v, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// scratch layouts (all 256-byte aligned) and the launchers
// ---------------------------------------------------------------------------------------------------------------------
struct AdjScratch {
    uint32_t *hdr, *ka, *ka_tmp, *kb, *kb_tmp, *blk, *long_rows;
    void *sort;
    size_t sort_bytes, long_cap, total;
    int nblk;
};

static AdjScratch adjacency_layout(size_t V, size_t T, Arena &a)
{
    AdjScratch s;
    const size_t n6 = 6 * T;
    s.nblk = AdjChunks::count(n6);
    s.long_cap = adj_long_cap(V, T);
    s.hdr = a.take<uint32_t>(16);
    s.ka = a.take<uint32_t>(n6);
    s.ka_tmp = a.take<uint32_t>(n6);
    s.kb = a.take<uint32_t>(n6);
    s.kb_tmp = a.take<uint32_t>(n6);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.long_rows = a.take<uint32_t>(s.long_cap);
    s.sort_bytes = sort_scratch_bytes((uint64_t)n6);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

struct SmoothScratch {
    AdjScratch adj;
    uint32_t *offsets;
    int32_t *neighbours;
    uint8_t *boundary;
    float4 *ping, *pong;
    size_t total;
};

static SmoothScratch smooth_layout(size_t V, size_t T, void *base)
{
    SmoothScratch s;
    Arena a(base);
    s.adj = adjacency_layout(V, T, a);
    s.offsets = a.take<uint32_t>(V + 1);
    s.neighbours = a.take<int32_t>(6 * T);
    s.boundary = a.take<uint8_t>(V);
    s.ping = a.take<float4>(V);
    s.pong = a.take<float4>(V);
    s.total = a.off;
    return s;
}

size_t mesh_adjacency_scratch_bytes(int V, int T)
{
    Arena a(nullptr);
    return mesh_sizes_ok(V, T) ? adjacency_layout((size_t)V, (size_t)T, a).total : 0;
}

size_t mesh_smooth_scratch_bytes(int V, int T)
{
    return mesh_sizes_ok(V, T) ? smooth_layout((size_t)V, (size_t)T, nullptr).total : 0;
}

// offsets (V + 1), neighbours (capacity 6 T), boundary (V) and the hdr words; vertices may be null (no non-finite count)
static int adjacency_build(int V, int T, const int32_t *faces, const float *vertices, uint32_t *offsets, int32_t *neighbours,
                           uint8_t *boundary, const AdjScratch &s, hipStream_t st)
{
    const uint32_t Vu = (uint32_t)V, n6 = 6u * (uint32_t)T;
    const int bits = sls_mesh_index_bits(V);
    ScopedTimer tm_keys(T_SMOOTH_ADJACENCY, st);
    SLS_HIP_CHECK(hipMemsetAsync(boundary, 0, (size_t)V, st));
    hipLaunchKernelGGL(adj_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, n6);
    SLS_LAUNCH_CHECK("adj_init_kernel");
    hipLaunchKernelGGL(adj_keys_kernel, grid_for((size_t)T, kAdjThreads), dim3(kAdjThreads), 0, st, T, faces, V, s.hdr, s.ka, s.kb);
    SLS_LAUNCH_CHECK("adj_keys_kernel");
    tm_keys.end_now();
    uint32_t *a2[2] = { s.ka, s.ka_tmp }, *b2[2] = { s.kb, s.kb_tmp };
    int cur = 0;
    const int rc = sort_pairs_ab(a2, b2, s.hdr + AH_N6, n6, bits, s.sort, s.sort_bytes, &cur, st);
    if (rc) return rc;
    const uint32_t *sa = a2[cur], *sb = b2[cur];
    uint32_t *rank = a2[cur ^ 1];                                   // (the other copy is free: its room holds the ranks)
    ScopedTimer tm_rows(T_SMOOTH_ADJACENCY, st);
    hipLaunchKernelGGL(adj_heads_kernel, dim3(s.nblk), dim3(kAdjThreads), 0, st, n6, sa, sb, s.blk);
    SLS_LAUNCH_CHECK("adj_heads_kernel");
    hipLaunchKernelGGL(adj_scan_kernel, dim3(1), dim3(kAdjThreads), 0, st, s.nblk, s.blk, s.hdr);
    SLS_LAUNCH_CHECK("adj_scan_kernel");
    hipLaunchKernelGGL(adj_write_kernel, dim3(s.nblk), dim3(kAdjThreads), 0, st, n6, Vu, sa, sb, (const uint32_t *)s.blk, rank,
                       neighbours, boundary);
    SLS_LAUNCH_CHECK("adj_write_kernel");
    hipLaunchKernelGGL(adj_offsets_kernel, grid_for((size_t)V + 1, kAdjThreads), dim3(kAdjThreads), 0, st, n6, Vu, sa, (const uint32_t *)rank,
                       (const uint32_t *)s.hdr, offsets);
    SLS_LAUNCH_CHECK("adj_offsets_kernel");
    hipLaunchKernelGGL(adj_rows_kernel, grid_for((size_t)V, kAdjThreads), dim3(kAdjThreads), 0, st, Vu, (const uint32_t *)offsets,
                       (const uint8_t *)boundary, vertices, (uint32_t)s.long_cap, s.hdr, s.long_rows);
    SLS_LAUNCH_CHECK("adj_rows_kernel");
    return SLS_OK;
}

int launch_mesh_adjacency(int V, int T, const int32_t *faces, int32_t *out_offsets, int32_t *out_neighbours, uint8_t *out_boundary,
                          uint32_t *out_status, void *scratch, hipStream_t st)
{
    Arena a(scratch);
    const AdjScratch s = adjacency_layout((size_t)V, (size_t)T, a);
    const int rc = adjacency_build(V, T, faces, nullptr, (uint32_t *)out_offsets, out_neighbours, out_boundary, s, st);
    if (rc) return rc;
    hipLaunchKernelGGL(adj_status_kernel, dim3(1), dim3(64), 0, st, (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("adj_status_kernel");
    return SLS_OK;
}

int launch_mesh_smooth(int V, const float *vertices, int T, const int32_t *faces, int method, int weights, int iterations,
                       double lambda, double mu, int fix_boundary, float *out_vertices, uint32_t *out_status, void *scratch,
                       hipStream_t st)
{
    const SmoothScratch s = smooth_layout((size_t)V, (size_t)T, scratch);
    const uint32_t Vu = (uint32_t)V;
    const int rc = adjacency_build(V, T, faces, vertices, s.offsets, s.neighbours, s.boundary, s.adj, st);
    if (rc) return rc;
    hipLaunchKernelGGL(adj_status_kernel, dim3(1), dim3(64), 0, st, (const uint32_t *)s.adj.hdr, out_status);
    SLS_LAUNCH_CHECK("adj_status_kernel");
    const int64_t steps = method == SLS_SMOOTH_TAUBIN ? 2 * (int64_t)iterations : (int64_t)iterations;
    if (steps == 0) {
        SLS_HIP_CHECK(hipMemcpyAsync(out_vertices, vertices, 3 * sizeof(float) * (size_t)V, hipMemcpyDeviceToDevice, st));
        return SLS_OK;
    }
    ScopedTimer tm_step(T_SMOOTH_STEP, st);
    const dim3 grid = grid_for(Vu, kStepThreads);
    const size_t long_blocks = (s.adj.long_cap + kStepThreads / 64 - 1) / (kStepThreads / 64);
    const dim3 grid_long((unsigned)(long_blocks < (size_t)kLongMaxBlocks ? long_blocks : (size_t)kLongMaxBlocks));
    hipLaunchKernelGGL(smooth_pack_kernel, grid, dim3(kStepThreads), 0, st, Vu, vertices, s.ping);
    SLS_LAUNCH_CHECK("smooth_pack_kernel");
    float4 *buf[2] = { s.ping, s.pong };
    StepArgs a;
    a.V = Vu; a.n6 = 6u * (uint32_t)T;
    a.offsets = s.offsets; a.neighbours = s.neighbours; a.boundary = s.boundary;
    a.simple = method == SLS_SMOOTH_SIMPLE; a.weights = weights; a.fix_boundary = fix_boundary;
    for (int64_t k = 0; k < steps; ++k) {
        a.in = buf[k & 1];
        a.f = (method == SLS_SMOOTH_TAUBIN && (k & 1)) ? mu : lambda;
        a.out4 = k + 1 == steps ? nullptr : buf[(k & 1) ^ 1];
        a.out3 = out_vertices;
        hipLaunchKernelGGL(smooth_step_kernel, grid, dim3(kStepThreads), 0, st, a);
        SLS_LAUNCH_CHECK("smooth_step_kernel");
        hipLaunchKernelGGL(smooth_long_kernel, grid_long, dim3(kStepThreads), 0, st, a, (const uint32_t *)s.adj.hdr,
                           (const uint32_t *)s.adj.long_rows, (uint32_t)s.adj.long_cap);
        SLS_LAUNCH_CHECK("smooth_long_kernel");
    }
    return SLS_OK;
}

}  // namespace sls
