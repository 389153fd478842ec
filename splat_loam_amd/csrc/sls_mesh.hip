// sls_mesh.hip — cleaning an extracted mesh on the device: bit-equal vertices merged (sls_mesh_weld), connected
// clusters of triangles and the edge statistics (sls_mesh_clusters), the largest clusters kept and the mesh compacted
// (sls_mesh_filter), area-weighted vertex normals (sls_mesh_vertex_normals).  include/sls_mesh_math.h states every rule,
// tests/mesh_ref.py restates it in NumPy; DESIGN.md section 2, "Mesh cleaning", states the contract.
// Built EXACT (-ffp-contract=off): the bits of the normals are part of the contract.
//
// sls_mesh_weld, launches ordered by the stream alone:
//   mesh_word_keys x 3 + the stable LSD sort x 3   (u32 key, u32 row) pairs over the sign-flipped words z, then y, then
//                               x (sls_radix.hip: radix_sort_pairs_u32, 32 bits each): rows in ascending (x, y, z)
//   weld_heads / _scan / _write head flags of the sorted rows (a row that differs from its predecessor), their scan in
//                               chunks of 2048 positions, the unique rows, the rank of every row and the status words
//
// sls_mesh_clusters:
//   mesh_edges                  three edge keys per triangle (0: a degenerate triangle has none), parent[t] = t, the counts
//                               of degenerate / out-of-range triangles (integer atomics: order-free)
//   the stable LSD sort         2 x bits(V) key bits over (u64 key, u32 edge id 3 t + e) pairs (radix_sort_pairs_u64)
//   mesh_union                  union-find over triangles: equal neighbouring keys unite their two triangles, the larger
//                               root linked under the smaller with a compare-and-swap, so the root of a component is its
//                               lowest triangle whatever the order of execution.  Every access to a parent word is an
//                               agent-scope atomic; no workgroup waits for another; the only retry is a failed
//                               compare-and-swap, and parents only decrease.  Edge statistics from the runs of equal keys.
//   mesh_flatten / _rootscan / _rank / _label   every triangle's root (plain loads: nothing writes parent any more), the
//                               roots ranked in ascending order by a chunked scan, labels, counts by integer atomics
//                               (sls_cluster.hip numbers the clusters of a cloud so: uf_root and uf_kth_largest serve both)
//
// sls_mesh_filter:  mesh_nmin (one workgroup: the k-th largest count by bisection over the value), mesh_mark (kept
//                   triangles flag their vertices), mesh_vcount, mesh_filter_scan, mesh_vwrite, mesh_fwrite: two ordered
//                   compactions by chunked scans, no atomics.
// sls_mesh_vertex_normals:  corners sorted by vertex (stable: ascending triangle within a vertex), then one thread per
//                   vertex finds its run by bisection and sums the face normals in that order.  No float atomics.
#include "sls_geom.hpp"
#include "sls_scan.hpp"
#include "sls_unionfind.hpp"
#include "../../include/sls_mesh_math.h"

namespace sls {

constexpr int kMeshThreads = 512;
using MeshChunks = Chunks<kMeshThreads, 4>;                 // the chunked scans: 2048 positions per workgroup
constexpr uint32_t kMeshNone = 0xFFFFFFFFu;                 // parent / root of a degenerate triangle

enum { MH_COUNT = 0, MH_DEGENERATE = 1, MH_RANGE = 2, MH_BOUNDARY = 3, MH_NONMANIFOLD = 4, MH_NMIN = 5 };   // hdr words


__global__ void mesh_hdr_kernel(uint32_t *hdr, uint32_t n)
{
    if (threadIdx.x < 16) hdr[threadIdx.x] = threadIdx.x == MH_COUNT ? n : 0u;
}

// ---------------------------------------------------------------------------------------------------------------------
// weld
// ---------------------------------------------------------------------------------------------------------------------
// keys[j] = the key of word w of the row at sorted position j (rows_in null: the identity, written to rows_out)
__global__ __launch_bounds__(kMeshThreads) void mesh_word_keys_kernel(uint32_t n, const uint32_t *__restrict__ soup, int w,
                                                                      const uint32_t *rows_in, uint32_t *keys, uint32_t *rows_out)
{
    const size_t j = (size_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = rows_in ? rows_in[j] : (uint32_t)j;
    keys[j] = sls_mesh_word_key(soup[3 * (size_t)r + w]);
    if (!rows_in) rows_out[j] = r;
}

// the three words of a soup row: two rows differ unless they are the same vertex
struct WeldRow {
    uint32_t w[3];
    __device__ __forceinline__ bool operator!=(const WeldRow &o) const { return !sls_mesh_same_row(w, o.w); }
};

// the head flags of this thread's four consecutive sorted positions, as a bit mask
__device__ __forceinline__ uint32_t weld_head_mask(uint32_t n, const uint32_t *__restrict__ soup, const uint32_t *__restrict__ rows,
                                                   uint32_t p0)
{
    return MeshChunks::head_mask(n, p0, [&](uint32_t p) {
        const size_t r = rows[p];
        return WeldRow{ { soup[3 * r], soup[3 * r + 1], soup[3 * r + 2] } };
    });
}

__global__ __launch_bounds__(kMeshThreads) void weld_heads_kernel(uint32_t n, const uint32_t *__restrict__ soup,
                                                                  const uint32_t *__restrict__ rows, uint32_t *__restrict__ blk)
{
    MeshChunks::total((uint32_t)__popc(weld_head_mask(n, soup, rows, MeshChunks::first())), blk);
}

__global__ __launch_bounds__(kMeshThreads) void weld_scan_kernel(int nblk, uint32_t *blk, uint32_t *__restrict__ status)
{
    const uint32_t nv = MeshChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) { status[0] = nv; status[1] = 0u; status[2] = 0u; status[3] = 1u; }
}

__global__ __launch_bounds__(kMeshThreads) void weld_write_kernel(uint32_t n, const uint32_t *__restrict__ soup,
                                                                  const uint32_t *__restrict__ rows, const uint32_t *__restrict__ blk,
                                                                  uint32_t *__restrict__ out_vertices, int32_t *__restrict__ out_index)
{
    const uint32_t p0 = MeshChunks::first();
    const uint32_t mask = weld_head_mask(n, soup, rows, p0);
    uint32_t id = MeshChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j) {
        const uint32_t p = p0 + (uint32_t)j;
        if (p < n) {
            const size_t r = rows[p];
            if ((mask >> j) & 1u) {                 // (id < n always: there are at most n heads, and the output holds n rows)
                out_vertices[3 * (size_t)id] = soup[3 * r]; out_vertices[3 * (size_t)id + 1] = soup[3 * r + 1];
                out_vertices[3 * (size_t)id + 2] = soup[3 * r + 2];
                ++id;
            }
            out_index[r] = (int32_t)(id - 1u);      // (position 0 is always a head: id >= 1 here)
        }
    }
}

// scratch layouts (all 256-byte aligned)
struct MeshSortScratch {
    uint32_t *hdr, *keys, *keys_tmp, *vals, *vals_tmp, *blk;
    void *sort;
    size_t sort_bytes, total;
    int nblk;
};

static MeshSortScratch mesh_sort_layout(size_t n, void *base)
{
    MeshSortScratch s;
    Arena a(base);
    s.nblk = MeshChunks::count(n);
    s.hdr = a.take<uint32_t>(16);
    s.keys = a.take<uint32_t>(n);
    s.keys_tmp = a.take<uint32_t>(n);
    s.vals = a.take<uint32_t>(n);
    s.vals_tmp = a.take<uint32_t>(n);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.sort_bytes = sort_scratch_bytes((uint64_t)n);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t mesh_weld_scratch_bytes(int64_t n_rows)
{
    return (n_rows > 0 && n_rows <= 3 * (int64_t)SLS_MESH_MAX_TRIANGLES) ? mesh_sort_layout((size_t)n_rows, nullptr).total : 0;
}

int launch_mesh_weld(int n_rows, const float *soup, float *out_vertices, int32_t *out_index, uint32_t *out_status, void *scratch,
                     hipStream_t st)
{
    const MeshSortScratch s = mesh_sort_layout((size_t)n_rows, scratch);
    const uint32_t n = (uint32_t)n_rows;
    const uint32_t *words = (const uint32_t *)soup;
    hipLaunchKernelGGL(mesh_hdr_kernel, dim3(1), dim3(64), 0, st, s.hdr, n);
    SLS_LAUNCH_CHECK("mesh_hdr_kernel");
    uint32_t *kb[2] = { s.keys, s.keys_tmp }, *vb[2] = { s.vals, s.vals_tmp };
    int cur = 0;
    for (int w = 2; w >= 0; --w) {                  // LSD over the words: z first
        hipLaunchKernelGGL(mesh_word_keys_kernel, grid_for(n, kMeshThreads), dim3(kMeshThreads), 0, st, n, words, w,
                           w == 2 ? (const uint32_t *)nullptr : (const uint32_t *)vb[cur], kb[cur], vb[cur]);
        SLS_LAUNCH_CHECK("mesh_word_keys_kernel");
        int which = 0;
        const int rc = radix_sort_pairs_u32(kb[cur], vb[cur], kb[cur ^ 1], vb[cur ^ 1], s.hdr + MH_COUNT, n, 32, s.sort, s.sort_bytes,
                                            &which, st);
        if (rc) return rc;
        cur ^= which;
    }
    const uint32_t *rows = vb[cur];
    hipLaunchKernelGGL(weld_heads_kernel, dim3(s.nblk), dim3(kMeshThreads), 0, st, n, words, rows, s.blk);
    SLS_LAUNCH_CHECK("weld_heads_kernel");
    hipLaunchKernelGGL(weld_scan_kernel, dim3(1), dim3(kMeshThreads), 0, st, s.nblk, s.blk, out_status);
    SLS_LAUNCH_CHECK("weld_scan_kernel");
    hipLaunchKernelGGL(weld_write_kernel, dim3(s.nblk), dim3(kMeshThreads), 0, st, n, words, rows, (const uint32_t *)s.blk,
                       (uint32_t *)out_vertices, out_index);
    SLS_LAUNCH_CHECK("weld_write_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// clusters
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshThreads) void mesh_edges_kernel(int T, const int32_t *__restrict__ faces, int V, int bits,
                                                                  uint32_t *hdr, uint64_t *__restrict__ keys,
                                                                  uint32_t *__restrict__ vals, uint32_t *__restrict__ parent)
{
    const size_t t = (size_t)blockIdx.x * kMeshThreads + threadIdx.x;
    int d = 0;
    if (t < (size_t)T) {
        const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
        d = sls_mesh_degenerate(f, V);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            keys[3 * t + e] = d ? (uint64_t)0 : sls_mesh_edge_key(f, e, bits);
            vals[3 * t + e] = (uint32_t)(3 * t + e);
        }
        parent[t] = d ? kMeshNone : (uint32_t)t;
    }
    count_degenerate(d, &hdr[MH_DEGENERATE], &hdr[MH_RANGE]);
}

__global__ __launch_bounds__(kMeshThreads) void mesh_union_kernel(uint32_t n, const uint64_t *__restrict__ keys,
                                                                  const uint32_t *__restrict__ vals, uint32_t *parent, uint32_t *hdr)
{
    const size_t j = (size_t)blockIdx.x * kMeshThreads + threadIdx.x;
    bool boundary = false, nonmanifold = false;
    if (j < n) {
        const uint64_t k = keys[j];
        if (k != 0u) {
            if (j > 0 && keys[j - 1] == k) uf_unite(parent, vals[j] / 3u, vals[j - 1] / 3u);
            else {                                  // the head of a run of equal keys: how long is it?
                const bool two = j + 1 < n && keys[j + 1] == k;
                boundary = !two;
                nonmanifold = two && j + 2 < n && keys[j + 2] == k;
            }
        }
    }
    const uint64_t mb = __ballot(boundary), mn = __ballot(nonmanifold);
    if ((threadIdx.x & 63) == 0) {
        if (mb) atomicAdd(&hdr[MH_BOUNDARY], (uint32_t)__popcll(mb));
        if (mn) atomicAdd(&hdr[MH_NONMANIFOLD], (uint32_t)__popcll(mn));
    }
}

// root[t] of this thread's four consecutive triangles (a launch of its own: parent is only read) and the chunk's roots
__global__ __launch_bounds__(kMeshThreads) void mesh_flatten_kernel(uint32_t T, const uint32_t *__restrict__ parent,
                                                                    uint32_t *__restrict__ root, uint32_t *__restrict__ blk)
{
    const uint32_t t0 = MeshChunks::first();
    uint32_t nroots = 0u;
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j) {
        const uint32_t t = t0 + (uint32_t)j;
        if (t < T) {
            uint32_t x = parent[t];
            if (x != kMeshNone) {
                x = uf_root(parent, x);
                nroots += x == t ? 1u : 0u;
            }
            root[t] = x;
        }
    }
    MeshChunks::total(nroots, blk);
}

__global__ __launch_bounds__(kMeshThreads) void mesh_rootscan_kernel(int nblk, uint32_t *blk, const uint32_t *__restrict__ hdr,
                                                                     uint32_t *__restrict__ status)
{
    const uint32_t nc = MeshChunks::scan_totals(blk, blk, nblk);
    if (threadIdx.x == 0) {
        status[0] = nc; status[1] = hdr[MH_DEGENERATE]; status[2] = hdr[MH_RANGE]; status[3] = hdr[MH_BOUNDARY];
        status[4] = hdr[MH_NONMANIFOLD]; status[5] = 1u;
    }
}

// dense[t] = the rank of root t among the roots; its count starts at 0
__global__ __launch_bounds__(kMeshThreads) void mesh_rank_kernel(uint32_t T, const uint32_t *__restrict__ root,
                                                                 const uint32_t *__restrict__ blk, uint32_t *__restrict__ dense,
                                                                 int32_t *__restrict__ counts)
{
    const uint32_t t0 = MeshChunks::first();
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j) {
        const uint32_t t = t0 + (uint32_t)j;
        if (t < T && root[t] == t) mask |= 1u << j;
    }
    uint32_t id = MeshChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j)
        if ((mask >> j) & 1u) {                     // (id < T: there are at most T roots, and counts holds T entries)
            dense[t0 + (uint32_t)j] = id;
            counts[id] = 0;
            ++id;
        }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_label_kernel(uint32_t T, const uint32_t *__restrict__ root,
                                                                  const uint32_t *__restrict__ dense, int32_t *__restrict__ labels,
                                                                  int32_t *counts)
{
    const size_t t = (size_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= T) return;
    const uint32_t r = root[t];
    if (r == kMeshNone) { labels[t] = -1; return; }
    const uint32_t c = dense[r];
    labels[t] = (int32_t)c;
    atomicAdd(&counts[c], 1);
}

struct MeshClusterScratch {
    uint32_t *hdr;
    uint64_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp, *parent, *root, *dense, *blk;
    void *sort;
    size_t sort_bytes, total;
    int nblk;
};

static MeshClusterScratch mesh_cluster_layout(size_t T, void *base)
{
    MeshClusterScratch s;
    Arena a(base);
    const size_t n = 3 * T;
    s.nblk = MeshChunks::count(T);
    s.hdr = a.take<uint32_t>(16);
    s.keys = a.take<uint64_t>(n);
    s.keys_tmp = a.take<uint64_t>(n);
    s.vals = a.take<uint32_t>(n);
    s.vals_tmp = a.take<uint32_t>(n);
    s.parent = a.take<uint32_t>(T);
    s.root = a.take<uint32_t>(T);
    s.dense = a.take<uint32_t>(T);
    s.blk = a.take<uint32_t>((size_t)s.nblk);
    s.sort_bytes = sort_scratch_bytes((uint64_t)n);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

size_t mesh_clusters_scratch_bytes(int T)
{
    return (T > 0 && T <= SLS_MESH_MAX_TRIANGLES) ? mesh_cluster_layout((size_t)T, nullptr).total : 0;
}

int launch_mesh_clusters(int T, const int32_t *faces, int V, int32_t *out_labels, int32_t *out_counts, uint32_t *out_status,
                         void *scratch, hipStream_t st)
{
    const MeshClusterScratch s = mesh_cluster_layout((size_t)T, scratch);
    const uint32_t n = 3u * (uint32_t)T;
    const int bits = sls_mesh_index_bits(V);
    hipLaunchKernelGGL(mesh_hdr_kernel, dim3(1), dim3(64), 0, st, s.hdr, n);
    SLS_LAUNCH_CHECK("mesh_hdr_kernel");
    hipLaunchKernelGGL(mesh_edges_kernel, grid_for((size_t)T, kMeshThreads), dim3(kMeshThreads), 0, st, T, faces, V, bits, s.hdr, s.keys, s.vals,
                       s.parent);
    SLS_LAUNCH_CHECK("mesh_edges_kernel");
    int which = 0;
    const int rc = radix_sort_pairs_u64(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + MH_COUNT, n, 2 * bits, s.sort, s.sort_bytes,
                                        &which, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_union_kernel, grid_for((size_t)n, kMeshThreads), dim3(kMeshThreads), 0, st, n,
                       (const uint64_t *)(which ? s.keys_tmp : s.keys), (const uint32_t *)(which ? s.vals_tmp : s.vals), s.parent, s.hdr);
    SLS_LAUNCH_CHECK("mesh_union_kernel");
    hipLaunchKernelGGL(mesh_flatten_kernel, dim3(s.nblk), dim3(kMeshThreads), 0, st, (uint32_t)T, (const uint32_t *)s.parent, s.root,
                       s.blk);
    SLS_LAUNCH_CHECK("mesh_flatten_kernel");
    hipLaunchKernelGGL(mesh_rootscan_kernel, dim3(1), dim3(kMeshThreads), 0, st, s.nblk, s.blk, (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("mesh_rootscan_kernel");
    hipLaunchKernelGGL(mesh_rank_kernel, dim3(s.nblk), dim3(kMeshThreads), 0, st, (uint32_t)T, (const uint32_t *)s.root,
                       (const uint32_t *)s.blk, s.dense, out_counts);
    SLS_LAUNCH_CHECK("mesh_rank_kernel");
    hipLaunchKernelGGL(mesh_label_kernel, grid_for((size_t)T, kMeshThreads), dim3(kMeshThreads), 0, st, (uint32_t)T, (const uint32_t *)s.root,
                       (const uint32_t *)s.dense, out_labels, out_counts);
    SLS_LAUNCH_CHECK("mesh_label_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// selection and compaction
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup: n_min from the k-th largest of the C counts (uf_kth_largest)
__global__ __launch_bounds__(kMeshThreads) void mesh_nmin_kernel(uint32_t T, const uint32_t *__restrict__ cluster_status,
                                                                 const int32_t *__restrict__ counts, int keep_clusters, int min_triangles,
                                                                 uint32_t *__restrict__ hdr)
{
    const uint32_t C = min(cluster_status[0], T);
    const uint32_t lo = uf_kth_largest<MeshChunks>(T, C, sls_mesh_keep_rank(keep_clusters, C), counts);
    if (threadIdx.x == 0) hdr[MH_NMIN] = sls_mesh_n_min(min_triangles, lo);
}

// the kept flags of this thread's four consecutive triangles, as a bit mask
__device__ __forceinline__ uint32_t mesh_kept_mask(uint32_t T, int V, uint32_t C, uint32_t n_min, const int32_t *__restrict__ faces,
                                                   const int32_t *__restrict__ labels, const int32_t *__restrict__ counts, uint32_t t0)
{
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j) {
        const uint32_t t = t0 + (uint32_t)j;
        if (t < T) {
            const int32_t l = labels[t];
            const int32_t f[3] = { faces[3 * (size_t)t], faces[3 * (size_t)t + 1], faces[3 * (size_t)t + 2] };
            if (l >= 0 && (uint32_t)l < C && sls_mesh_degenerate(f, V) == 0 && (uint32_t)counts[l] >= n_min) mask |= 1u << j;
        }
    }
    return mask;
}

__global__ __launch_bounds__(kMeshThreads) void mesh_mark_kernel(uint32_t T, int V, const int32_t *__restrict__ faces,
                                                                 const int32_t *__restrict__ labels, const int32_t *__restrict__ counts,
                                                                 const uint32_t *__restrict__ cluster_status, const uint32_t *__restrict__ hdr,
                                                                 uint32_t *vflag, uint32_t *__restrict__ blk)
{
    const uint32_t t0 = MeshChunks::first();
    const uint32_t mask = mesh_kept_mask(T, V, min(cluster_status[0], T), hdr[MH_NMIN], faces, labels, counts, t0);
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j)
        if ((mask >> j) & 1u) {
            const size_t t = t0 + (uint32_t)j;
            vflag[faces[3 * t]] = 1u; vflag[faces[3 * t + 1]] = 1u; vflag[faces[3 * t + 2]] = 1u;     // (every writer stores 1)
        }
    MeshChunks::total((uint32_t)__popc(mask), blk);
}

__global__ __launch_bounds__(kMeshThreads) void mesh_vcount_kernel(uint32_t V, const uint32_t *__restrict__ vflag, uint32_t *__restrict__ blk)
{
    MeshChunks::total((uint32_t)__popc(MeshChunks::flag_mask(V, vflag, MeshChunks::first())), blk);
}

__global__ __launch_bounds__(kMeshThreads) void mesh_filter_scan_kernel(int nblk_t, uint32_t *blk_t, int nblk_v, uint32_t *blk_v,
                                                                        const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    __shared__ uint32_t s_wave_t[kMeshThreads / 64], s_wave_v[kMeshThreads / 64];
    const uint32_t nt = scan_in_place<uint32_t, kMeshThreads>(blk_t, blk_t, nblk_t, s_wave_t);
    const uint32_t nv = scan_in_place<uint32_t, kMeshThreads>(blk_v, blk_v, nblk_v, s_wave_v);
    if (threadIdx.x == 0) { status[0] = nv; status[1] = nt; status[2] = hdr[MH_NMIN]; status[3] = 1u; }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_vwrite_kernel(uint32_t V, const uint32_t *__restrict__ vflag,
                                                                   const uint32_t *__restrict__ blk, const uint32_t *__restrict__ vertices,
                                                                   uint32_t *__restrict__ out_vertices, int32_t *__restrict__ vmap)
{
    const uint32_t v0 = MeshChunks::first();
    const uint32_t mask = MeshChunks::flag_mask(V, vflag, v0);
    uint32_t id = MeshChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j) {
        const size_t v = v0 + (uint32_t)j;
        if (v < V) {
            if ((mask >> j) & 1u) {                 // (id < V: the output holds V rows)
                out_vertices[3 * (size_t)id] = vertices[3 * v]; out_vertices[3 * (size_t)id + 1] = vertices[3 * v + 1];
                out_vertices[3 * (size_t)id + 2] = vertices[3 * v + 2];
                vmap[v] = (int32_t)id;
                ++id;
            } else vmap[v] = -1;
        }
    }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_fwrite_kernel(uint32_t T, int V, const int32_t *__restrict__ faces,
                                                                   const int32_t *__restrict__ labels, const int32_t *__restrict__ counts,
                                                                   const uint32_t *__restrict__ cluster_status, const uint32_t *__restrict__ hdr,
                                                                   const uint32_t *__restrict__ blk, const int32_t *__restrict__ vmap,
                                                                   int32_t *__restrict__ out_faces)
{
    const uint32_t t0 = MeshChunks::first();
    const uint32_t mask = mesh_kept_mask(T, V, min(cluster_status[0], T), hdr[MH_NMIN], faces, labels, counts, t0);
    uint32_t id = MeshChunks::rank((uint32_t)__popc(mask), blk);
#pragma unroll
    for (int j = 0; j < MeshChunks::kPer; ++j)
        if ((mask >> j) & 1u) {                     // (id < T: the output holds T rows)
            const size_t t = t0 + (uint32_t)j;
            out_faces[3 * (size_t)id] = vmap[faces[3 * t]]; out_faces[3 * (size_t)id + 1] = vmap[faces[3 * t + 1]];
            out_faces[3 * (size_t)id + 2] = vmap[faces[3 * t + 2]];
            ++id;
        }
}

struct MeshFilterScratch {
    uint32_t *hdr, *vflag, *blk_t, *blk_v;
    int32_t *vmap;
    size_t total;
    int nblk_t, nblk_v;
};

static MeshFilterScratch mesh_filter_layout(size_t V, size_t T, void *base)
{
    MeshFilterScratch s;
    Arena a(base);
    s.nblk_t = MeshChunks::count(T); s.nblk_v = MeshChunks::count(V);
    s.hdr = a.take<uint32_t>(16);
    s.vflag = a.take<uint32_t>(V);
    s.vmap = a.take<int32_t>(V);
    s.blk_t = a.take<uint32_t>((size_t)s.nblk_t);
    s.blk_v = a.take<uint32_t>((size_t)s.nblk_v);
    s.total = a.off;
    return s;
}

size_t mesh_filter_scratch_bytes(int V, int T)
{
    return mesh_sizes_ok(V, T) ? mesh_filter_layout((size_t)V, (size_t)T, nullptr).total : 0;
}

int launch_mesh_filter(int V, const float *vertices, int T, const int32_t *faces, const int32_t *labels, const int32_t *counts,
                       const uint32_t *cluster_status, int keep_clusters, int min_triangles, float *out_vertices, int32_t *out_faces,
                       int32_t *out_vmap, uint32_t *out_status, void *scratch, hipStream_t st)
{
    const MeshFilterScratch s = mesh_filter_layout((size_t)V, (size_t)T, scratch);
    int32_t *vmap = out_vmap ? out_vmap : s.vmap;
    SLS_HIP_CHECK(hipMemsetAsync(s.vflag, 0, sizeof(uint32_t) * (size_t)V, st));
    hipLaunchKernelGGL(mesh_nmin_kernel, dim3(1), dim3(kMeshThreads), 0, st, (uint32_t)T, cluster_status, counts, keep_clusters,
                       min_triangles, s.hdr);
    SLS_LAUNCH_CHECK("mesh_nmin_kernel");
    hipLaunchKernelGGL(mesh_mark_kernel, dim3(s.nblk_t), dim3(kMeshThreads), 0, st, (uint32_t)T, V, faces, labels, counts, cluster_status,
                       (const uint32_t *)s.hdr, s.vflag, s.blk_t);
    SLS_LAUNCH_CHECK("mesh_mark_kernel");
    hipLaunchKernelGGL(mesh_vcount_kernel, dim3(s.nblk_v), dim3(kMeshThreads), 0, st, (uint32_t)V, (const uint32_t *)s.vflag, s.blk_v);
    SLS_LAUNCH_CHECK("mesh_vcount_kernel");
    hipLaunchKernelGGL(mesh_filter_scan_kernel, dim3(1), dim3(kMeshThreads), 0, st, s.nblk_t, s.blk_t, s.nblk_v, s.blk_v,
                       (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("mesh_filter_scan_kernel");
    hipLaunchKernelGGL(mesh_vwrite_kernel, dim3(s.nblk_v), dim3(kMeshThreads), 0, st, (uint32_t)V, (const uint32_t *)s.vflag,
                       (const uint32_t *)s.blk_v, (const uint32_t *)vertices, (uint32_t *)out_vertices, vmap);
    SLS_LAUNCH_CHECK("mesh_vwrite_kernel");
    hipLaunchKernelGGL(mesh_fwrite_kernel, dim3(s.nblk_t), dim3(kMeshThreads), 0, st, (uint32_t)T, V, faces, labels, counts, cluster_status,
                       (const uint32_t *)s.hdr, (const uint32_t *)s.blk_t, (const int32_t *)vmap, out_faces);
    SLS_LAUNCH_CHECK("mesh_fwrite_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// vertex normals
// ---------------------------------------------------------------------------------------------------------------------
// the key of corner 3 t + c: its vertex, or V for a corner of a degenerate triangle (sorted behind every vertex)
__global__ __launch_bounds__(kMeshThreads) void mesh_corner_keys_kernel(int T, const int32_t *__restrict__ faces, int V,
                                                                        uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const size_t t = (size_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= (size_t)T) return;
    const int32_t f[3] = { faces[3 * t], faces[3 * t + 1], faces[3 * t + 2] };
    const int d = sls_mesh_degenerate(f, V);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        keys[3 * t + c] = d ? (uint32_t)V : (uint32_t)f[c];
        vals[3 * t + c] = (uint32_t)(3 * t + c);
    }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_normals_kernel(uint32_t V, uint32_t n, const float *__restrict__ vertices,
                                                                    const int32_t *__restrict__ faces, const uint32_t *__restrict__ keys,
                                                                    const uint32_t *__restrict__ vals, float *__restrict__ normals)
{
    const size_t v = (size_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (v >= V) return;
    uint32_t lo = 0u, hi = n;                       // the first position with keys >= v lies in [lo, hi]
    while (lo < hi) {                               // (lower_bound_u32, sls_geom.hpp, is this walk; calling it here changes
        const uint32_t mid = lo + ((hi - lo) >> 1); // this kernel's instructions, so the kernel keeps its own text)
        if (keys[mid] < (uint32_t)v) lo = mid + 1u; else hi = mid;
    }
    float s[3] = { 0.0f, 0.0f, 0.0f }, nv[3];
    for (uint32_t j = lo; j < n && keys[j] == (uint32_t)v; ++j) {
        const size_t t = vals[j] / 3u;
        const size_t a = (size_t)faces[3 * t], b = (size_t)faces[3 * t + 1], c = (size_t)faces[3 * t + 2];
        const float p0[3] = { vertices[3 * a], vertices[3 * a + 1], vertices[3 * a + 2] };
        const float p1[3] = { vertices[3 * b], vertices[3 * b + 1], vertices[3 * b + 2] };
        const float p2[3] = { vertices[3 * c], vertices[3 * c + 1], vertices[3 * c + 2] };
        float fn[3];
        sls_mesh_face_normal(p0, p1, p2, fn);
        s[0] += fn[0]; s[1] += fn[1]; s[2] += fn[2];
    }
    sls_mesh_normalise(s, nv);
    normals[3 * v] = nv[0]; normals[3 * v + 1] = nv[1]; normals[3 * v + 2] = nv[2];
}

size_t mesh_normals_scratch_bytes(int V, int T)
{
    return mesh_sizes_ok(V, T) ? mesh_sort_layout(3 * (size_t)T, nullptr).total : 0;
}

// The 3 T corners sorted by vertex (T >= 1): *keys the vertex of every sorted position (V for a corner of a degenerate
// triangle, behind every vertex), *vals its corner id 3 t + c, ascending within a vertex.  Both point into the scratch
// (mesh_normals_scratch_bytes).  sls_signdist.hip sums its vertex pseudo-normals over the same runs.
int mesh_corner_sort(int V, int T, const int32_t *faces, void *scratch, const uint32_t **keys, const uint32_t **vals, hipStream_t st)
{
    const MeshSortScratch s = mesh_sort_layout(3 * (size_t)T, scratch);
    const uint32_t n = 3u * (uint32_t)T;
    hipLaunchKernelGGL(mesh_hdr_kernel, dim3(1), dim3(64), 0, st, s.hdr, n);
    SLS_LAUNCH_CHECK("mesh_hdr_kernel");
    hipLaunchKernelGGL(mesh_corner_keys_kernel, grid_for((size_t)T, kMeshThreads), dim3(kMeshThreads), 0, st, T, faces, V, s.keys, s.vals);
    SLS_LAUNCH_CHECK("mesh_corner_keys_kernel");
    int which = 0;
    const int rc = radix_sort_pairs_u32(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + MH_COUNT, n, sls_mesh_index_bits(V + 1), s.sort,
                                        s.sort_bytes, &which, st);
    if (rc) return rc;
    *keys = which ? s.keys_tmp : s.keys;
    *vals = which ? s.vals_tmp : s.vals;
    return SLS_OK;
}

int launch_mesh_vertex_normals(int V, const float *vertices, int T, const int32_t *faces, float *out_normals, void *scratch,
                               hipStream_t st)
{
    if (T == 0) {
        SLS_HIP_CHECK(hipMemsetAsync(out_normals, 0, 3 * sizeof(float) * (size_t)V, st));
        return SLS_OK;
    }
    const uint32_t *keys = nullptr, *vals = nullptr;
    const int rc = mesh_corner_sort(V, T, faces, scratch, &keys, &vals, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_normals_kernel, grid_for((size_t)V, kMeshThreads), dim3(kMeshThreads), 0, st, (uint32_t)V, 3u * (uint32_t)T,
                       vertices, faces, keys, vals, out_normals);
    SLS_LAUNCH_CHECK("mesh_normals_kernel");
    return SLS_OK;
}

}  // namespace sls
