// sls_meshdist.hip — sls_mesh_distance: for every query point the nearest TRIANGLE of a mesh — the squared distance of
// include/sls_meshdist_math.h and the lowest face index attaining it.  A user of the sweep (sls_sweep.hpp): an index whose
// items are triangles (three float4: the vertices, the face index in a.w) in the curve order of their CENTROIDS, and whose
// boxes and sub-boxes bound ALL THREE vertices of their 256 / 32 triangles — the sweep prunes by "a gap never exceeds the
// distance to anything in the box", which a box over centroids would break.  A few huge triangles among many small ones
// make their runs' boxes loose: more runs are scanned, nothing is missed.  The codes live in the cube of the valid faces'
// vertices, so the queries' codes (nn_query_codes, nn_front_sorted_queries of sls_knn.hip: unchanged) live there too.
// A face with a vertex index outside [0, V) or a non-finite vertex is counted in the status words and indexed as three
// points at the origin: nothing is read out of range, and the caller discards the outputs.
// Built with the flags of sls_knn.hip (contraction allowed): tri_code_kernel's centroid arithmetic, and with it the
// faces' curve order, depends on them.  The results do not — any order gives the exact nearest face.
#include <float.h>

#include "sls_sweep.hpp"
#include "../../include/sls_nn_math.h"
#include "../../include/sls_meshdist_math.h"

namespace sls {

__global__ void tri_init_kernel(uint32_t *bbox, uint32_t *status, uint32_t F, uint32_t Mq, uint32_t word3)
{
    if (threadIdx.x < 3) bbox[threadIdx.x] = 0xFFFFFFFFu;
    else if (threadIdx.x < 6) bbox[threadIdx.x] = 0u;
    else if (threadIdx.x == 6) bbox[6] = F;
    else if (threadIdx.x == 7) bbox[7] = Mq;
    else if (threadIdx.x < 12) status[threadIdx.x - 8] = threadIdx.x == 8 ? F : (threadIdx.x == 11 ? word3 : 0u);
}

// the cube of the valid faces' vertices and the counts of the others (integer atomics: any order gives the same words)
__global__ __launch_bounds__(256) void tri_bbox_kernel(int V, const float *__restrict__ vertices, int F,
                                                       const int32_t *__restrict__ faces, uint32_t *bbox, uint32_t *status)
{
    float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    uint32_t n_index = 0, n_nonfinite = 0;
    for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) {
        float4 a, b, c;
        bool bad_index;
        if (!tri_load(V, vertices, faces, (size_t)f, a, b, c, &bad_index)) {
            if (bad_index) ++n_index; else ++n_nonfinite;
            continue;
        }
        mn[0] = fminf(mn[0], fminf(a.x, fminf(b.x, c.x))); mx[0] = fmaxf(mx[0], fmaxf(a.x, fmaxf(b.x, c.x)));
        mn[1] = fminf(mn[1], fminf(a.y, fminf(b.y, c.y))); mx[1] = fmaxf(mx[1], fmaxf(a.y, fmaxf(b.y, c.y)));
        mn[2] = fminf(mn[2], fminf(a.z, fminf(b.z, c.z))); mx[2] = fmaxf(mx[2], fmaxf(a.z, fmaxf(b.z, c.z)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
        }
        n_index += __shfl_xor(n_index, off, 64);
        n_nonfinite += __shfl_xor(n_nonfinite, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (mn[k] <= mx[k]) { atomicMin(&bbox[k], f2ord(mn[k])); atomicMax(&bbox[3 + k], f2ord(mx[k])); }
        }
        if (n_index) atomicAdd(&status[1], n_index);
        if (n_nonfinite) atomicAdd(&status[2], n_nonfinite);
    }
}

__global__ __launch_bounds__(256) void tri_code_kernel(int V, const float *__restrict__ vertices, int F,
                                                       const int32_t *__restrict__ faces, const uint32_t *__restrict__ bbox,
                                                       uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, int key_bits)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float4 a, b, c;
    bool bad_index;
    tri_load(V, vertices, faces, (size_t)f, a, b, c, &bad_index);
    const float third = 1.0f / 3.0f;
    keys[f] = curve_code(((a.x + b.x) + c.x) * third, ((a.y + b.y) + c.y) * third, ((a.z + b.z) + c.z) * third, bbox, key_bits);
    vals[f] = (uint32_t)f;
}

__global__ __launch_bounds__(256) void tri_gather_boxes_kernel(int V, const float *__restrict__ vertices, int F,
                                                               const int32_t *__restrict__ faces,
                                                               const uint32_t *__restrict__ sorted_idx,
                                                               TriItem *__restrict__ items, float4 *__restrict__ boxes,
                                                               float4 *__restrict__ subboxes)
{
    const int j = blockIdx.x * kSweepBox + threadIdx.x;
    float4 mn = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.0f), mx = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f);
    if (j < F) {
        const uint32_t f = sorted_idx[j];
        TriItem t;
        bool bad_index;
        tri_load(V, vertices, faces, (size_t)f, t.a, t.b, t.c, &bad_index);
        mn = make_float4(fminf(t.a.x, fminf(t.b.x, t.c.x)), fminf(t.a.y, fminf(t.b.y, t.c.y)), fminf(t.a.z, fminf(t.b.z, t.c.z)), 0.0f);
        mx = make_float4(fmaxf(t.a.x, fmaxf(t.b.x, t.c.x)), fmaxf(t.a.y, fmaxf(t.b.y, t.c.y)), fmaxf(t.a.z, fmaxf(t.b.z, t.c.z)), 0.0f);
        t.a.w = __uint_as_float(f);
        items[j] = t;
    }
    store_boxes(mn, mx, boxes, subboxes);
}

struct TriBestSearch {
    const float4 me;
    uint64_t best;
    __device__ __forceinline__ float bound() const { return sls_nn_key_dist2(best); }
    // a copy of the run's first triangle, as BestKeySearch pads: a sentinel at 1e30 would give inf - inf inside the arithmetic
    __device__ __forceinline__ TriItem pad(const TriItem *__restrict__ items, int r0) const { return items[r0]; }
    __device__ __forceinline__ void scan(const TriItem *s_run)
    {
#pragma unroll 2
        for (int k = 0; k < kSweepSub; ++k) {
            const float4 a = s_run[k].a, b = s_run[k].b, c = s_run[k].c;
            const float d2 = sls_meshdist_triangle(me.x, me.y, me.z, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, nullptr);
            const uint64_t key = sls_nn_key(d2, __float_as_uint(a.w));
            best = key < best ? key : best;
        }
    }
};

__global__ __launch_bounds__(64) void tri_query_kernel(int F, int nboxes, const TriItem *__restrict__ items,
                                                       const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes,
                                                       const uint32_t *__restrict__ tkeys, int Mq,
                                                       const float4 *__restrict__ qpts, const uint32_t *__restrict__ qkeys, int V,
                                                       const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                       float *__restrict__ out_dist2, int32_t *__restrict__ out_face,
                                                       float *__restrict__ out_closest)
{
    __shared__ SweepLdsOf<TriItem> lds;
    const TriIndex ix = { F, nboxes, items, boxes, subboxes };
    const int q0 = blockIdx.x * 64, q = q0 + threadIdx.x;   // (the grid has ceil(Mq / 64) waves: q0 < Mq)
    const bool live = q < Mq;
    const float4 me = qpts[live ? q : Mq - 1];
    TriBestSearch s = { me, SLS_NN_KEY_NONE };
    nn_search(ix, tkeys, qkeys[q0], live, me, s, lds);
    if (live) {
        const size_t i = __float_as_uint(me.w);
        const uint32_t face = sls_nn_key_index(s.best);
        out_dist2[i] = sls_nn_key_dist2(s.best);
        if (out_face) out_face[i] = (int32_t)face;
        if (out_closest) {
            // the winner's closest point, recomputed once from (q, face); a query that met only NaN holds no face
            float cp[3] = { me.x, me.y, me.z };
            float4 a, b, c;
            bool bad_index;
            if (face < (uint32_t)F && tri_load(V, vertices, faces, (size_t)face, a, b, c, &bad_index))
                sls_meshdist_triangle(me.x, me.y, me.z, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, cp);
            out_closest[3 * i] = cp[0];
            out_closest[3 * i + 1] = cp[1];
            out_closest[3 * i + 2] = cp[2];
        }
    }
}

// scratch: sls_nn_query's for (F, Mq) — codes, sorter, boxes, the queries' buffers; its float4 per target stays unused —
// then the triangles
static NnScratch mesh_distance_layout(int F, int Mq, void *base, TriItem **items)
{
    NnScratch s = nn_layout(F, Mq, base);
    Arena a(base);
    a.off = (s.total + 255) & ~(size_t)255;
    *items = a.take<TriItem>((size_t)F);
    s.total = a.off;
    return s;
}

size_t mesh_distance_scratch_bytes(int V, int F, int Mq)
{
    TriItem *items;
    return (V >= 1 && F >= 1 && Mq >= 0) ? mesh_distance_layout(F, Mq, nullptr, &items).total : 0;
}

// The index of a mesh's triangles, for launch_mesh_distance and for launch_mesh_rayindex_build (sls_raycast.hip) alike: the
// status words [F, faces with a bad index, faces with a non-finite vertex, word3] and the cube of the valid faces; then,
// unless counts_only, the centroids' codes, the sort, the triangles in curve order and their boxes and sub-boxes.
// count2: the item count of a second sort that follows (bbox[7]).  *which: where the sorted (code, index) pairs ended up.
int tri_index_build(int V, const float *vertices, int F, const int32_t *faces, const TriIndexBuild &b, uint32_t count2,
                    uint32_t *out_status, uint32_t word3, bool counts_only, hipStream_t st, int *which)
{
    const int nb = (F + 255) / 256, key_bits = knn_key_bits(F), nboxes = (F + kSweepBox - 1) / kSweepBox;
    hipLaunchKernelGGL(tri_init_kernel, dim3(1), dim3(64), 0, st, b.bbox, out_status, (uint32_t)F, count2, word3);
    SLS_LAUNCH_CHECK("tri_init_kernel");
    hipLaunchKernelGGL(tri_bbox_kernel, dim3(nb < 256 ? nb : 256), dim3(256), 0, st, V, vertices, F, faces, b.bbox, out_status);
    SLS_LAUNCH_CHECK("tri_bbox_kernel");
    if (counts_only) return SLS_OK;
    hipLaunchKernelGGL(tri_code_kernel, dim3(nb), dim3(256), 0, st, V, vertices, F, faces, b.bbox, b.keys, b.vals, key_bits);
    SLS_LAUNCH_CHECK("tri_code_kernel");
    const int rc = radix_sort_pairs_u32(b.keys, b.vals, b.keys_tmp, b.vals_tmp, b.bbox + 6, (uint32_t)F, key_bits, b.sort, b.sort_bytes,
                                        which, st);
    if (rc) return rc;
    hipLaunchKernelGGL(tri_gather_boxes_kernel, dim3(nboxes), dim3(kSweepBox), 0, st, V, vertices, F, faces,
                       *which ? b.vals_tmp : b.vals, b.items, b.boxes, b.subboxes);
    SLS_LAUNCH_CHECK("tri_gather_boxes_kernel");
    return SLS_OK;
}

int launch_mesh_distance(int V, const float *vertices, int F, const int32_t *faces, int Mq, const float *query_xyz,
                         float *out_dist2, int32_t *out_face, float *out_closest, uint32_t *out_status, void *scratch,
                         hipStream_t st)
{
    ScopedTimer tm(T_KNN, st);
    NnFront f;
    TriItem *items;
    const NnScratch &s = f.s = mesh_distance_layout(F, Mq, scratch, &items);
    const int key_bits = knn_key_bits(F), nboxes = (F + kSweepBox - 1) / kSweepBox;
    TriIndexBuild b{};
    b.bbox = s.t.bbox; b.keys = s.t.keys; b.keys_tmp = s.t.keys_tmp; b.vals = s.t.vals; b.vals_tmp = s.t.vals_tmp;
    b.items = items; b.boxes = s.t.boxes; b.subboxes = s.t.subboxes; b.sort = s.t.sort; b.sort_bytes = s.t.sort_bytes;
    int which = 0;
    int rc = tri_index_build(V, vertices, F, faces, b, (uint32_t)Mq, out_status, 1u, Mq == 0, st, &which);
    if (rc || Mq == 0) return rc;                       // (Mq == 0: the status alone)
    f.tkeys = which ? s.t.keys_tmp : s.t.keys;
    rc = nn_query_codes(Mq, query_xyz, s.t.bbox, s.qkeys, s.qvals, key_bits, st);
    if (rc) return rc;
    rc = nn_front_sorted_queries(F, Mq, query_xyz, st, &f);
    if (rc) return rc;
    hipLaunchKernelGGL(tri_query_kernel, dim3((Mq + 63) / 64), dim3(64), 0, st, F, nboxes, items, s.t.boxes, s.t.subboxes, f.tkeys,
                       Mq, f.qpts, f.qkeys, V, vertices, faces, out_dist2, out_face, out_closest);
    SLS_LAUNCH_CHECK("tri_query_kernel");
    return SLS_OK;
}

}  // namespace sls
