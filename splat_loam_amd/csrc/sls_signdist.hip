// sls_signdist.hip — the SIGNED distance of points to a triangle mesh: the pseudo-normal tables of a mesh
// (sls_mesh_pseudonormals) and the sign of sls_mesh_distance's result from them (sls_mesh_signed_distance); the signed
// twins of sls_nn_stats and sls_error_colors live with them in sls_metrics.hip.  include/sls_signdist_math.h
// states every rule; tests/signdist_ref.py compiles it for the host.  Built EXACT (-ffp-contract=off): the bits of the
// tables are part of the contract.
//
// sls_mesh_pseudonormals, launches ordered by the stream alone, nothing read back:
//   sd_face          a thread per face: its class, its unit normal and its three corner angles in float64 (kept in the
//                    scratch for the two sums), the float32 face row, the three edge keys (0 for a degenerate face)
//   the stable sort  2 x bits(V) key bits over (u64 edge key, u32 corner id) pairs (radix_sort_pairs_u64): the corners of
//                    an edge next to each other, in ascending corner id
//   sd_edge          a thread per sorted position; the HEAD of a run of equal keys walks it twice: the sum of the unit
//                    normals in that order, then the same float32 row to every corner of the run.  Edge statistics from
//                    the run's length (integer atomics: order-free)
//   the corner sort  corners by vertex, as sls_mesh_vertex_normals sorts them (mesh_corner_sort, sls_mesh.hip)
//   sd_vertex        a thread per vertex: its run by bisection (lower_bound_u32), the sum of angle x normal in that order
// No float atomics, no hash table: every sum runs in ascending corner id, so every run gives the same bytes.
//
// sls_mesh_signed_distance: launch_mesh_distance as it is (d2, face, closest), then sd_sign, a thread per query: the named
// face's vertices again, sls_sd_triangle for the feature, the feature's row, the sign.  52 bytes gathered per query.
#include "sls_geom.hpp"
#include "../../include/sls_signdist_math.h"

namespace sls {

constexpr int kSdThreads = 256;
enum { SH_COUNT = 8 };          // hdr[0 .. 6]: the status words; hdr[SH_COUNT]: 3 F, the sorter's device-side count

__global__ void sd_init_kernel(uint32_t *hdr, uint32_t n)
{
    if (threadIdx.x < 16) hdr[threadIdx.x] = threadIdx.x == SH_COUNT ? n : 0u;
}

__global__ __launch_bounds__(kSdThreads) void sd_face_kernel(int F, int V, int bits, const float *__restrict__ vertices,
                                                             const int32_t *__restrict__ faces, float *__restrict__ out_face_n,
                                                             double *__restrict__ fn64, double *__restrict__ ang,
                                                             uint64_t *__restrict__ ekeys, uint32_t *__restrict__ evals, uint32_t *hdr)
{
    const size_t f = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
    int cls = 0;
    if (f < (size_t)F) {
        const int32_t idx[3] = { faces[3 * f], faces[3 * f + 1], faces[3 * f + 2] };
        double n[3], theta[3];
        cls = sls_sd_face(vertices, idx, V, n, theta);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_face_n[3 * f + k] = (float)n[k];
            fn64[3 * f + k] = n[k];
            ang[3 * f + k] = theta[k];
            ekeys[3 * f + k] = (cls == 1 || cls == 2) ? (uint64_t)0 : sls_mesh_edge_key(idx, k, bits);
            evals[3 * f + k] = (uint32_t)(3 * f + k);
        }
    }
    const uint64_t m0 = __ballot(cls == 1 || cls == 2), m1 = __ballot(cls == 2), m2 = __ballot(cls == 3), m3 = __ballot(cls == 4);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(&hdr[0], (uint32_t)__popcll(m0));
        if (m1) atomicAdd(&hdr[1], (uint32_t)__popcll(m1));
        if (m2) atomicAdd(&hdr[2], (uint32_t)__popcll(m2));
        if (m3) atomicAdd(&hdr[3], (uint32_t)__popcll(m3));
    }
}

__global__ __launch_bounds__(kSdThreads) void sd_edge_kernel(uint32_t n, const uint64_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ vals, const int32_t *__restrict__ faces,
                                                             const double *__restrict__ fn64, float *__restrict__ out_edge_n,
                                                             uint32_t *hdr)
{
    const size_t j = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
    bool boundary = false, nonmanifold = false, same_way = false;
    if (j < n) {
        const uint64_t k = keys[j];
        if (k == 0u) {                              // a corner of a degenerate face: zeros
            const size_t c = vals[j];
            out_edge_n[3 * c] = 0.0f; out_edge_n[3 * c + 1] = 0.0f; out_edge_n[3 * c + 2] = 0.0f;
        } else if (j == 0 || keys[j - 1] != k) {    // the head of a run of equal keys
            double s[3] = { 0.0, 0.0, 0.0 };
            size_t e = j;
            for (; e < n && keys[e] == k; ++e) {
                const size_t t = vals[e] / 3u;
                const double fn[3] = { fn64[3 * t], fn64[3 * t + 1], fn64[3 * t + 2] };
                sls_sd_accumulate(s, 1.0, fn);
            }
            const float r[3] = { (float)s[0], (float)s[1], (float)s[2] };
            for (size_t i = j; i < e; ++i) {
                const size_t c = vals[i];
                out_edge_n[3 * c] = r[0]; out_edge_n[3 * c + 1] = r[1]; out_edge_n[3 * c + 2] = r[2];
            }
            const size_t g = e - j;
            boundary = g == 1;
            nonmanifold = g >= 3;
            // corner c runs from faces[c] to the face's next vertex: two owners that START at the same vertex disagree
            same_way = g == 2 && faces[vals[j]] == faces[vals[j + 1]];
        }
    }
    const uint64_t mb = __ballot(boundary), mn = __ballot(nonmanifold), ms = __ballot(same_way);
    if ((threadIdx.x & 63) == 0) {
        if (mb) atomicAdd(&hdr[4], (uint32_t)__popcll(mb));
        if (mn) atomicAdd(&hdr[5], (uint32_t)__popcll(mn));
        if (ms) atomicAdd(&hdr[6], (uint32_t)__popcll(ms));
    }
}

__global__ __launch_bounds__(kSdThreads) void sd_vertex_kernel(uint32_t V, uint32_t n, const uint32_t *__restrict__ keys,
                                                               const uint32_t *__restrict__ vals, const double *__restrict__ fn64,
                                                               const double *__restrict__ ang, float *__restrict__ out_vertex_n)
{
    const size_t v = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
    if (v >= V) return;
    double s[3] = { 0.0, 0.0, 0.0 };
    for (uint32_t j = lower_bound_u32(keys, n, (uint32_t)v); j < n && keys[j] == (uint32_t)v; ++j) {
        const size_t c = vals[j], t = c / 3u;
        const double fn[3] = { fn64[3 * t], fn64[3 * t + 1], fn64[3 * t + 2] };
        sls_sd_accumulate(s, ang[c], fn);
    }
    out_vertex_n[3 * v] = (float)s[0]; out_vertex_n[3 * v + 1] = (float)s[1]; out_vertex_n[3 * v + 2] = (float)s[2];
}

__global__ void sd_status_kernel(const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    if (threadIdx.x < 8) status[threadIdx.x] = threadIdx.x < 7 ? hdr[threadIdx.x] : 1u;
}

struct PseudoScratch {
    uint32_t *hdr;
    double *fn64, *ang;
    uint64_t *keys, *keys_tmp;
    uint32_t *vals, *vals_tmp;
    void *sort, *corner;        // the edge sort's scratch; the corner sort's (mesh_normals_scratch_bytes)
    size_t sort_bytes, total;
};

static PseudoScratch pseudo_layout(int V, int F, void *base)
{
    PseudoScratch s;
    Arena a(base);
    const size_t n = 3 * (size_t)F;
    s.hdr = a.take<uint32_t>(16);
    s.fn64 = a.take<double>(n);
    s.ang = a.take<double>(n);
    s.keys = a.take<uint64_t>(n);
    s.keys_tmp = a.take<uint64_t>(n);
    s.vals = a.take<uint32_t>(n);
    s.vals_tmp = a.take<uint32_t>(n);
    s.sort_bytes = sort_scratch_bytes((uint64_t)n);
    s.sort = a.take<char>(s.sort_bytes);
    s.corner = a.take<char>(mesh_normals_scratch_bytes(V, F));
    s.total = a.off;
    return s;
}

size_t mesh_pseudonormals_scratch_bytes(int V, int F) { return mesh_sizes_ok(V, F) ? pseudo_layout(V, F, nullptr).total : 0; }

int launch_mesh_pseudonormals(int V, const float *vertices, int F, const int32_t *faces, float *out_face_normals,
                              float *out_edge_normals, float *out_vertex_normals, uint32_t *out_status, void *scratch, hipStream_t st)
{
    const PseudoScratch s = pseudo_layout(V, F, scratch);
    const uint32_t n = 3u * (uint32_t)F;
    const int bits = sls_mesh_index_bits(V);
    hipLaunchKernelGGL(sd_init_kernel, dim3(1), dim3(64), 0, st, s.hdr, n);
    SLS_LAUNCH_CHECK("sd_init_kernel");
    hipLaunchKernelGGL(sd_face_kernel, grid_for((size_t)F, kSdThreads), dim3(kSdThreads), 0, st, F, V, bits, vertices, faces,
                       out_face_normals, s.fn64, s.ang, s.keys, s.vals, s.hdr);
    SLS_LAUNCH_CHECK("sd_face_kernel");
    int which = 0;
    int rc = radix_sort_pairs_u64(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + SH_COUNT, n, 2 * bits, s.sort, s.sort_bytes, &which, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sd_edge_kernel, grid_for((size_t)n, kSdThreads), dim3(kSdThreads), 0, st, n,
                       (const uint64_t *)(which ? s.keys_tmp : s.keys), (const uint32_t *)(which ? s.vals_tmp : s.vals), faces,
                       (const double *)s.fn64, out_edge_normals, s.hdr);
    SLS_LAUNCH_CHECK("sd_edge_kernel");
    const uint32_t *ckeys = nullptr, *cvals = nullptr;
    rc = mesh_corner_sort(V, F, faces, s.corner, &ckeys, &cvals, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sd_vertex_kernel, grid_for((size_t)V, kSdThreads), dim3(kSdThreads), 0, st, (uint32_t)V, n, ckeys, cvals,
                       (const double *)s.fn64, (const double *)s.ang, out_vertex_normals);
    SLS_LAUNCH_CHECK("sd_vertex_kernel");
    hipLaunchKernelGGL(sd_status_kernel, dim3(1), dim3(64), 0, st, (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("sd_status_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the sign
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSdThreads) void sd_sign_kernel(int V, const float *__restrict__ vertices, int F,
                                                             const int32_t *__restrict__ faces, const float *__restrict__ face_n,
                                                             const float *__restrict__ edge_n, const float *__restrict__ vertex_n,
                                                             int Mq, const float *__restrict__ query, const float *__restrict__ dist2,
                                                             const int32_t *__restrict__ face, float *__restrict__ out_sdist,
                                                             uint8_t *__restrict__ out_feature)
{
    const size_t i = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
    if (i >= (size_t)Mq) return;
    const float d2 = dist2[i];
    const int32_t f = face[i];
    float sd = sqrtf(d2);                           // a query that met no face (a NaN) keeps the non-negative value
    int feature = 0;
    if (f >= 0 && f < F) {
        const int32_t idx[3] = { faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2] };
        if (sls_mesh_degenerate(idx, V) != 2) {
            const float q[3] = { query[3 * i], query[3 * i + 1], query[3 * i + 2] };
            float p[3][3], rel[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[k][0] = vertices[3 * (size_t)idx[k]]; p[k][1] = vertices[3 * (size_t)idx[k] + 1]; p[k][2] = vertices[3 * (size_t)idx[k] + 2];
            }
            sls_sd_triangle(q, p[0], p[1], p[2], rel, &feature);
            // the feature's row: the face's, the corner's edge row, the vertex's
            const float *row = face_n + 3 * (size_t)f;
            if (feature >= 4) row = vertex_n + 3 * (size_t)(feature == 4 ? idx[0] : feature == 5 ? idx[1] : idx[2]);
            else if (feature >= 1) row = edge_n + 3 * (3 * (size_t)f + (size_t)(feature - 1));
            const float n[3] = { row[0], row[1], row[2] };
            sd = sls_sd_signed(d2, rel, n);
        }
    }
    out_sdist[i] = sd;
    if (out_feature) out_feature[i] = (uint8_t)feature;
}

struct SignedScratch {
    void *dist;                 // launch_mesh_distance's
    float *d2;
    int32_t *face;
    size_t total;
};

static SignedScratch signed_layout(int V, int F, int Mq, void *base)
{
    SignedScratch s;
    Arena a(base);
    s.dist = a.take<char>(mesh_distance_scratch_bytes(V, F, Mq));
    s.d2 = a.take<float>((size_t)Mq);
    s.face = a.take<int32_t>((size_t)Mq);
    s.total = a.off;
    return s;
}

size_t mesh_signed_distance_scratch_bytes(int V, int F, int Mq)
{
    return (V >= 1 && F >= 1 && Mq >= 0) ? signed_layout(V, F, Mq, nullptr).total : 0;
}

int launch_mesh_signed_distance(const SignedDistanceLaunch &a, hipStream_t st)
{
    const SignedScratch s = signed_layout(a.V, a.F, a.Mq, a.scratch);
    int32_t *face = a.out_face ? a.out_face : s.face;
    const int rc = launch_mesh_distance(a.V, a.vertices, a.F, a.faces, a.Mq, a.query_xyz, s.d2, face, a.out_closest, a.out_status,
                                        s.dist, st);
    if (rc || a.Mq == 0) return rc;                 // (Mq == 0: the status alone)
    hipLaunchKernelGGL(sd_sign_kernel, grid_for((size_t)a.Mq, kSdThreads), dim3(kSdThreads), 0, st, a.V, a.vertices, a.F, a.faces,
                       a.face_n, a.edge_n, a.vertex_n, a.Mq, a.query_xyz, (const float *)s.d2, (const int32_t *)face, a.out_sdist,
                       a.out_feature);
    SLS_LAUNCH_CHECK("sd_sign_kernel");
    return SLS_OK;
}

}  // namespace sls
