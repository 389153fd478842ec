// sls_geom.hpp — the small pieces the device geometry ops share besides their scans (sls_scan.hpp): the finiteness test
// and the ordered-float mapping with the bounding-box minimum built on them (sls_cloud.hip, sls_simplify.hip, sls_tsdf.hip),
// the xor butterfly of the long-row sums, and for the mesh ops (sls_mesh.hip, sls_simplify.hip, sls_smooth.hip,
// sls_fill.hip) the size guard, the degenerate / out-of-range counters and the directed index pairs sorted by (a, b).
#pragma once
#include <float.h>

#include "sls_launch.hpp"
#include "../../include/sls_mesh_math.h"

namespace sls {

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= FLT_MAX; }
__device__ __forceinline__ bool finite_row(const float *__restrict__ xyz, size_t i)
{
    return finite_f32(xyz[3 * i]) && finite_f32(xyz[3 * i + 1]) && finite_f32(xyz[3 * i + 2]);
}

__device__ __forceinline__ uint32_t f2ord(float f)
{   // monotone float -> uint mapping
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__device__ __forceinline__ uint32_t spread10(uint32_t v)
{   // 10 bits -> every third bit
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The curve code of a point in the bounding cube of an indexed cloud (bbox: 3 minima, 3 maxima, ordered floats; a point
// outside is clamped to the border cells): what sls_knn.hip sorts its clouds by and sls_icp.hip its moved queries.
__device__ __forceinline__ uint32_t curve_code(float x, float y, float z, const uint32_t *__restrict__ bbox, int key_bits)
{
    const float mnx = ord2f(bbox[0]), mny = ord2f(bbox[1]), mnz = ord2f(bbox[2]);
    const float ext = fmaxf(fmaxf(ord2f(bbox[3]) - mnx, ord2f(bbox[4]) - mny), fmaxf(ord2f(bbox[5]) - mnz, 1e-30f));
    const float s = 1024.0f / ext;
    const uint32_t qx = (uint32_t)fminf(fmaxf((x - mnx) * s, 0.0f), 1023.0f);
    const uint32_t qy = (uint32_t)fminf(fmaxf((y - mny) * s, 0.0f), 1023.0f);
    const uint32_t qz = (uint32_t)fminf(fmaxf((z - mnz) * s, 0.0f), 1023.0f);
    // Hilbert index of the cell (Skilling's axes-to-transpose form, 10 bits per axis): unlike the Morton
    // order it has no jumps, so runs of consecutive points (the boxes of the search) stay compact in space.
    uint32_t X[3] = { qx, qy, qz };
#pragma unroll
    for (uint32_t Q = 512u; Q > 1u; Q >>= 1) {
        const uint32_t P = Q - 1u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (X[a] & Q) X[0] ^= P;
            else { const uint32_t t = (X[0] ^ X[a]) & P; X[0] ^= t; X[a] ^= t; }
        }
    }
    X[1] ^= X[0]; X[2] ^= X[1];
    uint32_t t = 0;
#pragma unroll
    for (uint32_t Q = 512u; Q > 1u; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1u;
    X[0] ^= t; X[1] ^= t; X[2] ^= t;
    // small clouds are sorted on the top 21 bits only (two 11-bit radix passes instead of three 10-bit ones;
    // points of one 2^-7 cell stay in input order): measured faster up to ~200 k points, slower beyond
    return ((spread10(X[0]) << 2) | (spread10(X[1]) << 1) | spread10(X[2])) >> (30 - key_bits);
}

// The body of a bounding-box-minimum kernel of THREADS threads (grid-stride over the n rows of xyz): mn[0 .. 2] <- the
// float32 minimum per axis over the finite rows (integer atomicMin in the ordered domain: order-free; the caller set the
// words to 0xFFFFFFFF), *nonfinite += the rows with a non-finite coordinate, which take no part in the minimum.  A row whose
// live flag is 0 takes part in neither (live null: all live).
template <int THREADS>
__device__ __forceinline__ void bbox_min(uint32_t n, const float *__restrict__ xyz, const uint32_t *__restrict__ live, uint32_t *mn_out,
                                         uint32_t *nonfinite)
{
    float mn[3] = { INFINITY, INFINITY, INFINITY };
    uint32_t bad = 0u;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * THREADS) {
        if (live && !live[i]) continue;
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (finite_f32(x) && finite_f32(y) && finite_f32(z)) {
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        } else {
            bad += 1u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
        bad += __shfl_xor(bad, off, 64);
    }
    __shared__ uint32_t s_box[4];
    if (threadIdx.x < 4) s_box[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicMin(&s_box[k], f2ord(mn[k]));
        atomicAdd(&s_box[3], bad);
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&mn_out[threadIdx.x], s_box[threadIdx.x]);
    else if (threadIdx.x == 3 && s_box[3]) atomicAdd(nonfinite, s_box[3]);
}

// the sum of the 64 lanes' part[k] in every lane, by a fixed xor butterfly (a + b == b + a: every lane ends with the same
// bits; the offsets 32, 16, ..., 1 are the contract of the long-row sums)
template <int N>
__device__ __forceinline__ void xor_butterfly(double part[N])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) part[k] += __shfl_xor(part[k], off, 64);
    }
}

// ---- the mesh ops ---------------------------------------------------------------------------------------------------
inline bool mesh_sizes_ok(int V, int T) { return V > 0 && T > 0 && T <= SLS_MESH_MAX_TRIANGLES && V <= SLS_MESH_MAX_VERTICES; }

// deg = sls_mesh_degenerate of this thread's triangle (0 for a thread without one): the wave's counts of degenerate and of
// out-of-range triangles by one integer atomic each (order-free).  Called by whole waves.
__device__ __forceinline__ void count_degenerate(int deg, uint32_t *degenerate, uint32_t *range)
{
    const uint64_t md = __ballot(deg != 0), mr = __ballot(deg == 2);
    if ((threadIdx.x & 63) == 0) {
        if (md) atomicAdd(degenerate, (uint32_t)__popcll(md));
        if (mr) atomicAdd(range, (uint32_t)__popcll(mr));
    }
}

// the first position of the n ascending keys that holds a key >= v (n where there is none): where vertex v's run of
// sorted corners starts (sls_mesh.hip: the vertex normals; sls_signdist.hip: the vertex pseudo-normals)
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *__restrict__ keys, uint32_t n, uint32_t v)
{
    uint32_t lo = 0u, hi = n;                       // the position lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the sorted directed pair (a, b) at position p as one word: a in the high half
__device__ __forceinline__ uint64_t pair_key(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb, uint32_t p)
{
    return ((uint64_t)sa[p] << 32) | (uint64_t)sb[p];
}

// Orders the n directed pairs (a2[0][i], b2[0][i]) by (a, b) with two stable sorts (sls_radix.hip) of `bits` key bits each — by b with a as
// the value, then by a with b as the value: the order of a << bits | b at 8 bytes per item and pass instead of 12.
// a2[1] / b2[1] are the ping-pong copies; a2[*cur] / b2[*cur] hold the result.
inline int sort_pairs_ab(uint32_t *const a2[2], uint32_t *const b2[2], const uint32_t *count_ptr, uint32_t n, int bits, void *sort,
                         size_t sort_bytes, int *cur, hipStream_t st)
{
    int which = 0;
    int rc = radix_sort_pairs_u32(b2[0], a2[0], b2[1], a2[1], count_ptr, n, bits, sort, sort_bytes, &which, st);
    if (rc) return rc;
    *cur = which;
    rc = radix_sort_pairs_u32(a2[*cur], b2[*cur], a2[*cur ^ 1], b2[*cur ^ 1], count_ptr, n, bits, sort, sort_bytes, &which, st);
    *cur ^= which;
    return rc;
}

}  // namespace sls
