// sls_raycast.hip — sls_mesh_rayindex_build / sls_mesh_raycast: for every ray the FIRST triangle of a mesh it hits — the
// parameter t, the face and its barycentric weights as include/sls_raycast_math.h defines them, the lowest face index
// among hits of equal t bits.  The index is the one sls_mesh_distance sweeps (tri_index_build, sls_meshdist.hip): triangles in
// the curve order of their centroids, boxes over runs of 256 and sub-boxes over runs of 32 that bound all three
// vertices.  It is built once and cast against many times (one range image per keyframe).
//
// The traversal is a second walk over that index, ray against box instead of point against box.  One WAVE per 64
// consecutive rays in the CALLER's order (lane = ray), the workgroup IS the wave, every loop bounded by the box count:
//   1. chunks of 64 boxes in index order, lane = box: a box is listed if ANY of the wave's 64 rays passes sls_ray_box
//      against its own current bound — its best t so far, t_max until it has a hit; the rays are broadcast with v_readlane;
//   2. the listed boxes' sub-boxes the same way, 8 boxes per step, lane = (box slot, sub-box), compacted into LDS;
//   3. 64 listed sub-boxes at a time, lane = candidate: one bit per ray that passes it; a run some ray passes goes through
//      LDS, and only the lanes whose bit is set run sls_ray_triangle_frame over its 32 faces;
//   4. at the end the winner's u, v are recomputed once from (ray, face), as sls_mesh_distance recomputes its closest point.
// Exact whatever the order of the boxes: a lane keeps the minimum of the keys (bits(t) << 32 | face) of the hits it is
// shown, a minimum does not care about order or repeats, and sls_ray_box never rejects a box holding a face that
// sls_ray_triangle would report at or below the bound it is given (the derivation stands next to it) — bounds only
// shrink, and equality passes, so the equally near face of lower index in another box is still shown.  A lane is shown
// more than it needs (a run is staged for the lanes that pass its sub-box at the bounds of step 3's start): harmless.
// The order decides how soon the bounds shrink, nothing else; only the index order has been built.
// No float atomics, no scratch memory; the one integer atomic counts the refused rays.
#include "sls_sweep.hpp"
#include "../../include/sls_raycast_math.h"

namespace sls {

// what the index keeps in front of its arrays: the status words of its build, [F, bad index, non-finite, 0]
constexpr int kRayIndexHeaderWords = 64;

struct RayIndexLayout {
    uint32_t *header;
    TriIndexBuild b;
    size_t total;
};

static RayIndexLayout rayindex_layout(int F, void *base)
{
    const size_t nboxes = (size_t)((F + kSweepBox - 1) / kSweepBox);
    Arena a(base);
    RayIndexLayout L{};
    L.header = a.take<uint32_t>(kRayIndexHeaderWords);
    L.b.items = a.take<TriItem>((size_t)F);
    L.b.boxes = a.take<float4>(2 * nboxes);
    L.b.subboxes = a.take<float4>(2 * nboxes * kSweepSubs);
    // the rest serves the build alone
    L.b.bbox = a.take<uint32_t>(8);
    L.b.keys = a.take<uint32_t>((size_t)F);
    L.b.keys_tmp = a.take<uint32_t>((size_t)F);
    L.b.vals = a.take<uint32_t>((size_t)F);
    L.b.vals_tmp = a.take<uint32_t>((size_t)F);
    L.b.sort_bytes = sort_scratch_bytes((uint64_t)F);
    L.b.sort = a.take<char>(L.b.sort_bytes);
    L.total = a.off;
    return L;
}

size_t mesh_rayindex_bytes(int V, int F) { return (V >= 1 && F >= 1) ? rayindex_layout(F, nullptr).total : 0; }

__global__ void ray_status_kernel(const uint32_t *__restrict__ from, uint32_t *__restrict__ to)
{
    if (threadIdx.x < 4) to[threadIdx.x] = threadIdx.x < 3 ? from[threadIdx.x] : 0u;
}

int launch_mesh_rayindex_build(int V, const float *vertices, int F, const int32_t *faces, void *index, uint32_t *out_status,
                               hipStream_t st)
{
    ScopedTimer tm(T_KNN, st);
    const RayIndexLayout L = rayindex_layout(F, index);
    int which = 0;
    const int rc = tri_index_build(V, vertices, F, faces, L.b, 0u, L.header, 0u, false, st, &which);
    if (rc) return rc;
    hipLaunchKernelGGL(ray_status_kernel, dim3(1), dim3(64), 0, st, L.header, out_status);
    SLS_LAUNCH_CHECK("ray_status_kernel");
    return SLS_OK;
}

// A lane's ray: what the box test and the triangle test read of it
struct RayLane {
    float o[3], inv[3];
    int kz;
    sls_ray_frame fr;
};

// does ray q of the wave (its fields broadcast from lane q) pass the box at the bound hi_q?
__device__ __forceinline__ bool ray_q_passes(const RayLane &me, float t_min, float bound, int q, const float4 mn, const float4 mx)
{
    const float o[3] = { rl(me.o[0], q), rl(me.o[1], q), rl(me.o[2], q) };
    const float inv[3] = { rl(me.inv[0], q), rl(me.inv[1], q), rl(me.inv[2], q) };
    const float bmn[3] = { mn.x, mn.y, mn.z }, bmx[3] = { mx.x, mx.y, mx.z };
    return sls_ray_box(o, inv, __builtin_amdgcn_readlane(me.kz, q), bmn, bmx, t_min, rl(bound, q)) != 0;
}

__global__ __launch_bounds__(64) void raycast_kernel(int F, int nboxes, const TriItem *__restrict__ items,
                                                     const float4 *__restrict__ boxes, const float4 *__restrict__ subboxes, int Mr,
                                                     const float *__restrict__ origins, const float *__restrict__ directions,
                                                     float t_min, float t_max, int V, const float *__restrict__ vertices,
                                                     const int32_t *__restrict__ faces, float *__restrict__ out_t,
                                                     int32_t *__restrict__ out_face, float *__restrict__ out_uv,
                                                     uint32_t *__restrict__ status)
{
    __shared__ SweepLdsOf<TriItem> lds;
    const TriIndex ix = { F, nboxes, items, boxes, subboxes };
    const int lane = threadIdx.x, nsub = ix.nsub();
    const size_t r = (size_t)blockIdx.x * 64 + lane;      // (the grid has ceil(Mr / 64) waves)
    const bool live = r < (size_t)Mr;
    const size_t rr = live ? r : (size_t)Mr - 1;
    const float o_in[3] = { origins[3 * rr], origins[3 * rr + 1], origins[3 * rr + 2] };
    const float d_in[3] = { directions[3 * rr], directions[3 * rr + 1], directions[3 * rr + 2] };
    const bool valid = sls_ray_valid(o_in, d_in) != 0;
    const uint64_t refused = __ballot(live && !valid);
    if (lane == 0 && refused) atomicAdd(&status[3], (uint32_t)__builtin_popcountll(refused));
    const bool ok = live && valid;
    if (!__ballot(ok)) {
        if (live) {
            out_t[r] = INFINITY;
            if (out_face) out_face[r] = -1;
            if (out_uv) { out_uv[2 * r] = 0.0f; out_uv[2 * r + 1] = 0.0f; }
        }
        return;
    }
    // a lane without a ray of its own carries a harmless one and a bound nothing passes
    RayLane me;
    me.o[0] = ok ? o_in[0] : 0.0f; me.o[1] = ok ? o_in[1] : 0.0f; me.o[2] = ok ? o_in[2] : 0.0f;
    const float d[3] = { ok ? d_in[0] : 0.0f, ok ? d_in[1] : 0.0f, ok ? d_in[2] : 1.0f };
    sls_ray_inverse(d, me.inv);
    me.kz = sls_ray_axis(d);
    sls_ray_setup(me.o, d, &me.fr);
    uint64_t best = SLS_NN_KEY_NONE;
    // a hit at or below both t_max and the best t so far can still matter (an equal t of a lower face index does)
    auto bound = [&]() -> float { return ok ? fminf(sls_nn_key_dist2(best), t_max) : -INFINITY; };
    auto any_ray_passes = [&](const float4 mn, const float4 mx, float b) -> bool {
        bool pass = false;
        for (int q = 0; q < 64; ++q) pass = pass | ray_q_passes(me, t_min, b, q, mn, mx);
        return pass;
    };

    const int nchunks = (nboxes + 63) / 64;
    for (int it = 0; it < nchunks; ++it) {
        const float b0 = bound();
        // 1. the chunk's boxes, lane = box
        const int b = it * 64 + lane;
        bool c = false;
        if (b < nboxes) c = any_ray_passes(boxes[2 * b], boxes[2 * b + 1], b0);
        __builtin_amdgcn_wave_barrier();
        const int nb = wave_compact(c, (uint32_t)b, lds.box);
        if (nb == 0) continue;
        __syncthreads();
        // 2. their sub-boxes, 8 boxes per step
        int ns = 0;                                     // <= 8 * nb <= 512 = the size of lds.sub
        for (int g = 0; g < nb; g += 8) {
            const int slot = g + (lane >> 3);
            bool cs = false;
            uint32_t sb = 0;
            if (slot < nb) {
                sb = lds.box[slot] * kSweepSubs + (uint32_t)(lane & 7);
                if ((int)sb < nsub) cs = any_ray_passes(subboxes[2 * (size_t)sb], subboxes[2 * (size_t)sb + 1], b0);
            }
            ns += wave_compact(cs, sb, lds.sub + ns);
        }
        __syncthreads();
        // 3. the listed runs, 64 at a time: bit q of `shown` = ray q passes my candidate at its bound of now
        for (int base = 0; base < ns; base += 64) {
            const int nk = min(64, ns - base);
            const uint32_t sbl = lds.sub[base + min(lane, nk - 1)];
            const float4 mnl = subboxes[2 * (size_t)sbl], mxl = subboxes[2 * (size_t)sbl + 1];
            const float b1 = bound();
            uint64_t shown = 0ull;
            for (int q = 0; q < 64; ++q)
                if (ray_q_passes(me, t_min, b1, q, mnl, mxl)) shown |= 1ull << q;
            if (lane >= nk) shown = 0ull;
            uint64_t todo = __ballot(shown != 0ull);
            while (todo) {
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int sb = __builtin_amdgcn_readlane((int)sbl, j);
                const uint64_t mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(shown >> 32), j) << 32) |
                                      (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)shown, j);
                // a short last run is padded with copies of its first triangle: a minimum meets it again and does not change
                const int r0 = sb * kSweepSub, i = r0 + (lane & (kSweepSub - 1));
                __builtin_amdgcn_wave_barrier();
                if (lane < kSweepSub) lds.run[lane] = items[i < F ? i : r0];
                __syncthreads();
                if ((mask >> lane) & 1ull) {
#pragma unroll 2
                    for (int k = 0; k < kSweepSub; ++k) {
                        const float4 a = lds.run[k].a, bb = lds.run[k].b, cc = lds.run[k].c;
                        const float va[3] = { a.x, a.y, a.z }, vb[3] = { bb.x, bb.y, bb.z }, vc[3] = { cc.x, cc.y, cc.z };
                        float t, u, v;
                        if (sls_ray_triangle_frame(&me.fr, va, vb, vc, t_min, t_max, &t, &u, &v)) {
                            const uint64_t key = sls_nn_key(t, __float_as_uint(a.w));
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        }
    }

    if (live) {
        // 4. the winner's weights, recomputed once from (ray, face)
        const uint32_t face = sls_nn_key_index(best);
        float t = INFINITY, u = 0.0f, v = 0.0f;
        int32_t hit_face = -1;
        float4 a, b, c;
        bool bad_index;
        if (ok && face < (uint32_t)F && tri_load(V, vertices, faces, (size_t)face, a, b, c, &bad_index)) {
            const float va[3] = { a.x, a.y, a.z }, vb[3] = { b.x, b.y, b.z }, vc[3] = { c.x, c.y, c.z };
            float t2;
            if (sls_ray_triangle_frame(&me.fr, va, vb, vc, t_min, t_max, &t2, &u, &v)) { t = t2; hit_face = (int32_t)face; }
        }
        out_t[r] = t;
        if (out_face) out_face[r] = hit_face;
        if (out_uv) { out_uv[2 * r] = u; out_uv[2 * r + 1] = v; }
    }
}

int launch_mesh_raycast(const RaycastLaunch &a, hipStream_t st)
{
    ScopedTimer tm(T_KNN, st);
    const RayIndexLayout L = rayindex_layout(a.F, const_cast<void *>(a.index));
    hipLaunchKernelGGL(ray_status_kernel, dim3(1), dim3(64), 0, st, L.header, a.out_status);
    SLS_LAUNCH_CHECK("ray_status_kernel");
    if (a.Mr == 0) return SLS_OK;                       // the status alone
    static_assert(kSweepBox == 256 && kSweepSub == 32, "the kernel's lane mappings are written for 8 runs of 32");
    hipLaunchKernelGGL(raycast_kernel, dim3((a.Mr + 63) / 64), dim3(64), 0, st, a.F, (a.F + kSweepBox - 1) / kSweepBox, L.b.items,
                       L.b.boxes, L.b.subboxes, a.Mr, a.origins, a.directions, a.t_min, a.t_max, a.V, a.vertices, a.faces, a.out_t,
                       a.out_face, a.out_uv, a.out_status);
    SLS_LAUNCH_CHECK("raycast_kernel");
    return SLS_OK;
}

}  // namespace sls
