// sls_poisson.hip — screened Poisson surface reconstruction over the sparse 8x8x8-block volume of sls_tsdf.hip: the
// oriented samples splatted into a vector field and a density (sls_poisson_splat), the least-squares system over the edges
// of the band solved by Jacobi-preconditioned conjugate gradients (sls_poisson_solve) and the smoothed density the surface
// is trimmed by (sls_poisson_density).  include/sls_poisson_math.h states the arithmetic and every order of summation,
// tests/poisson_ref.py restates it in NumPy; DESIGN.md section 2, "Poisson volume", states the contract.  The zero surface
// leaves through sls_tsdf_extract_count / _emit unchanged.  Built EXACT (-ffp-contract=off); no float atomics anywhere.
//
// sls_poisson_splat, launches ordered by the stream alone:
//   poisson_keys      a thread per point: its cell's key (rank of the block << 9 | voxel; B << 9: none), its three
//                     fractions in float64, the identity permutation, the three counts (integer atomics: order-free)
//   the stable sort   radix_sort_pairs_u32 over the key's bits: inside a cell the points stay in input order
//   poisson_cells     the first and one-past-last sorted position of every cell that holds a point
//   poisson_gather    a workgroup per block, a thread per node: its eight cells c = 0 .. 7, the -x/-y/-z neighbour blocks
//                     from a table of eight bisections; a gather, not a scatter — that is what fixes the order
//
// sls_poisson_solve: poisson_neighbours (six bisections per block, once), poisson_system (b, diag, the start vectors and
// the block partials of <b,b> and <r,z>), then per pass four dependent launches — apply (p = z + beta p_old made on the
// way into the tile, own voxels and face halos alike, into the other half of a ping-pong pair; q = A p with p and its six
// face halos in LDS, the block partial of <p,q>), reduce (the step), update (x, r, z and the partials of <r,r>, <r,z>),
// reduce (the stopping test, beta) — and at the end the iso-level and chi.  The scalars live in a PoissonState in
// the scratch, written by the one-workgroup reduce launches and read by every later kernel; `done` is a uniform early
// exit, so the passes still enqueued after the end change nothing.  No host read, no synchronisation, no graph.
#include "sls_geom.hpp"
#include "../../include/sls_poisson_math.h"

namespace sls {

constexpr int kPoiThreads = SLS_TSDF_BLOCK_VOXELS;          // 512: a thread per voxel of a block
static_assert(kPoiThreads == SLS_POISSON_REDUCE && kPoiThreads == 512, "the sums' order is written for 8 waves of 64");
static_assert(SLS_TSDF_MAX_BLOCKS <= (1 << 19), "a cell key is rank << 9 | voxel in 32 bits");

struct PoissonGrid { double origin[3], h; };
enum { PH_COUNT = 0, PH_NONFINITE = 1, PH_RANGE = 2, PH_DROPPED = 3 };

// ---------------------------------------------------------------------------------------------------------------------
// splat
// ---------------------------------------------------------------------------------------------------------------------
__global__ void poisson_hdr_kernel(uint32_t *hdr, uint32_t M)
{
    if (threadIdx.x < 8) hdr[threadIdx.x] = threadIdx.x == PH_COUNT ? M : 0u;
}

__global__ __launch_bounds__(256) void poisson_keys_kernel(int M, const float *__restrict__ xyz, const float *__restrict__ normals,
                                                           int B, const int32_t *__restrict__ blocks, PoissonGrid g,
                                                           uint32_t *hdr, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                           double *__restrict__ frac)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool nonfinite = false, range = false, dropped = false;
    if (i < (size_t)M) {
        uint32_t key = (uint32_t)B << 9;
        double f[3] = { 0.0, 0.0, 0.0 };
        if (finite_row(xyz, i) && finite_row(normals, i)) {
            const float p[3] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
            int32_t cell[3];
            if (sls_poisson_cell(p, g.origin, g.h, cell, f)) {
                int d;
                key = sls_poisson_cell_key(B, blocks, cell, &d);
                dropped = d != 0;
            } else {
                range = true;
            }
        } else {
            nonfinite = true;
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
        frac[3 * i] = f[0]; frac[3 * i + 1] = f[1]; frac[3 * i + 2] = f[2];
    }
    const uint64_t mn = __ballot(nonfinite), mr = __ballot(range), md = __ballot(dropped);
    if ((threadIdx.x & 63) == 0) {
        if (mn) atomicAdd(&hdr[PH_NONFINITE], (uint32_t)__popcll(mn));
        if (mr) atomicAdd(&hdr[PH_RANGE], (uint32_t)__popcll(mr));
        if (md) atomicAdd(&hdr[PH_DROPPED], (uint32_t)__popcll(md));
    }
}

// first[k] / end[k] of every cell key k < limit that occurs in the sorted keys (the caller zeroed both arrays)
__global__ __launch_bounds__(256) void poisson_cells_kernel(uint32_t M, const uint32_t *__restrict__ keys, uint32_t limit,
                                                            uint32_t *__restrict__ first, uint32_t *__restrict__ end)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)M) return;
    const uint32_t k = keys[p];
    if (k >= limit) return;
    if (p == 0 || keys[p - 1] != k) first[k] = (uint32_t)p;
    if (p + 1 == (size_t)M || keys[p + 1] != k) end[k] = (uint32_t)p + 1u;
}

__global__ __launch_bounds__(kPoiThreads) void poisson_gather_kernel(int B, const int32_t *__restrict__ blocks, uint32_t M,
                                                                     const float *__restrict__ normals, const double *__restrict__ frac,
                                                                     const uint32_t *__restrict__ vals, const uint32_t *__restrict__ first,
                                                                     const uint32_t *__restrict__ end, float4 *__restrict__ field)
{
    __shared__ int s_nb[8];
    const int k = blockIdx.x, l = threadIdx.x;              // (the grid is B workgroups)
    if (l < 8)
        s_nb[l] = l == 0 ? k : sls_poisson_find(B, blocks, blocks[3 * (size_t)k] - (l & 1), blocks[3 * (size_t)k + 1] - ((l >> 1) & 1),
                                                blocks[3 * (size_t)k + 2] - (l >> 2));
    __syncthreads();
    const int x = l & 7, y = (l >> 3) & 7, z = l >> 6;
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cx = x - (c & 1), cy = y - ((c >> 1) & 1), cz = z - (c >> 2);
        const int kb = s_nb[(cx < 0 ? 1 : 0) | (cy < 0 ? 2 : 0) | (cz < 0 ? 4 : 0)];
        if (kb < 0) continue;
        const size_t slot = (size_t)kb * SLS_TSDF_BLOCK_VOXELS + (size_t)((cx & 7) | (cy & 7) << 3 | (cz & 7) << 6);
        const uint32_t q0 = first[slot], q1 = min(end[slot], M);
        for (uint32_t q = q0; q < q1; ++q) {
            const size_t i = vals[q];
            if (i >= (size_t)M) continue;                   // (a permutation of 0 .. M - 1: a guard)
            const double f[3] = { frac[3 * i], frac[3 * i + 1], frac[3 * i + 2] };
            const float n[3] = { normals[3 * i], normals[3 * i + 1], normals[3 * i + 2] };
            sls_poisson_splat_addf(f, n, c, acc);
        }
    }
    field[(size_t)k * SLS_TSDF_BLOCK_VOXELS + l] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
}

__global__ void poisson_splat_status_kernel(const uint32_t *__restrict__ hdr, uint32_t *__restrict__ status)
{
    if (threadIdx.x == 0) { status[0] = hdr[PH_NONFINITE]; status[1] = hdr[PH_RANGE]; status[2] = hdr[PH_DROPPED]; status[3] = 1u; }
}

struct PoissonSplatScratch {
    uint32_t *hdr, *keys, *keys_tmp, *vals, *vals_tmp, *first, *end;
    double *frac;
    void *sort;
    size_t sort_bytes, total;
};

static PoissonSplatScratch poisson_splat_layout(int M, int B, void *base)
{
    PoissonSplatScratch s;
    Arena a(base);
    const size_t S = (size_t)B * SLS_TSDF_BLOCK_VOXELS;
    s.hdr = a.take<uint32_t>(16);
    s.keys = a.take<uint32_t>((size_t)M);
    s.keys_tmp = a.take<uint32_t>((size_t)M);
    s.vals = a.take<uint32_t>((size_t)M);
    s.vals_tmp = a.take<uint32_t>((size_t)M);
    s.frac = a.take<double>(3 * (size_t)M);
    s.first = a.take<uint32_t>(S);
    s.end = a.take<uint32_t>(S);
    s.sort_bytes = sort_scratch_bytes((uint64_t)M);
    s.sort = a.take<char>(s.sort_bytes);
    s.total = a.off;
    return s;
}

static bool poisson_sizes_ok(int M, int B) { return M >= 0 && M <= SLS_TSDF_MAX_POINTS && B >= 0 && B <= SLS_TSDF_MAX_BLOCKS; }

size_t poisson_splat_scratch_bytes(int M, int B) { return (poisson_sizes_ok(M, B) && M > 0) ? poisson_splat_layout(M, B, nullptr).total : 0; }

int launch_poisson_splat(int M, const float *xyz, const float *normals, int B, const int32_t *blocks, double voxel_size,
                         const double *origin, float *out_field, uint32_t *out_status, void *scratch, hipStream_t st)
{
    const PoissonSplatScratch s = poisson_splat_layout(M, B, scratch);
    const size_t S = (size_t)B * SLS_TSDF_BLOCK_VOXELS;
    PoissonGrid g;
    g.origin[0] = origin[0]; g.origin[1] = origin[1]; g.origin[2] = origin[2]; g.h = voxel_size;
    hipLaunchKernelGGL(poisson_hdr_kernel, dim3(1), dim3(64), 0, st, s.hdr, (uint32_t)M);
    SLS_LAUNCH_CHECK("poisson_hdr_kernel");
    hipLaunchKernelGGL(poisson_keys_kernel, grid_for((size_t)M, 256), dim3(256), 0, st, M, xyz, normals, B, blocks, g, s.hdr, s.keys,
                       s.vals, s.frac);
    SLS_LAUNCH_CHECK("poisson_keys_kernel");
    if (B > 0) {
        int nbits = 0;
        while (nbits < 32 && ((uint64_t)B << 9) >> nbits) ++nbits;     // the sentinel B << 9 is the largest key
        int which = 0;
        const int rc = radix_sort_pairs_u32(s.keys, s.vals, s.keys_tmp, s.vals_tmp, s.hdr + PH_COUNT, (uint32_t)M, nbits, s.sort,
                                            s.sort_bytes, &which, st);
        if (rc) return rc;
        const uint32_t *keys = which ? s.keys_tmp : s.keys, *vals = which ? s.vals_tmp : s.vals;
        SLS_HIP_CHECK(hipMemsetAsync(s.first, 0, S * sizeof(uint32_t), st));
        SLS_HIP_CHECK(hipMemsetAsync(s.end, 0, S * sizeof(uint32_t), st));
        hipLaunchKernelGGL(poisson_cells_kernel, grid_for((size_t)M, 256), dim3(256), 0, st, (uint32_t)M, keys, (uint32_t)S, s.first, s.end);
        SLS_LAUNCH_CHECK("poisson_cells_kernel");
        hipLaunchKernelGGL(poisson_gather_kernel, dim3(B), dim3(kPoiThreads), 0, st, B, blocks, (uint32_t)M, normals,
                           (const double *)s.frac, vals, (const uint32_t *)s.first, (const uint32_t *)s.end, (float4 *)out_field);
        SLS_LAUNCH_CHECK("poisson_gather_kernel");
    }
    hipLaunchKernelGGL(poisson_splat_status_kernel, dim3(1), dim3(64), 0, st, (const uint32_t *)s.hdr, out_status);
    SLS_LAUNCH_CHECK("poisson_splat_status_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the stencil tile: NC planes of the block's own 512 values and the six 64-voxel face halos of the neighbour blocks
// ---------------------------------------------------------------------------------------------------------------------
template <int NC>
struct PoissonTile {
    float c[NC][SLS_TSDF_BLOCK_VOXELS];
    float h[6][64];
    int nb[6];
};

// voxel j = u | v << 3 of the face the neighbour block in direction d turns to this block (u, v: the other two axes ascending)
__device__ __forceinline__ int poisson_face_voxel(int d, int j)
{
    const int a = d >> 1, c = (d & 1) ? 0 : 7, u = j & 7, v = j >> 3;
    return a == 0 ? (c | u << 3 | v << 6) : a == 1 ? (u | c << 3 | v << 6) : (u | v << 3 | c << 6);
}
__device__ __forceinline__ int poisson_face_index(int d, int l)
{
    const int a = d >> 1, x = l & 7, y = (l >> 3) & 7, z = l >> 6;
    return a == 0 ? (y | z << 3) : a == 1 ? (x | z << 3) : (x | y << 3);
}

// The caller has written t.c[..][threadIdx.x]; every thread of the workgroup must call this (it synchronises).
// load(block, voxel, component): the halo value; direction d takes component d >> 1 of three, or the only one.
template <int NC, typename Load>
__device__ __forceinline__ void poisson_stage_halo(PoissonTile<NC> &t, int k, const int32_t *__restrict__ nb6, Load load)
{
    const int l = threadIdx.x;
    if (l < 6) t.nb[l] = nb6[6 * (size_t)k + l];
    __syncthreads();
    if (l < 6 * 64) {
        const int d = l >> 6, j = l & 63, nbk = t.nb[d];
        t.h[d][j] = nbk >= 0 ? load(nbk, poisson_face_voxel(d, j), NC == 3 ? d >> 1 : 0) : 0.0f;
    }
    __syncthreads();
}

template <int NC>
__device__ __forceinline__ void poisson_fetch(const PoissonTile<NC> &t, int l, float vn[6], int has[6])
{
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        int outside;
        const int l2 = sls_poisson_step(l, d, &outside);
        if (outside) { has[d] = t.nb[d] >= 0; vn[d] = t.h[d][poisson_face_index(d, l)]; }
        else { has[d] = 1; vn[d] = t.c[NC == 3 ? d >> 1 : 0][l2]; }
    }
}

// the workgroup's sum of every thread's v[N] by the steps 2 and 3 of the header: valid in thread 0 (one use per kernel)
template <int N>
__device__ __forceinline__ void poisson_block_sum(double v[N])
{
    __shared__ double s_w[kPoiThreads / 64][N];
    xor_butterfly<N>(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_w[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double s = s_w[0][k];
#pragma unroll
            for (int w = 1; w < kPoiThreads / 64; ++w) s = s + s_w[w][k];
            v[k] = s;
        }
    }
}

__global__ __launch_bounds__(256) void poisson_neighbours_kernel(int B, const int32_t *__restrict__ blocks, int32_t *__restrict__ nb6)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 6 * (size_t)B) return;
    const size_t k = i / 6;
    const int d = (int)(i % 6);
    int32_t b[3] = { blocks[3 * k], blocks[3 * k + 1], blocks[3 * k + 2] };
    b[d >> 1] += (d & 1) ? 1 : -1;
    nb6[i] = sls_poisson_find(B, blocks, b[0], b[1], b[2]);
}

// ---------------------------------------------------------------------------------------------------------------------
// solve
// ---------------------------------------------------------------------------------------------------------------------
struct PoissonState {
    double rz, step, beta, rr, bb, thr, iso, w1;
    unsigned long long done, iters, flags, pad;
};

struct PoissonVectors { float *b, *diag, *x, *r, *z, *p, *q; };

__global__ __launch_bounds__(kPoiThreads) void poisson_system_kernel(int B, const int32_t *__restrict__ nb6, const float4 *__restrict__ field,
                                                                     double alpha, PoissonVectors v, double *__restrict__ partials)
{
    __shared__ PoissonTile<3> t;
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t slot = (size_t)k * SLS_TSDF_BLOCK_VOXELS + l;
    const float4 f = field[slot];
    t.c[0][l] = f.x; t.c[1][l] = f.y; t.c[2][l] = f.z;
    poisson_stage_halo<3>(t, k, nb6, [&](int nbk, int vox, int comp) {
        return ((const float *)field)[4 * ((size_t)nbk * SLS_TSDF_BLOCK_VOXELS + vox) + comp];
    });
    float vn[6], bv, dv;
    int has[6];
    poisson_fetch<3>(t, l, vn, has);
    const float vc[3] = { f.x, f.y, f.z };
    sls_poisson_rhs(vc, vn, has, f.w, alpha, &bv, &dv);
    const float zv = sls_poisson_precond(bv, dv);
    v.b[slot] = bv; v.diag[slot] = dv; v.x[slot] = 0.0f; v.r[slot] = bv; v.z[slot] = zv; v.p[slot] = zv;
    double s[2] = { (double)bv * (double)bv, (double)bv * (double)zv };
    poisson_block_sum<2>(s);
    if (l == 0) { partials[k] = s[0]; partials[(size_t)B + k] = s[1]; }
}

enum { PR_INIT = 0, PR_STEP = 1, PR_BETA = 2, PR_ISO = 3 };

// one workgroup: the B block partials by step 4 of the header, then thread 0 advances the state
template <int MODE>
__global__ __launch_bounds__(kPoiThreads) void poisson_reduce_kernel(int B, const double *__restrict__ partials, PoissonState *state, double tol,
                                                                     unsigned long long *__restrict__ status)
{
    if ((MODE == PR_STEP || MODE == PR_BETA) && state->done) return;        // (uniform: written by an earlier launch)
    double v[2] = { 0.0, 0.0 };
    for (int k = threadIdx.x; k < B; k += kPoiThreads) {
        v[0] = v[0] + partials[k];
        if (MODE != PR_STEP) v[1] = v[1] + partials[(size_t)B + k];
    }
    poisson_block_sum<2>(v);
    if (threadIdx.x != 0) return;
    if (MODE == PR_INIT) {
        const double bb = v[0];
        state->bb = bb; state->rr = bb; state->rz = v[1]; state->step = 0.0; state->beta = 0.0; state->iso = 0.0; state->w1 = 0.0;
        state->thr = sls_poisson_threshold(tol, bb);
        state->iters = 0ull; state->pad = 0ull;
        if (bb == 0.0) { state->flags = SLS_POISSON_FLAG_CONVERGED | SLS_POISSON_FLAG_EMPTY; state->done = 1ull; }
        else if (bb <= state->thr) { state->flags = SLS_POISSON_FLAG_CONVERGED; state->done = 1ull; }
        else { state->flags = 0ull; state->done = 0ull; }
    } else if (MODE == PR_STEP) {
        if (!sls_poisson_pd(v[0])) { state->flags |= SLS_POISSON_FLAG_NOT_PD; state->done = 1ull; }
        else state->step = state->rz / v[0];
    } else if (MODE == PR_BETA) {
        state->rr = v[0];
        state->iters += 1ull;
        if (v[0] <= state->thr) { state->flags |= SLS_POISSON_FLAG_CONVERGED; state->done = 1ull; }
        else { state->beta = v[1] / state->rz; state->rz = v[1]; }
    } else {
        const double iso = v[1] == 0.0 ? 0.0 : v[0] / v[1];
        state->iso = iso; state->w1 = v[1];
        status[0] = state->iters; status[1] = state->flags; status[2] = (unsigned long long)B;
        status[3] = (unsigned long long)__double_as_longlong(state->rr);
        status[4] = (unsigned long long)__double_as_longlong(state->bb);
        status[5] = (unsigned long long)__double_as_longlong(iso);
        status[6] = (unsigned long long)__double_as_longlong(v[1]);
        status[7] = 0ull;
    }
}

// q = A p and the block partial of <p,q>.  From the second pass on p is made here, p = z + beta p_old at the block's own
// voxels (stored to p_cur) and again at the six face halos — the same operation on the same operands, so the same bits as a
// launch of its own would give; p_old and p_cur are the two halves of a ping-pong pair, so no workgroup reads what another
// writes.  FIRST: p_cur holds p already (poisson_system wrote it).
template <bool FIRST>
__global__ __launch_bounds__(kPoiThreads) void poisson_apply_kernel(const int32_t *__restrict__ nb6, const float *__restrict__ diag,
                                                                    const float *__restrict__ z, const float *__restrict__ p_old,
                                                                    float *p_cur, float *__restrict__ q,
                                                                    double *__restrict__ partials, const PoissonState *__restrict__ state)
{
    if (state->done) return;
    __shared__ PoissonTile<1> t;
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t slot = (size_t)k * SLS_TSDF_BLOCK_VOXELS + l;
    const double beta = FIRST ? 0.0 : state->beta;
    const auto direction = [&](size_t s) { return FIRST ? p_cur[s] : sls_poisson_axpy(z[s], beta, p_old[s]); };
    const float pc = direction(slot);
    if (!FIRST) p_cur[slot] = pc;
    t.c[0][l] = pc;
    poisson_stage_halo<1>(t, k, nb6, [&](int nbk, int vox, int) { return direction((size_t)nbk * SLS_TSDF_BLOCK_VOXELS + vox); });
    float pn[6];
    int has[6];
    poisson_fetch<1>(t, l, pn, has);
    const float qv = sls_poisson_apply(diag[slot], pc, pn, has);
    q[slot] = qv;
    double s[1] = { (double)pc * (double)qv };
    poisson_block_sum<1>(s);
    if (l == 0) partials[k] = s[0];
}

__global__ __launch_bounds__(kPoiThreads) void poisson_update_kernel(int B, PoissonVectors v, double *__restrict__ partials,
                                                                     const PoissonState *__restrict__ state)
{
    if (state->done) return;
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t slot = (size_t)k * SLS_TSDF_BLOCK_VOXELS + l;
    const double a = state->step;
    v.x[slot] = sls_poisson_axpy(v.x[slot], a, v.p[slot]);
    const float rv = sls_poisson_axmy(v.r[slot], a, v.q[slot]);
    const float zv = sls_poisson_precond(rv, v.diag[slot]);
    v.r[slot] = rv; v.z[slot] = zv;
    double s[2] = { (double)rv * (double)rv, (double)rv * (double)zv };
    poisson_block_sum<2>(s);
    if (l == 0) { partials[k] = s[0]; partials[(size_t)B + k] = s[1]; }
}

__global__ __launch_bounds__(kPoiThreads) void poisson_iso_kernel(int B, const float4 *__restrict__ field, const float *__restrict__ x,
                                                                  double *__restrict__ partials)
{
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t slot = (size_t)k * SLS_TSDF_BLOCK_VOXELS + l;
    const double w = (double)field[slot].w;
    double s[2] = { w * (double)x[slot], w * 1.0 };
    poisson_block_sum<2>(s);
    if (l == 0) { partials[k] = s[0]; partials[(size_t)B + k] = s[1]; }
}

__global__ __launch_bounds__(kPoiThreads) void poisson_chi_kernel(float *__restrict__ x, const PoissonState *__restrict__ state)
{
    const size_t slot = (size_t)blockIdx.x * SLS_TSDF_BLOCK_VOXELS + threadIdx.x;
    x[slot] = sls_poisson_shift(x[slot], state->iso);
}

__global__ void poisson_empty_status_kernel(unsigned long long *__restrict__ status)
{
    if (threadIdx.x < SLS_POISSON_STATUS_WORDS)
        status[threadIdx.x] = threadIdx.x == 1 ? (unsigned long long)(SLS_POISSON_FLAG_CONVERGED | SLS_POISSON_FLAG_EMPTY) : 0ull;
}

struct PoissonSolveScratch {
    int32_t *nb6;
    float *vec[7];
    double *partials;
    PoissonState *state;
    size_t total;
};

static PoissonSolveScratch poisson_solve_layout(int B, void *base)
{
    PoissonSolveScratch s;
    Arena a(base);
    const size_t S = (size_t)B * SLS_TSDF_BLOCK_VOXELS;
    s.nb6 = a.take<int32_t>(6 * (size_t)B);
    for (int i = 0; i < 7; ++i) s.vec[i] = a.take<float>(S);
    s.partials = a.take<double>(2 * (size_t)B);
    s.state = a.take<PoissonState>(1);
    s.total = a.off;
    return s;
}

size_t poisson_solve_scratch_bytes(int B) { return (B > 0 && B <= SLS_TSDF_MAX_BLOCKS) ? poisson_solve_layout(B, nullptr).total : 0; }

int launch_poisson_solve(int B, const int32_t *blocks, const float *field, double alpha, int iterations, double tol, float *out_chi,
                         uint64_t *out_status, void *scratch, hipStream_t st)
{
    unsigned long long *status = (unsigned long long *)out_status;
    if (B == 0) {
        hipLaunchKernelGGL(poisson_empty_status_kernel, dim3(1), dim3(64), 0, st, status);
        SLS_LAUNCH_CHECK("poisson_empty_status_kernel");
        return SLS_OK;
    }
    const PoissonSolveScratch s = poisson_solve_layout(B, scratch);
    PoissonVectors v = { s.vec[0], s.vec[1], out_chi, s.vec[2], s.vec[3], s.vec[4], s.vec[5] };           // x lives in out_chi
    float *const p2[2] = { s.vec[4], s.vec[6] };            // the ping-pong pair of p: pass `it` makes p in p2[it & 1]
    const float4 *f4 = (const float4 *)field;
    const dim3 grid(B), block(kPoiThreads);
    hipLaunchKernelGGL(poisson_neighbours_kernel, grid_for(6 * (size_t)B, 256), dim3(256), 0, st, B, blocks, s.nb6);
    SLS_LAUNCH_CHECK("poisson_neighbours_kernel");
    hipLaunchKernelGGL(poisson_system_kernel, grid, block, 0, st, B, (const int32_t *)s.nb6, f4, alpha, v, s.partials);
    SLS_LAUNCH_CHECK("poisson_system_kernel");
    hipLaunchKernelGGL(poisson_reduce_kernel<PR_INIT>, dim3(1), block, 0, st, B, (const double *)s.partials, s.state, tol, status);
    SLS_LAUNCH_CHECK("poisson_reduce_kernel");
    for (int it = 0; it < iterations; ++it) {
        v.p = p2[it & 1];
        if (it == 0)
            hipLaunchKernelGGL(poisson_apply_kernel<true>, grid, block, 0, st, (const int32_t *)s.nb6, (const float *)v.diag,
                               (const float *)v.z, (const float *)nullptr, v.p, v.q, s.partials, (const PoissonState *)s.state);
        else
            hipLaunchKernelGGL(poisson_apply_kernel<false>, grid, block, 0, st, (const int32_t *)s.nb6, (const float *)v.diag,
                               (const float *)v.z, (const float *)p2[(it - 1) & 1], v.p, v.q, s.partials, (const PoissonState *)s.state);
        SLS_LAUNCH_CHECK("poisson_apply_kernel");
        hipLaunchKernelGGL(poisson_reduce_kernel<PR_STEP>, dim3(1), block, 0, st, B, (const double *)s.partials, s.state, tol, status);
        SLS_LAUNCH_CHECK("poisson_reduce_kernel");
        hipLaunchKernelGGL(poisson_update_kernel, grid, block, 0, st, B, v, s.partials, (const PoissonState *)s.state);
        SLS_LAUNCH_CHECK("poisson_update_kernel");
        hipLaunchKernelGGL(poisson_reduce_kernel<PR_BETA>, dim3(1), block, 0, st, B, (const double *)s.partials, s.state, tol, status);
        SLS_LAUNCH_CHECK("poisson_reduce_kernel");
    }
    hipLaunchKernelGGL(poisson_iso_kernel, grid, block, 0, st, B, f4, (const float *)v.x, s.partials);
    SLS_LAUNCH_CHECK("poisson_iso_kernel");
    hipLaunchKernelGGL(poisson_reduce_kernel<PR_ISO>, dim3(1), block, 0, st, B, (const double *)s.partials, s.state, tol, status);
    SLS_LAUNCH_CHECK("poisson_reduce_kernel");
    hipLaunchKernelGGL(poisson_chi_kernel, grid, block, 0, st, v.x, (const PoissonState *)s.state);
    SLS_LAUNCH_CHECK("poisson_chi_kernel");
    return SLS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// density
// ---------------------------------------------------------------------------------------------------------------------
// src: rows of `stride` floats, component comp (the field's W: 4, 3; a density array: 1, 0)
__global__ __launch_bounds__(kPoiThreads) void poisson_smooth_kernel(const int32_t *__restrict__ nb6, const float *__restrict__ src, int stride,
                                                                     int comp, float *__restrict__ dst)
{
    __shared__ PoissonTile<1> t;
    const int k = blockIdx.x, l = threadIdx.x;
    const size_t slot = (size_t)k * SLS_TSDF_BLOCK_VOXELS + l;
    const float dc = src[slot * (size_t)stride + comp];
    t.c[0][l] = dc;
    poisson_stage_halo<1>(t, k, nb6, [&](int nbk, int vox, int) {
        return src[((size_t)nbk * SLS_TSDF_BLOCK_VOXELS + vox) * (size_t)stride + comp];
    });
    float dn[6];
    int has[6];
    poisson_fetch<1>(t, l, dn, has);
    dst[slot] = sls_poisson_smooth(dc, dn, has);
}

__global__ __launch_bounds__(kPoiThreads) void poisson_weight_kernel(const float4 *__restrict__ field, float *__restrict__ dst)
{
    const size_t slot = (size_t)blockIdx.x * SLS_TSDF_BLOCK_VOXELS + threadIdx.x;
    dst[slot] = field[slot].w;
}

struct PoissonDensityScratch {
    int32_t *nb6;
    float *tmp;
    size_t total;
};

static PoissonDensityScratch poisson_density_layout(int B, void *base)
{
    PoissonDensityScratch s;
    Arena a(base);
    s.nb6 = a.take<int32_t>(6 * (size_t)B);
    s.tmp = a.take<float>((size_t)B * SLS_TSDF_BLOCK_VOXELS);
    s.total = a.off;
    return s;
}

size_t poisson_density_scratch_bytes(int B) { return (B > 0 && B <= SLS_TSDF_MAX_BLOCKS) ? poisson_density_layout(B, nullptr).total : 0; }

int launch_poisson_density(int B, const int32_t *blocks, const float *field, int sweeps, float *out_density, void *scratch, hipStream_t st)
{
    const dim3 grid(B), block(kPoiThreads);
    if (sweeps == 0) {
        hipLaunchKernelGGL(poisson_weight_kernel, grid, block, 0, st, (const float4 *)field, out_density);
        SLS_LAUNCH_CHECK("poisson_weight_kernel");
        return SLS_OK;
    }
    const PoissonDensityScratch s = poisson_density_layout(B, scratch);
    hipLaunchKernelGGL(poisson_neighbours_kernel, grid_for(6 * (size_t)B, 256), dim3(256), 0, st, B, blocks, s.nb6);
    SLS_LAUNCH_CHECK("poisson_neighbours_kernel");
    const float *src = field;
    for (int i = 1; i <= sweeps; ++i) {                     // the last sweep lands in out_density
        float *dst = ((sweeps - i) & 1) ? s.tmp : out_density;
        hipLaunchKernelGGL(poisson_smooth_kernel, grid, block, 0, st, (const int32_t *)s.nb6, src, i == 1 ? 4 : 1, i == 1 ? 3 : 0, dst);
        SLS_LAUNCH_CHECK("poisson_smooth_kernel");
        src = dst;
    }
    return SLS_OK;
}

}  // namespace sls
