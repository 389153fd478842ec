/*
 * sls_poisson_math.h — the arithmetic of screened Poisson surface reconstruction over the sparse block volume
 * (sls_poisson_splat, sls_poisson_solve, sls_poisson_density), shared by the HIP kernels (csrc/sls_poisson.hip), by a host
 * program and by the NumPy restatement (tests/poisson_ref.py), which reproduce the kernels' results bit for bit.
 * DESIGN.md section 2, "Poisson volume", states the contract.
 *
 * THE RULE that makes this possible (as in sls_icp_math.h): + - * / and floor alone, every sum in ONE stated order, no
 * implicit fma (build with -ffp-contract=off).  Stored values are float32; every operation on them is done in float64
 * from the float32 operands and rounded to float32 ONCE.
 *
 * WHAT IT IS NOT: a uniform-resolution band, not Kazhdan's adaptive octree; trilinear splats, not B-splines; no Dirichlet
 * envelope; not compared against Open3D, which is not a dependency.
 *
 * ---- the grid ------------------------------------------------------------------------------------------------------
 * The TSDF volume's (sls_tsdf_math.h): block b covers origin + 8 h [b, b + 1), voxel l = x | y << 3 | z << 6, blocks in
 * ascending key order; the node of global voxel coordinate g sits at origin + (g + 0.5) h, which is sls_tsdf_centre.
 * The six directions d = 0 .. 5 are -x, +x, -y, +y, -z, +z: axis d >> 1, towards + iff d & 1.  A neighbour is PRESENT
 * iff its block exists; deg_v is the number of present neighbours (3 at least: a block is 8 voxels wide).
 *
 * ---- 1. splat (sls_poisson_splat) -----------------------------------------------------------------------------------
 * Point i with six finite floats p, n:  u_a = ((double)p_a - o_a) / h - 0.5,  i_a = floor(u_a),  f_a = u_a - i_a; the
 * cell i is IN RANGE iff floor(i_a / 8) and floor((i_a + 1) / 8) lie inside (-2^20, 2^20) on every axis.  Corner
 * c = 0 .. 7 has the offset d = (c & 1, c >> 1 & 1, c >> 2) and the weight w_c = (wx wy) wz, w_a = d_a ? f_a : 1 - f_a,
 * float64.  Node i + d receives w_c (density W) and w_c (double)n_a (field V).  A contribution to a node whose block is
 * absent is dropped; A POINT WHOSE CELL i LIES IN NO BLOCK IS DROPPED WHOLE (its cell has no slot to be sorted into; with
 * the allocator's margin of one voxel or more this never happens to a point the blocks were allocated from).
 * The sum at node g has ONE order: the cells g - d(c) for c = 0 .. 7; inside a cell ascending input index; the four sums
 * (Vx, Vy, Vz, W) float64 from zero, each rounded once to float32.  Status: points with a non-finite value, points out of
 * range, points with at least one dropped corner (the points dropped whole among them), 1.
 *
 * ---- 2. system ------------------------------------------------------------------------------------------------------
 * Least squares over the edges of the band: minimise  sum_edges (chi_j - chi_i - g_ij)^2 + alpha sum_v W_v chi_v^2,  an
 * edge (v, v + e_a) existing iff both blocks do, g = 0.5 ((double)V_a(v) + (double)V_a(v + e_a)) (the lower voxel first;
 * h is not folded in: it scales chi, not its zero set).  Normal equations (L + alpha diag(W)) chi = b:
 *   b_v    = float64 from zero over the present directions in the order 0 .. 5:  s <- s + g for a - direction (the edge
 *            arrives at v), s <- s - g for a + direction (it leaves v); rounded once                    sls_poisson_rhs
 *   diag_v = (float)((double)deg_v + alpha (double)W_v)
 *   (A p)_v = (float)(((double)diag_v (double)p_v - p_n0) - p_n1 ...) over the present directions in order  sls_poisson_apply
 * alpha must be finite and > 0: at alpha = 0 the matrix has a constant null vector per connected component.
 *
 * ---- 3. solve -------------------------------------------------------------------------------------------------------
 * Jacobi-preconditioned conjugate gradients from x = 0, float32 vectors:
 *   r = b, z_v = (float)((double)r_v / (double)diag_v), p = z, rz = <r,z>, bb = <b,b>, rr = bb, thr = (tol tol) bb
 *   bb == 0: flags = CONVERGED | EMPTY, ended.   rr <= thr: CONVERGED, ended.
 *   pass:  q = A p;  pq = <p,q>;  !(pq > 0) or pq not finite: NOT_PD, ended, x kept
 *          a = rz / pq;  x_v = (float)((double)x_v + a (double)p_v);  r_v = (float)((double)r_v - a (double)q_v);  z = r / diag
 *          rr = <r,r>, rz' = <r,z>, iterations += 1;  rr <= thr: CONVERGED, ended
 *          beta = rz' / rz;  p_v = (float)((double)z_v + beta (double)p_v);  rz = rz'
 * at most `iterations` passes; once ended the remaining passes change nothing.
 * THE INNER PRODUCT <a,b> — the order is part of the rule (SLS_POISSON_REDUCE = 512 = 8 waves of 64):
 *   1. voxel l of block k belongs to lane l % 64 of wave l / 64 and holds the exact float64 product (double)a (double)b;
 *   2. a wave sums its 64 lanes by the xor butterfly with the offsets 32, 16, 8, 4, 2, 1 (the sum of a balanced tree that
 *      pairs l with l + 32 first);
 *   3. the eight wave sums are added ascending, ((w0 + w1) + w2) ... + w7: one partial per block;
 *   4. the final step runs 512 threads: thread t adds the partials t, t + 512, t + 1024, ... in this order starting from
 *      zero, and the 512 thread sums are added by the steps 2 and 3 again (the ICP sums' order at 512 wide).
 *
 * ---- 4. iso-level ---------------------------------------------------------------------------------------------------
 * iso = <W,x> / <W,1> (the same sums), 0 if <W,1> == 0 — the mean of x at the samples; chi_v = (float)((double)x_v - iso).
 * chi < 0 is inside when the normals point to free space.
 *
 * ---- 5. density -----------------------------------------------------------------------------------------------------
 * D = W after `sweeps` sweeps of  D_v <- (float)(((double)D_v + D_n0 + ...) / (double)(1 + deg_v)), the present directions
 * in order, every voxel from the previous sweep's values.
 *
 * DEFAULTS (screening alpha = 4, tol = 1e-4, iterations = 300, a margin of 3 voxels, 2 density sweeps) are a JUDGEMENT, not
 * taken from any reference.
 *
 * Rules for users of this header: no fast-math, -ffp-contract=off.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_POISSON_MATH_H
#define SLS_POISSON_MATH_H

#include <string.h>

#include "sls_tsdf_math.h"

#define SLS_POISSON_REDUCE 512
#ifndef SLS_POISSON_FLAG_CONVERGED
#define SLS_POISSON_FLAG_CONVERGED 1    /* (include/sls_abi.h defines the same) */
#define SLS_POISSON_FLAG_NOT_PD 2
#define SLS_POISSON_FLAG_EMPTY 4
#define SLS_POISSON_STATUS_WORDS 8
#endif
#if SLS_POISSON_FLAG_CONVERGED != 1 || SLS_POISSON_FLAG_NOT_PD != 2 || SLS_POISSON_FLAG_EMPTY != 4 || SLS_POISSON_STATUS_WORDS != 8
#error "include/sls_abi.h and include/sls_poisson_math.h disagree on the SLS_POISSON_* constants"
#endif

/* index of block (bx, by, bz) in the sorted list, -1 when it is absent (bisection by key) */
SLS_HD int sls_poisson_find(int B, const int32_t *blocks, int32_t bx, int32_t by, int32_t bz)
{
    const uint64_t want = sls_tsdf_key(bx, by, bz);
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const uint64_t key = sls_tsdf_key(blocks[3 * (size_t)mid], blocks[3 * (size_t)mid + 1], blocks[3 * (size_t)mid + 2]);
        if (key < want) lo = mid + 1; else hi = mid;
    }
    if (lo >= B) return -1;
    return (blocks[3 * (size_t)lo] == bx && blocks[3 * (size_t)lo + 1] == by && blocks[3 * (size_t)lo + 2] == bz) ? lo : -1;
}

/* the cell of a finite point and its fractions: 1 when it is in range (cell, f written), else 0 */
SLS_HD int sls_poisson_cell(const float p[3], const double origin[3], double h, int32_t cell[3], double f[3])
{
    int ok = 1;
    for (int a = 0; a < 3; ++a) {
        const double u = ((double)p[a] - origin[a]) / h - 0.5;
        const double i = floor(u);
        if (sls_tsdf_index_ok(floor(i / 8.0)) && sls_tsdf_index_ok(floor((i + 1.0) / 8.0))) { cell[a] = (int32_t)i; f[a] = u - i; }
        else { cell[a] = 0; f[a] = 0.0; ok = 0; }
    }
    return ok;
}

SLS_HD double sls_poisson_corner_weight(const double f[3], int c)
{
    const double wx = (c & 1) ? f[0] : 1.0 - f[0], wy = (c & 2) ? f[1] : 1.0 - f[1], wz = (c & 4) ? f[2] : 1.0 - f[2];
    return (wx * wy) * wz;
}

/* floor(g / 8) and g mod 8 of a global voxel coordinate */
SLS_HD int32_t sls_poisson_block_of(int32_t g) { return g >> 3; }

/* The sort key of a cell: rank of its block << 9 | local voxel, or B << 9 when the block is absent.  *dropped: 1 when the
 * block of the cell or of one of its eight corner nodes is absent. */
SLS_HD uint32_t sls_poisson_cell_key(int B, const int32_t *blocks, const int32_t cell[3], int *dropped)
{
    const int32_t b[3] = { sls_poisson_block_of(cell[0]), sls_poisson_block_of(cell[1]), sls_poisson_block_of(cell[2]) };
    const int lx = cell[0] & 7, ly = cell[1] & 7, lz = cell[2] & 7;
    const int k = sls_poisson_find(B, blocks, b[0], b[1], b[2]);
    int drop = k < 0;
    const int edge = (lx == 7 ? 1 : 0) | (ly == 7 ? 2 : 0) | (lz == 7 ? 4 : 0);
    for (int m = 1; m < 8 && !drop; ++m)
        if ((m & edge) == m && sls_poisson_find(B, blocks, b[0] + (m & 1), b[1] + ((m >> 1) & 1), b[2] + (m >> 2)) < 0) drop = 1;
    *dropped = drop;
    return k < 0 ? (uint32_t)B << 9 : ((uint32_t)k << 9) | (uint32_t)(lx | ly << 3 | lz << 6);
}

/* one point's corner c into the four float64 sums of a node: from its fractions f, or from the point itself */
SLS_HD void sls_poisson_splat_addf(const double f[3], const float n[3], int c, double acc[4])
{
    const double w = sls_poisson_corner_weight(f, c);
    acc[0] += w * (double)n[0]; acc[1] += w * (double)n[1]; acc[2] += w * (double)n[2]; acc[3] += w;
}
SLS_HD void sls_poisson_splat_add(const float p[3], const float n[3], const double origin[3], double h, int c, double acc[4])
{
    int32_t cell[3];
    double f[3];
    sls_poisson_cell(p, origin, h, cell, f);
    sls_poisson_splat_addf(f, n, c, acc);
}

/* vn[d]: V_(d >> 1) of the neighbour in direction d, vc: V of the voxel itself, has[d]: the neighbour is present */
SLS_HD void sls_poisson_rhs(const float vc[3], const float vn[6], const int has[6], float W, double alpha, float *b, float *diag)
{
    double s = 0.0;
    int deg = 0;
    if (has[0]) { s = s + 0.5 * ((double)vn[0] + (double)vc[0]); ++deg; }
    if (has[1]) { s = s - 0.5 * ((double)vc[0] + (double)vn[1]); ++deg; }
    if (has[2]) { s = s + 0.5 * ((double)vn[2] + (double)vc[1]); ++deg; }
    if (has[3]) { s = s - 0.5 * ((double)vc[1] + (double)vn[3]); ++deg; }
    if (has[4]) { s = s + 0.5 * ((double)vn[4] + (double)vc[2]); ++deg; }
    if (has[5]) { s = s - 0.5 * ((double)vc[2] + (double)vn[5]); ++deg; }
    *b = (float)s;
    *diag = (float)((double)deg + alpha * (double)W);
}

SLS_HD float sls_poisson_apply(float diag, float pc, const float pn[6], const int has[6])
{
    double s = (double)diag * (double)pc;
    if (has[0]) s = s - (double)pn[0];
    if (has[1]) s = s - (double)pn[1];
    if (has[2]) s = s - (double)pn[2];
    if (has[3]) s = s - (double)pn[3];
    if (has[4]) s = s - (double)pn[4];
    if (has[5]) s = s - (double)pn[5];
    return (float)s;
}

SLS_HD float sls_poisson_smooth(float dc, const float dn[6], const int has[6])
{
    double s = (double)dc;
    int deg = 0;
    if (has[0]) { s = s + (double)dn[0]; ++deg; }
    if (has[1]) { s = s + (double)dn[1]; ++deg; }
    if (has[2]) { s = s + (double)dn[2]; ++deg; }
    if (has[3]) { s = s + (double)dn[3]; ++deg; }
    if (has[4]) { s = s + (double)dn[4]; ++deg; }
    if (has[5]) { s = s + (double)dn[5]; ++deg; }
    return (float)(s / (double)(1 + deg));
}

SLS_HD float sls_poisson_precond(float r, float diag) { return (float)((double)r / (double)diag); }
SLS_HD float sls_poisson_axpy(float x, double a, float p) { return (float)((double)x + a * (double)p); }
SLS_HD float sls_poisson_axmy(float r, double a, float q) { return (float)((double)r - a * (double)q); }
SLS_HD float sls_poisson_shift(float x, double iso) { return (float)((double)x - iso); }
SLS_HD double sls_poisson_threshold(double tol, double bb) { return (tol * tol) * bb; }
SLS_HD int sls_poisson_pd(double pq) { return pq > 0.0 && pq - pq == 0.0; }

/* the voxel the stencil of voxel l reaches in direction d: the same block (*outside = 0), or voxel l' of the neighbour block */
SLS_HD int sls_poisson_step(int l, int d, int *outside)
{
    const int sh = 3 * (d >> 1), c = (l >> sh) & 7;
    if (d & 1) { *outside = c == 7; return c == 7 ? l - (7 << sh) : l + (1 << sh); }
    *outside = c == 0;
    return c == 0 ? l + (7 << sh) : l - (1 << sh);
}

/* ---- serial host routines: the same functions in plain loops ------------------------------------------------------ */

/* nb6[6 k + d]: the block next to block k in direction d, -1 when absent */
SLS_HD void sls_poisson_neighbours_host(int B, const int32_t *blocks, int32_t *nb6)
{
    for (int k = 0; k < B; ++k)
        for (int d = 0; d < 6; ++d) {
            int32_t b[3] = { blocks[3 * (size_t)k], blocks[3 * (size_t)k + 1], blocks[3 * (size_t)k + 2] };
            b[d >> 1] += (d & 1) ? 1 : -1;
            nb6[6 * (size_t)k + d] = sls_poisson_find(B, blocks, b[0], b[1], b[2]);
        }
}

/* component `comp` of the row of `stride` floats of the voxel next to (k, l) in direction d; *has: it is present */
SLS_HD float sls_poisson_next_host(const float *arr, int stride, int comp, const int32_t *nb6, int k, int l, int d, int *has)
{
    int outside;
    const int l2 = sls_poisson_step(l, d, &outside);
    const int k2 = outside ? nb6[6 * (size_t)k + d] : k;
    *has = k2 >= 0;
    return k2 >= 0 ? arr[((size_t)k2 * 512 + (size_t)l2) * (size_t)stride + comp] : 0.0f;
}

/* the sum of 64 values by the butterfly's tree; v is overwritten */
SLS_HD double sls_poisson_tree64(double *v)
{
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

/* the steps 2 and 3 on 512 values; v is overwritten */
SLS_HD double sls_poisson_sum512(double *v)
{
    double s = sls_poisson_tree64(v);
    for (int w = 1; w < 8; ++w) s = s + sls_poisson_tree64(v + 64 * w);
    return s;
}

/* <a,b> over B blocks, rows of stride_a / stride_b floats (b null: ones) */
SLS_HD double sls_poisson_dot_host(int B, const float *a, int stride_a, const float *b, int stride_b)
{
    double t[SLS_POISSON_REDUCE], v[SLS_POISSON_REDUCE];
    for (int i = 0; i < SLS_POISSON_REDUCE; ++i) t[i] = 0.0;
    for (int k = 0; k < B; ++k) {
        for (int l = 0; l < 512; ++l) {
            const size_t s = (size_t)k * 512 + (size_t)l;
            v[l] = (double)a[s * (size_t)stride_a] * (b ? (double)b[s * (size_t)stride_b] : 1.0);
        }
        t[k % SLS_POISSON_REDUCE] = t[k % SLS_POISSON_REDUCE] + sls_poisson_sum512(v);
    }
    return sls_poisson_sum512(t);
}

/* Splat: field (B,512,4), status[4].  Work: keys[M], order[M], first[512 B + 1] (uint32). */
SLS_HD void sls_poisson_splat_host(int M, const float *xyz, const float *normals, int B, const int32_t *blocks, double h,
                                   const double origin[3], float *field, uint32_t *status, uint32_t *keys, uint32_t *order,
                                   uint32_t *first)
{
    const size_t S = (size_t)B * 512;
    status[0] = status[1] = status[2] = 0u; status[3] = 1u;
    for (size_t s = 0; s <= S; ++s) first[s] = 0u;
    for (int i = 0; i < M; ++i) {
        const float *p = xyz + 3 * (size_t)i, *n = normals + 3 * (size_t)i;
        int finite = 1;
        for (int a = 0; a < 3; ++a) finite = finite && p[a] - p[a] == 0.0f && n[a] - n[a] == 0.0f;
        keys[i] = (uint32_t)B << 9;
        if (!finite) { status[0] += 1u; continue; }
        int32_t cell[3];
        double f[3];
        if (!sls_poisson_cell(p, origin, h, cell, f)) { status[1] += 1u; continue; }
        int dropped;
        keys[i] = sls_poisson_cell_key(B, blocks, cell, &dropped);
        if (dropped) status[2] += 1u;
        if (keys[i] < ((uint32_t)B << 9)) first[keys[i] + 1u] += 1u;
    }
    for (size_t s = 0; s < S; ++s) first[s + 1] += first[s];
    for (int i = 0; i < M; ++i)                     /* ascending i: the stable order inside a cell */
        if (keys[i] < ((uint32_t)B << 9)) order[first[keys[i]]++] = (uint32_t)i;
    for (size_t s = S; s > 0; --s) first[s] = first[s - 1];     /* (the fill moved every start to its end) */
    first[0] = 0u;
    for (int k = 0; k < B; ++k) {
        int nb[8];
        for (int m = 0; m < 8; ++m)
            nb[m] = m == 0 ? k : sls_poisson_find(B, blocks, blocks[3 * (size_t)k] - (m & 1), blocks[3 * (size_t)k + 1] - ((m >> 1) & 1),
                                                  blocks[3 * (size_t)k + 2] - (m >> 2));
        for (int l = 0; l < 512; ++l) {
            const int x = l & 7, y = (l >> 3) & 7, z = l >> 6;
            double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
            for (int c = 0; c < 8; ++c) {
                const int cx = x - (c & 1), cy = y - ((c >> 1) & 1), cz = z - (c >> 2);
                const int kb = nb[(cx < 0 ? 1 : 0) | (cy < 0 ? 2 : 0) | (cz < 0 ? 4 : 0)];
                if (kb < 0) continue;
                const size_t slot = (size_t)kb * 512 + (size_t)((cx & 7) | (cy & 7) << 3 | (cz & 7) << 6);
                for (uint32_t q = first[slot]; q < first[slot + 1]; ++q)
                    sls_poisson_splat_add(xyz + 3 * (size_t)order[q], normals + 3 * (size_t)order[q], origin, h, c, acc);
            }
            float *row = field + 4 * ((size_t)k * 512 + (size_t)l);
            row[0] = (float)acc[0]; row[1] = (float)acc[1]; row[2] = (float)acc[2]; row[3] = (float)acc[3];
        }
    }
}

/* b and diag (B,512) of the field; nb6 from sls_poisson_neighbours_host */
SLS_HD void sls_poisson_system_host(int B, const int32_t *nb6, const float *field, double alpha, float *b, float *diag)
{
    for (int k = 0; k < B; ++k)
        for (int l = 0; l < 512; ++l) {
            const size_t s = (size_t)k * 512 + (size_t)l;
            float vn[6];
            int has[6];
            for (int d = 0; d < 6; ++d) vn[d] = sls_poisson_next_host(field, 4, d >> 1, nb6, k, l, d, &has[d]);
            sls_poisson_rhs(field + 4 * s, vn, has, field[4 * s + 3], alpha, b + s, diag + s);
        }
}

SLS_HD void sls_poisson_apply_host(int B, const int32_t *nb6, const float *diag, const float *p, float *q)
{
    for (int k = 0; k < B; ++k)
        for (int l = 0; l < 512; ++l) {
            const size_t s = (size_t)k * 512 + (size_t)l;
            float pn[6];
            int has[6];
            for (int d = 0; d < 6; ++d) pn[d] = sls_poisson_next_host(p, 1, 0, nb6, k, l, d, &has[d]);
            q[s] = sls_poisson_apply(diag[s], p[s], pn, has);
        }
}

/* The solve.  chi (B,512), status[SLS_POISSON_STATUS_WORDS]: iterations run, flags, B, the bits of <r,r>, <b,b>, iso and
 * <W,1>, 0.  Work: nb6[6 B] and vec[7 * 512 B] floats, which hold b, diag, x, r, z, p, q afterwards. */
SLS_HD void sls_poisson_solve_host(int B, const int32_t *blocks, const float *field, double alpha, int iterations, double tol,
                                   float *chi, uint64_t *status, int32_t *nb6, float *vec)
{
    const size_t S = (size_t)B * 512;
    float *b = vec, *diag = vec + S, *x = vec + 2 * S, *r = vec + 3 * S, *z = vec + 4 * S, *p = vec + 5 * S, *q = vec + 6 * S;
    sls_poisson_neighbours_host(B, blocks, nb6);
    sls_poisson_system_host(B, nb6, field, alpha, b, diag);
    for (size_t s = 0; s < S; ++s) { x[s] = 0.0f; r[s] = b[s]; z[s] = sls_poisson_precond(r[s], diag[s]); p[s] = z[s]; q[s] = 0.0f; }
    const double bb = sls_poisson_dot_host(B, b, 1, b, 1);
    double rz = sls_poisson_dot_host(B, r, 1, z, 1), rr = bb;
    const double thr = sls_poisson_threshold(tol, bb);
    uint64_t flags = 0u, iters = 0u;
    int ended = 0;
    if (bb == 0.0) { flags = SLS_POISSON_FLAG_CONVERGED | SLS_POISSON_FLAG_EMPTY; ended = 1; }
    else if (rr <= thr) { flags = SLS_POISSON_FLAG_CONVERGED; ended = 1; }
    for (int it = 0; it < iterations && !ended; ++it) {
        sls_poisson_apply_host(B, nb6, diag, p, q);
        const double pq = sls_poisson_dot_host(B, p, 1, q, 1);
        if (!sls_poisson_pd(pq)) { flags |= SLS_POISSON_FLAG_NOT_PD; break; }
        const double a = rz / pq;
        for (size_t s = 0; s < S; ++s) {
            x[s] = sls_poisson_axpy(x[s], a, p[s]);
            r[s] = sls_poisson_axmy(r[s], a, q[s]);
            z[s] = sls_poisson_precond(r[s], diag[s]);
        }
        rr = sls_poisson_dot_host(B, r, 1, r, 1);
        const double rz2 = sls_poisson_dot_host(B, r, 1, z, 1);
        iters += 1u;
        if (rr <= thr) { flags |= SLS_POISSON_FLAG_CONVERGED; break; }
        const double beta = rz2 / rz;
        for (size_t s = 0; s < S; ++s) p[s] = sls_poisson_axpy(z[s], beta, p[s]);
        rz = rz2;
    }
    const double wx = sls_poisson_dot_host(B, field + 3, 4, x, 1), w1 = sls_poisson_dot_host(B, field + 3, 4, (const float *)0, 0);
    const double iso = w1 == 0.0 ? 0.0 : wx / w1;
    for (size_t s = 0; s < S; ++s) chi[s] = sls_poisson_shift(x[s], iso);
    status[0] = iters; status[1] = flags; status[2] = (uint64_t)B;
    memcpy(&status[3], &rr, 8); memcpy(&status[4], &bb, 8); memcpy(&status[5], &iso, 8); memcpy(&status[6], &w1, 8);
    status[7] = 0u;
}

/* density (B,512); work: nb6[6 B], tmp[512 B] */
SLS_HD void sls_poisson_density_host(int B, const int32_t *blocks, const float *field, int sweeps, float *density, int32_t *nb6,
                                     float *tmp)
{
    const size_t S = (size_t)B * 512;
    sls_poisson_neighbours_host(B, blocks, nb6);
    float *cur = (sweeps & 1) ? tmp : density;
    for (size_t s = 0; s < S; ++s) cur[s] = field[4 * s + 3];
    for (int it = 0; it < sweeps; ++it) {
        float *nxt = cur == tmp ? density : tmp;
        for (int k = 0; k < B; ++k)
            for (int l = 0; l < 512; ++l) {
                float dn[6];
                int has[6];
                for (int d = 0; d < 6; ++d) dn[d] = sls_poisson_next_host(cur, 1, 0, nb6, k, l, d, &has[d]);
                nxt[(size_t)k * 512 + (size_t)l] = sls_poisson_smooth(cur[(size_t)k * 512 + (size_t)l], dn, has);
            }
        cur = nxt;
    }
}

#endif /* SLS_POISSON_MATH_H */
