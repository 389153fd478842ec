/*
 * sls_simplify_math.h — the rules of mesh simplification by vertex clustering (sls_mesh_simplify), shared by the HIP
 * kernels (csrc/sls_simplify.hip) and by any CPU checker that wants to reproduce their results (tests/simplify_ref.py
 * compiles this header and restates it in NumPy).  DESIGN.md section 2, "Mesh simplification", states the contract.  It
 * restates what Open3D documents for simplify_vertex_clustering(voxel_size, contraction = Average | Quadric); where that
 * leaves something open (the grid's origin, the order of the outputs, the quadric's regularisation) this header defines it.
 *
 * Inputs: vertices V x 3 float32, faces T x 3 int32, voxel_size h (float64, finite, > 0), contraction (0: average,
 * 1: quadric), regularisation lambda (float64, finite, >= 0; used by the quadric alone).
 *
 * ---- 1. live vertices ------------------------------------------------------------------------------------------------
 * A triangle is degenerate by sls_mesh_degenerate (two equal indices, or an index outside [0, V)).  A vertex is LIVE iff
 * a non-degenerate triangle references it; everything below sees live vertices only (face rows of -1 and vertex rows
 * that nothing references take no part: the stage runs behind sls_mesh_filter at capacity).  A live vertex with a
 * non-finite coordinate is counted (status word 2), belongs to no cluster, and a triangle that references it is treated
 * as degenerate from here on — its other vertices stay live: liveness is decided by sls_mesh_degenerate alone.
 *
 * ---- 2. the voxel of a vertex ----------------------------------------------------------------------------------------
 * sls_cloud_math.h as it stands: mn_a = the float32 minimum of axis a over the FINITE LIVE vertices, then
 * sls_voxel_origin, sls_voxel_index, sls_voxel_key.  A finite live vertex with an index >= 2^21 is counted (status word 3)
 * and gets key 0; where that count is not 0 the outputs are unspecified, but every access stays in bounds.  Clusters are
 * the distinct keys, numbered in ascending key order.
 *
 * ---- 3. faces --------------------------------------------------------------------------------------------------------
 * Triangle t becomes (c(f0), c(f1), c(f2)); it is dropped as COLLAPSED when these are not three distinct clusters,
 * otherwise rotated (never reflected: sls_simplify_rotate) so that its smallest cluster id comes first.  Among the
 * triangles with the same rotated triple the one of lowest input index stays, the others are dropped as DUPLICATES (a
 * triple of opposite orientation is a different triple).  Kept triangles leave in input order.  A cluster SURVIVES iff a
 * kept triangle references it; the surviving clusters, renumbered 0 .. V'-1 in ascending key order, are the output
 * vertices.  vmap[v] is the output vertex of input vertex v, or -1 when v is not live, not finite, or its cluster did not
 * survive.
 *
 * ---- the order of every float64 sum ----------------------------------------------------------------------------------
 * A cluster's sums run over a SEGMENT of items in a fixed order: its finite live vertices in ascending vertex index
 * (rule 4), its corners in ascending corner id 3 t + k (rule 5).  A segment of n <= SLS_SIMPLIFY_LONG (64) items is added
 * one after the other, starting from +0.0.  A longer one is split over 64 lanes: lane l adds the items l, l + 64, l + 128,
 * ... one after the other starting from +0.0, then for off = 32, 16, 8, 4, 2, 1 every lane l replaces its partial sum by
 * part[l] + part[l ^ off] (all lanes at once: a butterfly; a + b == b + a, so every lane ends with the same bits).  Every
 * word of a sum (3 for the mean, 9 for the quadric) follows that order on its own.
 *
 * ---- 4. position, average --------------------------------------------------------------------------------------------
 * m_a = (the sum of (double)p_a over the cluster's finite live vertices) / (double)count; the output is (float)m_a.
 *
 * ---- 5. position, quadric --------------------------------------------------------------------------------------------
 * Every non-degenerate triangle whose three vertices are finite (sls_simplify_quadric): c = e1 x e2 and
 * L = sqrt((cx cx + cy cy) + cz cz) exactly as sls_mesh_face_area orders them; if !(L > 0) or L is not finite it
 * contributes nothing.  Otherwise n = c / L (three divisions), w = 0.5 L, s = (nx p0x + ny p0y) + nz p0z, and each of its
 * three corners adds  w n n^T = (wx nx, wx ny, wx nz, wy ny, wy nz, wz nz) with wx = w nx ...,  and  (w s) n  to the
 * cluster of that corner's vertex: a triangle with two corners in one cluster adds twice, collapsed triangles add too.
 * Then (sls_simplify_solve), with m the float64 mean of rule 4:
 *   tr = (A00 + A11) + A22,  M = A + (lambda tr) I,  r_a = g_a - ((A_a0 mx + A_a1 my) + A_a2 mz),
 *   delta = adj(M) r / det(M)  — every product and sum as the function writes them —  and the output is
 *   (float)(m_a + delta_a).
 * The cluster falls back to rule 4, and is counted (status word 6; surviving clusters only — no other position is ever
 * written), when !(tr > 0), !(det > 0), a delta_a is not finite, or some |delta_a| > voxel_size.
 *
 * Status: [V', T', non-finite live vertices, live vertices beyond 2^21, collapsed, duplicates, quadric fallbacks, 1].
 *
 * Rules for users of this header, as for sls_mesh_math.h: compile with -ffp-contract=off, no fast-math (float64 division
 * and square root are correctly rounded as they are).  Plain C99 / HIP device compatible.
 */
#ifndef SLS_SIMPLIFY_MATH_H
#define SLS_SIMPLIFY_MATH_H

#include <math.h>
#include <stdint.h>

#include "sls_cloud_math.h"
#include "sls_mesh_math.h"

#define SLS_SIMPLIFY_LONG 64       /* a segment of more items is summed by 64 lanes and a butterfly */
#define SLS_SIMPLIFY_DBL_MAX 1.7976931348623157e308

SLS_HD int sls_simplify_finite(float v)
{
    return fabsf(v) <= 3.402823466e+38f;
}

/* 0 and the rotation of (c0, c1, c2) with its smallest entry first when the three are distinct; 1 (collapsed) otherwise */
SLS_HD int sls_simplify_rotate(const int32_t c[3], int32_t r[3])
{
    if (c[0] == c[1] || c[1] == c[2] || c[2] == c[0]) return 1;
    if (c[0] < c[1] && c[0] < c[2]) { r[0] = c[0]; r[1] = c[1]; r[2] = c[2]; }
    else if (c[1] < c[2]) { r[0] = c[1]; r[1] = c[2]; r[2] = c[0]; }
    else { r[0] = c[2]; r[1] = c[0]; r[2] = c[1]; }
    return 0;
}

/* what each corner of the triangle adds: q[0..5] = w n n^T (xx, xy, xz, yy, yz, zz), q[6..8] = (w s) n; 0 when the
 * triangle contributes nothing (q is then untouched) */
SLS_HD int sls_simplify_quadric(const float p0[3], const float p1[3], const float p2[3], double q[9])
{
    const double e1x = (double)p1[0] - (double)p0[0], e1y = (double)p1[1] - (double)p0[1], e1z = (double)p1[2] - (double)p0[2];
    const double e2x = (double)p2[0] - (double)p0[0], e2y = (double)p2[1] - (double)p0[1], e2z = (double)p2[2] - (double)p0[2];
    const double cx = e1y * e2z - e1z * e2y;
    const double cy = e1z * e2x - e1x * e2z;
    const double cz = e1x * e2y - e1y * e2x;
    const double L = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(L > 0.0) || !(L <= SLS_SIMPLIFY_DBL_MAX)) return 0;
    const double nx = cx / L, ny = cy / L, nz = cz / L;
    const double w = 0.5 * L;
    const double s = (nx * (double)p0[0] + ny * (double)p0[1]) + nz * (double)p0[2];
    const double wx = w * nx, wy = w * ny, wz = w * nz, ws = w * s;
    q[0] = wx * nx; q[1] = wx * ny; q[2] = wx * nz; q[3] = wy * ny; q[4] = wy * nz; q[5] = wz * nz;
    q[6] = ws * nx; q[7] = ws * ny; q[8] = ws * nz;
    return 1;
}

/* the mean of a cluster from its sum */
SLS_HD double sls_simplify_mean(double sum, uint32_t count)
{
    return sum / (double)count;
}

/* the quadric position of a cluster from its sums q (as sls_simplify_quadric lays them out) and its mean m; returns 1 and
 * the mean's position when the cluster falls back */
SLS_HD int sls_simplify_solve(const double q[9], const double m[3], double lambda, double voxel_size, float out[3])
{
    out[0] = (float)m[0]; out[1] = (float)m[1]; out[2] = (float)m[2];
    const double tr = (q[0] + q[3]) + q[5];
    if (!(tr > 0.0)) return 1;
    const double reg = lambda * tr;
    const double m00 = q[0] + reg, m11 = q[3] + reg, m22 = q[5] + reg, m01 = q[1], m02 = q[2], m12 = q[4];
    const double rx = q[6] - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2]);
    const double ry = q[7] - ((q[1] * m[0] + q[3] * m[1]) + q[4] * m[2]);
    const double rz = q[8] - ((q[2] * m[0] + q[4] * m[1]) + q[5] * m[2]);
    const double c00 = m11 * m22 - m12 * m12;
    const double c01 = m02 * m12 - m01 * m22;
    const double c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02;
    const double c12 = m01 * m02 - m00 * m12;
    const double c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    if (!(det > 0.0)) return 1;
    const double dx = ((c00 * rx + c01 * ry) + c02 * rz) / det;
    const double dy = ((c01 * rx + c11 * ry) + c12 * rz) / det;
    const double dz = ((c02 * rx + c12 * ry) + c22 * rz) / det;
    if (!(fabs(dx) <= voxel_size) || !(fabs(dy) <= voxel_size) || !(fabs(dz) <= voxel_size)) return 1;   /* a NaN included */
    out[0] = (float)(m[0] + dx); out[1] = (float)(m[1] + dy); out[2] = (float)(m[2] + dz);
    return 0;
}

#endif /* SLS_SIMPLIFY_MATH_H */
