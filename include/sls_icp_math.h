/*
 * sls_icp_math.h — the arithmetic of the registration of two clouds (sls_cloud_icp): Gauss-Newton point-to-plane or
 * point-to-point ICP on exact nearest neighbours with a hard distance gate.  Shared by the HIP kernels, by a host program
 * and by the NumPy restatement (tests/icp_ref.py), which reproduce the kernels' results bit for bit.
 *
 * THE RULE that makes this possible (as in sls_normals_math.h): float64 throughout, + - * / and sqrt alone — no libm call
 * such as sin or cos, whose device and host versions differ — every sum in one fixed order, no implicit fma (build with
 * -ffp-contract=off).  That is why the pose is updated by the Cayley map and not by the exponential.
 *
 * THE POSE is 12 doubles T[0 .. 11], the row-major 3 x 4 matrix target_T_source = [R | t].
 *
 * TRANSFORM of a source point p (float32) — sls_icp_transform:
 *     p'_a = (float)(((T[4a] * p_x + T[4a+1] * p_y) + T[4a+2] * p_z) + T[4a+3]),   a = 0, 1, 2,
 * every product and sum float64, ONE rounding to float32 at the end.  p' is what the search sees and what the residual uses.
 *
 * ASSOCIATION: sls_nn_query's rule unchanged (sls_nn_math.h): float32 d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) between p'
 * and every target, the lowest target index among equally near ones.  The pair is an INLIER iff d2 <= g2 with
 * g2 = max_distance * max_distance, ONE float32 product (as sls_outlier_radius takes radius * radius) — sls_icp_gate2.
 * NO ROBUST WEIGHT is applied: the gate is the only outlier rule, every inlier counts with weight 1.
 *
 * TERMS of one inlier, for the left increment T <- exp(xi) T, xi = (v, w) — sls_icp_terms.  With q the target point, n its
 * normal, all promoted from float32 to float64, and d = p' - q:
 *   point-to-plane (SLS_ICP_PLANE), one row:  r = (n_x d_x + n_y d_y) + n_z d_z,  J = [n, p' x n],
 *       (p' x n)_x = p'_y n_z - p'_z n_y, _y = p'_z n_x - p'_x n_z, _z = p'_x n_y - p'_y n_x;
 *   point-to-point (SLS_ICP_POINT), three rows in the order x, y, z:  r = d_a,  J = [e_a, row a of -[p']x],
 *       -[p']x = [0, p'_z, -p'_y;  -p'_z, 0, p'_x;  p'_y, -p'_x, 0].
 * Starting from 29 zeros every row adds, in this order: acc[k] += J_a * J_c for the 21 pairs a <= c, row-major (k = 0: (0,0),
 * 1: (0,1), ... 5: (0,5), 6: (1,1), ...), acc[21 + a] += J_a * r, acc[27] += r * r; the point then adds 1 to acc[28].  A pair
 * that is not an inlier, and a thread without a point, contributes 29 zeros.  The zeros and ones of a point-to-point row are
 * multiplied like any other number: there is ONE row routine.
 *
 * SUM of the terms over the source cloud — the order is part of the rule (SLS_ICP_BLOCK = 256 = 4 waves of 64):
 *   1. point i belongs to lane i % 64 of wave (i / 64) % 4 of block i / 256: one point per thread, ceil(Ms / 256) blocks;
 *   2. a wave sums its 64 lanes by the xor butterfly with the offsets 32, 16, 8, 4, 2, 1 (x_l <- x_l + x_(l ^ off); a + b
 *      == b + a, so all lanes end with the same bits: the sum of a balanced tree that pairs l with l + 32 first);
 *   3. a block adds its 4 wave sums in wave order, ((w0 + w1) + w2) + w3: one partial row of 29 per block;
 *   4. the solve step runs SLS_ICP_BLOCK threads: thread t adds the partial rows t, t + 256, t + 512, ... in this order
 *      starting from zeros (beyond 256 blocks, Ms > 65 536, a thread takes a second round), and the 256 thread sums
 *      are added by the steps 2 and 3 again.
 *
 * SOLVE — sls_icp_solve, on the 29 sums S: H = the symmetric 6 x 6 matrix of S[0 .. 20], b = S[21 .. 26].
 *   fewer inliers than min_inliers (S[28] < min_inliers): SLS_ICP_FLAG_FEW, the pose is kept;
 *   H[a][a] += damping, then the Cholesky factor L (lower, row by row; each entry H[a][c] minus the products L[a][k] L[c][k],
 *   k ascending, subtracted one by one); a pivot that is not > 0 (or is NaN): SLS_ICP_FLAG_NOT_PD, the pose is kept;
 *   L y = -b forwards, L^T xi = y backwards, the products again subtracted one by one in ascending (descending) k; a step
 *   with a NaN or an infinity in it counts as not positive definite too;
 *   UPDATE by the Cayley map with a = w / 2:  s = (a_x a_x + a_y a_y) + a_z a_z,  den = 1 + s,  c = 1 - s,
 *       dR = [ (c + 2 a_x a_x) / den, 2 (a_x a_y - a_z) / den, 2 (a_x a_z + a_y) / den;
 *              2 (a_x a_y + a_z) / den, (c + 2 a_y a_y) / den, 2 (a_y a_z - a_x) / den;
 *              2 (a_x a_z - a_y) / den, 2 (a_y a_z + a_x) / den, (c + 2 a_z a_z) / den ]
 *     = (I - [a]x)^-1 (I + [a]x): an exact rotation about w by 2 atan(|w| / 2) — |w| to second order — with no sin or cos.
 *     R <- dR R, t <- dR t + v (each entry ((x0 + x1) + x2) [+ v]).  A retraction other than exp does not move the fixed
 *     point of Gauss-Newton (xi = 0 there), it only changes the path to it at third order in |w|.  R is NOT
 *     re-orthonormalised: a product of k exact-to-round-off rotations is off by about k eps.
 *   CONVERGED (SLS_ICP_FLAG_CONVERGED) when sqrt((w_x w_x + w_y w_y) + w_z w_z) < eps_rot and the same of v < eps_trans;
 *     the update that met the test IS applied.
 *
 * THE LOOP (sls_cloud_icp): `iterations` = n means up to n updates followed by ONE evaluation pass — a linearisation at the
 * final pose, whose sums, inlier count and association are the ones reported.  An update that converges, or a pass that
 * keeps the pose (FEW, NOT_PD), ends the updates; a pass that kept the pose IS the evaluation pass.  n = 0 is one
 * linearisation at the initial pose.
 *
 * Hard associations on noisy clouds can end in a CYCLE of period two instead of a fixed point: the pairs flip back and forth
 * between two poses (1e-4 apart on a room with 5 mm of noise).  The loop then runs all its iterations and ends without the
 * converged flag; nothing in the rule damps this.
 *
 * DEFAULTS (sls_icp_defaults): damping 1e-9, eps_rot 1e-7 rad, eps_trans 1e-7 (in the clouds' unit), min_inliers 6.  They
 * are a JUDGEMENT, not taken from any reference: the damping is far below the smallest curvature of a well-posed metre-scale
 * problem (H grows with the inlier count) and only keeps a nearly unobservable freedom from exploding; the thresholds sit
 * a decade above what the float32 rounding of p' lets a step reach (about 1e-8 of a metre-scale coordinate per point, less
 * after averaging); six inliers are the fewest that can hold six freedoms.
 *
 * Rules for users of this header: no fast-math, -ffp-contract=off, HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt.
 * Coordinates and normals must be finite.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_ICP_MATH_H
#define SLS_ICP_MATH_H

#include "sls_nn_math.h"

#define SLS_ICP_PLANE 0
#define SLS_ICP_POINT 1
#define SLS_ICP_TERMS 29            /* 21 + 6 + 1 + 1 */
#define SLS_ICP_BLOCK 256           /* points per block of the sum = threads of the solve step */
#ifndef SLS_ICP_FLAG_CONVERGED
#define SLS_ICP_FLAG_CONVERGED 1    /* (include/sls_abi.h defines the same) */
#define SLS_ICP_FLAG_FEW 2
#define SLS_ICP_FLAG_NOT_PD 4
#endif

#ifndef SLS_ICP_PARAMS_DEFINED
#define SLS_ICP_PARAMS_DEFINED
typedef struct SlsIcpParams {       /* (include/sls_abi.h defines the same) */
    int32_t method, iterations, min_inliers;
    float max_distance;
    double damping, eps_rot, eps_trans;
} SlsIcpParams;
#endif

SLS_HD void sls_icp_defaults(SlsIcpParams *p)
{
    p->method = SLS_ICP_PLANE; p->iterations = 30; p->min_inliers = 6; p->max_distance = 1.0f;
    p->damping = 1e-9; p->eps_rot = 1e-7; p->eps_trans = 1e-7;
}

SLS_HD float sls_icp_gate2(float max_distance) { return max_distance * max_distance; }

SLS_HD void sls_icp_transform(const double *T, const float *p, float *out)
{
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    out[0] = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    out[1] = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    out[2] = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
}

/* one row of the linearisation: six scalars, so that after inlining the 29 sums live in registers */
SLS_HD void sls_icp_row(double j0, double j1, double j2, double j3, double j4, double j5, double r, double *acc)
{
    acc[0] += j0 * j0; acc[1] += j0 * j1; acc[2] += j0 * j2; acc[3] += j0 * j3; acc[4] += j0 * j4; acc[5] += j0 * j5;
    acc[6] += j1 * j1; acc[7] += j1 * j2; acc[8] += j1 * j3; acc[9] += j1 * j4; acc[10] += j1 * j5;
    acc[11] += j2 * j2; acc[12] += j2 * j3; acc[13] += j2 * j4; acc[14] += j2 * j5;
    acc[15] += j3 * j3; acc[16] += j3 * j4; acc[17] += j3 * j5;
    acc[18] += j4 * j4; acc[19] += j4 * j5;
    acc[20] += j5 * j5;
    acc[21] += j0 * r; acc[22] += j1 * r; acc[23] += j2 * r; acc[24] += j3 * r; acc[25] += j4 * r; acc[26] += j5 * r;
    acc[27] += r * r;
}

/* acc[29] of ONE source point: pt = p' (transformed, float32), q its nearest target, n that target's normal (plane method
 * only; may be null for SLS_ICP_POINT), inlier as the gate decided.  Always writes all 29. */
SLS_HD void sls_icp_terms(int method, int inlier, const float *pt, const float *q, const float *n, double *acc)
{
    for (int k = 0; k < SLS_ICP_TERMS; ++k) acc[k] = 0.0;
    if (!inlier) return;
    const double px = (double)pt[0], py = (double)pt[1], pz = (double)pt[2];
    const double dx = px - (double)q[0], dy = py - (double)q[1], dz = pz - (double)q[2];
    if (method == SLS_ICP_PLANE) {
        const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
        const double r = (nx * dx + ny * dy) + nz * dz;
        sls_icp_row(nx, ny, nz, py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, r, acc);
    } else {
        sls_icp_row(1.0, 0.0, 0.0, 0.0, pz, -py, dx, acc);
        sls_icp_row(0.0, 1.0, 0.0, -pz, 0.0, px, dy, acc);
        sls_icp_row(0.0, 0.0, 1.0, py, -px, 0.0, dz, acc);
    }
    acc[28] += 1.0;
}

/* The solve on the 29 sums: T is updated in place, or kept.  Returns the flags of this step (0: an update that did not
 * converge; SLS_ICP_FLAG_CONVERGED: an update that did; SLS_ICP_FLAG_FEW / _NOT_PD: the pose was kept).  xi_out (optional):
 * the six numbers (v, w) of the step, zeros when the pose was kept. */
SLS_HD int sls_icp_solve(const double *S, const SlsIcpParams *prm, double *T, double *xi_out)
{
    double H[6][6], L[6][6], yv[6], xi[6];
    int t = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) { H[a][c] = S[t]; H[c][a] = S[t]; ++t; }
    if (xi_out) for (int a = 0; a < 6; ++a) xi_out[a] = 0.0;
    if (S[28] < (double)prm->min_inliers) return SLS_ICP_FLAG_FEW;
    for (int a = 0; a < 6; ++a) H[a][a] = H[a][a] + prm->damping;
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c <= a; ++c) {
            double s = H[a][c];
            for (int k = 0; k < c; ++k) s = s - L[a][k] * L[c][k];
            if (a == c) {
                if (!(s > 0.0)) return SLS_ICP_FLAG_NOT_PD;
                L[a][a] = sqrt(s);
            } else {
                L[a][c] = s / L[c][c];
            }
        }
    for (int a = 0; a < 6; ++a) {
        double s = -S[21 + a];
        for (int k = 0; k < a; ++k) s = s - L[a][k] * yv[k];
        yv[a] = s / L[a][a];
    }
    for (int a = 5; a >= 0; --a) {
        double s = yv[a];
        for (int k = a + 1; k < 6; ++k) s = s - L[k][a] * xi[k];
        xi[a] = s / L[a][a];
    }
    for (int a = 0; a < 6; ++a)
        if (!(xi[a] == xi[a]) || xi[a] - xi[a] != 0.0) return SLS_ICP_FLAG_NOT_PD;     /* NaN or inf: keep the pose */
    const double ax = 0.5 * xi[3], ay = 0.5 * xi[4], az = 0.5 * xi[5];
    const double s = (ax * ax + ay * ay) + az * az, den = 1.0 + s, c = 1.0 - s;
    double dR[9];
    dR[0] = (c + 2.0 * (ax * ax)) / den; dR[1] = 2.0 * (ax * ay - az) / den; dR[2] = 2.0 * (ax * az + ay) / den;
    dR[3] = 2.0 * (ax * ay + az) / den; dR[4] = (c + 2.0 * (ay * ay)) / den; dR[5] = 2.0 * (ay * az - ax) / den;
    dR[6] = 2.0 * (ax * az - ay) / den; dR[7] = 2.0 * (ay * az + ax) / den; dR[8] = (c + 2.0 * (az * az)) / den;
    double N[12];
    for (int a = 0; a < 3; ++a) {
        for (int j = 0; j < 3; ++j) N[4 * a + j] = (dR[3 * a] * T[j] + dR[3 * a + 1] * T[4 + j]) + dR[3 * a + 2] * T[8 + j];
        N[4 * a + 3] = ((dR[3 * a] * T[3] + dR[3 * a + 1] * T[7]) + dR[3 * a + 2] * T[11]) + xi[a];
    }
    for (int k = 0; k < 12; ++k) T[k] = N[k];
    if (xi_out) for (int a = 0; a < 6; ++a) xi_out[a] = xi[a];
    const double nw = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
    const double nv = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
    return (nw < prm->eps_rot && nv < prm->eps_trans) ? SLS_ICP_FLAG_CONVERGED : 0;
}

#endif /* SLS_ICP_MATH_H */
