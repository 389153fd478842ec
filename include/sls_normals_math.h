/*
 * sls_normals_math.h — the arithmetic of the PCA normal estimate of a point cloud (sls_cloud_normals), shared by the HIP
 * kernel, by a host program and by the NumPy restatement (tests/normals_ref.py), which reproduce the kernel's results bit
 * for bit.
 *
 * THE RULE that makes this possible: the eigen-solve uses + - * / and sqrt alone — no libm call such as acos or cos, whose
 * device and host versions differ — and every sum runs in one fixed order.  Built with -ffp-contract=off (no implicit fma)
 * the device result then equals this header compiled for the host, bit for bit.  A trigonometric closed form for the 3 x 3
 * eigenvalues cannot meet that, which is why the solver is a Jacobi iteration.
 *
 * Inputs: M points (float32), k = max_nn in [1, SLS_NORMALS_NN_MAX], a radius (float32, finite and > 0, or +inf for a pure
 * k-NN neighbourhood) and a viewpoint (three float32).  This restates Open3D's
 * estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) followed by orient_normals_towards_camera_location(viewpoint)
 * from their documented behaviour; Open3D is not a dependency and the device code is pinned against the NumPy restatement,
 * not against Open3D itself.
 *
 * Neighbourhood of point i: the entries of i's k-list in the cloud's self-query (include/sls_outlier_math.h: ascending by
 * (d2, index), SLS_NN_KEY_NONE beyond M) that are real and have d2 <= r2, r2 = radius * radius (ONE float32 product).  The
 * point itself, d2 = 0, is one of its neighbours, as in Open3D.  The list ascends, so the neighbourhood is a prefix of it;
 * n_i is its length (1 <= n_i <= min(k, M)).  Whether Open3D's hybrid search puts its boundary at < or <= was not verified.
 *
 * n_i < 3 — the fallback: the normal is unit(viewpoint - p), computed in float64 and rounded to float32; (0, 0, 1) if that
 * vector is zero.  This is deliberate: Open3D leaves (0, 0, 1) there before it orients, this project gives an isolated
 * return the reference's own default instead, -unit(point) for a viewpoint at the origin.  The eigenvalues are zeros.
 *
 * n_i >= 3:
 *   mean  = (sum in list order of (double)coordinate) / n_i, per axis;
 *   C     = six sums in list order of the products of d = (double)p_j - mean (xx, xy, xz, yy, yz, zz), each / n_i;
 *   C is diagonalised by cyclic Jacobi rotations, pairs (0,1), (0,2), (1,2) in this order, SLS_NORMALS_SWEEPS sweeps, a
 *   pair whose off-diagonal element is exactly 0 skipped, Rutishauser's formulas:
 *       theta = 0.5 * (a_qq - a_pp) / a_pq,  t = sgn(theta) / (|theta| + sqrt(theta^2 + 1))  (sgn(0) = +1),
 *       c = 1 / sqrt(t^2 + 1),  s = t c,  tau = s / (1 + c),  h = t a_pq,
 *       a_pp -= h,  a_qq += h,  a_pq = 0,  a_rp' = a_rp - s (a_rq + a_rp tau),  a_rq' = a_rq + s (a_rp - a_rq tau),
 *       and the same pair of updates on the columns p, q of V (V starts as the identity).
 *     (An overflowing theta^2 gives t = 0, the identity rotation, and still clears a_pq: no special case is needed.)
 *   the normal is the column of V under the smallest diagonal entry, ties to the lowest index; normalised in float64;
 *   flipped if its float64 dot product with (viewpoint - p), summed x, y, z, is negative; rounded to float32.
 *   The eigenvalues are the diagonal, ascending, rounded to float32 (a value just below 0 is not clamped).
 *
 * SLS_NORMALS_SWEEPS = 6.  Cyclic Jacobi converges quadratically once the off-diagonal norm is below the smallest gap
 * between eigenvalues, and no slower at a multiple eigenvalue: off -> O(off^2 / gap) per sweep, so from a relative 1e-2 the
 * sequence 1e-4, 1e-8, 1e-16 ends below eps64 three sweeps later, and a 3 x 3 matrix needs one or two sweeps to get there.
 * Measured on the restatement: over 200 000 random positive semi-definite matrices with condition numbers up to 1e12,
 * a tenth of them with three eigenvalues equal to 1e-3 relative, and the covariances of a 3000-point scan, no bit of d or
 * V changed after the FOURTH sweep.  Six leaves two to spare; a sweep on a converged matrix skips its pairs or applies
 * identity rotations (t underflows against 1), so spare sweeps change nothing.  tests/test_normals_math.py repeats the
 * measurement on a smaller set (six sweeps against eight, bit for bit) and checks the outcome against LAPACK.
 *
 * Rules for users of this header: no fast-math, -ffp-contract=off (unlike sls_nn_math.h this header DOES hold contractible
 * expressions), HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt.  Coordinates must be finite.  Plain C99 / HIP device
 * compatible.
 */
#ifndef SLS_NORMALS_MATH_H
#define SLS_NORMALS_MATH_H

#include "sls_nn_math.h"

#ifndef SLS_NORMALS_NN_MAX
#define SLS_NORMALS_NN_MAX 64   /* (include/sls_abi.h defines the same) */
#endif
#define SLS_NORMALS_SWEEPS 6

/* n_i: the length of the prefix of the k-list (d2 and index rows as sls_nn_query_k writes them: +inf and -1 beyond M)
 * that lies within the radius. */
SLS_HD int sls_normals_count(const float *d2, const int32_t *index, int k, float radius)
{
    const float r2 = radius * radius;
    int n = 0;
    for (int j = 0; j < k; ++j) {
        if (index[j] < 0 || !(d2[j] <= r2)) break;
        ++n;
    }
    return n;
}

/* unit(viewpoint - p) in float64, rounded; (0, 0, 1) for a zero vector */
SLS_HD void sls_normals_fallback(const float *p, const float *viewpoint, float *normal)
{
    const double vx = (double)viewpoint[0] - (double)p[0], vy = (double)viewpoint[1] - (double)p[1],
                 vz = (double)viewpoint[2] - (double)p[2];
    const double len2 = vx * vx + vy * vy + vz * vz;
    if (len2 == 0.0) { normal[0] = 0.0f; normal[1] = 0.0f; normal[2] = 1.0f; return; }
    const double len = sqrt(len2);
    normal[0] = (float)(vx / len); normal[1] = (float)(vy / len); normal[2] = (float)(vz / len);
}

/* cov[6] = xx, xy, xz, yy, yz, zz of the n points xyz[3 * index[j]], j in list order (n >= 1) */
SLS_HD void sls_normals_covariance(const float *xyz, const int32_t *index, int n, double *cov)
{
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < n; ++j) {
        const float *q = xyz + 3 * (size_t)index[j];
        sx += (double)q[0]; sy += (double)q[1]; sz += (double)q[2];
    }
    const double dn = (double)n, mx = sx / dn, my = sy / dn, mz = sz / dn;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (int j = 0; j < n; ++j) {
        const float *q = xyz + 3 * (size_t)index[j];
        const double dx = (double)q[0] - mx, dy = (double)q[1] - my, dz = (double)q[2] - mz;
        xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    cov[0] = xx / dn; cov[1] = xy / dn; cov[2] = xz / dn; cov[3] = yy / dn; cov[4] = yz / dn; cov[5] = zz / dn;
}

/* One rotation in the plane (p, q); r is the third index.  Every argument is one scalar, so that after inlining with
 * constant indices the matrix and V live in registers. */
SLS_HD void sls_normals_rotate(double *app, double *aqq, double *apq, double *arp, double *arq, double *v0p, double *v0q,
                               double *v1p, double *v1q, double *v2p, double *v2q)
{
    const double a = *apq;
    if (a == 0.0) return;
    const double theta = 0.5 * (*aqq - *app) / a;
    const double abs_theta = theta < 0.0 ? -theta : theta;
    const double den = abs_theta + sqrt(theta * theta + 1.0);
    const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c), h = t * a;
    double g, f;
    *app = *app - h; *aqq = *aqq + h; *apq = 0.0;
    g = *arp; f = *arq; *arp = g - s * (f + g * tau); *arq = f + s * (g - f * tau);
    g = *v0p; f = *v0q; *v0p = g - s * (f + g * tau); *v0q = f + s * (g - f * tau);
    g = *v1p; f = *v1q; *v1p = g - s * (f + g * tau); *v1q = f + s * (g - f * tau);
    g = *v2p; f = *v2q; *v2p = g - s * (f + g * tau); *v2q = f + s * (g - f * tau);
}

/* cov[6] -> d[3] (the diagonal, in place order) and v[9] (row-major; column j belongs to d[j]) */
SLS_HD void sls_normals_jacobi(const double *cov, double *d, double *v)
{
    double a00 = cov[0], a01 = cov[1], a02 = cov[2], a11 = cov[3], a12 = cov[4], a22 = cov[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < SLS_NORMALS_SWEEPS; ++sweep) {
        sls_normals_rotate(&a00, &a11, &a01, &a02, &a12, &v00, &v01, &v10, &v11, &v20, &v21);      /* (0,1), r = 2 */
        sls_normals_rotate(&a00, &a22, &a02, &a01, &a12, &v00, &v02, &v10, &v12, &v20, &v22);      /* (0,2), r = 1 */
        sls_normals_rotate(&a11, &a22, &a12, &a01, &a02, &v01, &v02, &v11, &v12, &v21, &v22);      /* (1,2), r = 0 */
    }
    d[0] = a00; d[1] = a11; d[2] = a22;
    v[0] = v00; v[1] = v01; v[2] = v02; v[3] = v10; v[4] = v11; v[5] = v12; v[6] = v20; v[7] = v21; v[8] = v22;
}

/* the oriented unit normal (float32) and the ascending eigenvalues (float32) from d, v of sls_normals_jacobi */
SLS_HD void sls_normals_select(const double *d, const double *v, const float *p, const float *viewpoint, float *normal,
                               float *eigenvalues)
{
    /* (every element is read before one is chosen: a choice between scalars, not between addresses) */
    const double d0 = d[0], d1 = d[1], d2 = d[2];
    const double v00 = v[0], v01 = v[1], v02 = v[2], v10 = v[3], v11 = v[4], v12 = v[5], v20 = v[6], v21 = v[7], v22 = v[8];
    double dm = d0, nx = v00, ny = v10, nz = v20;
    if (d1 < dm) { dm = d1; nx = v01; ny = v11; nz = v21; }
    if (d2 < dm) { dm = d2; nx = v02; ny = v12; nz = v22; }
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    nx = nx / len; ny = ny / len; nz = nz / len;
    const double vx = (double)viewpoint[0] - (double)p[0], vy = (double)viewpoint[1] - (double)p[1],
                 vz = (double)viewpoint[2] - (double)p[2];
    if (nx * vx + ny * vy + nz * vz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    normal[0] = (float)nx; normal[1] = (float)ny; normal[2] = (float)nz;
    double e0 = d0, e1 = d1, e2 = d2, sw;
    if (e1 < e0) { sw = e0; e0 = e1; e1 = sw; }
    if (e2 < e1) { sw = e1; e1 = e2; e2 = sw; }
    if (e1 < e0) { sw = e0; e0 = e1; e1 = sw; }
    eigenvalues[0] = (float)e0; eigenvalues[1] = (float)e1; eigenvalues[2] = (float)e2;
}

/* Point i whole: its list rows (k entries each), the cloud, the parameters -> normal[3], eigenvalues[3]; returns n_i. */
SLS_HD int sls_normals_point(const float *xyz, int i, const float *d2, const int32_t *index, int k, float radius,
                             const float *viewpoint, float *normal, float *eigenvalues)
{
    const int n = sls_normals_count(d2, index, k, radius);
    const float *p = xyz + 3 * (size_t)i;
    if (n < 3) {
        sls_normals_fallback(p, viewpoint, normal);
        eigenvalues[0] = 0.0f; eigenvalues[1] = 0.0f; eigenvalues[2] = 0.0f;
        return n;
    }
    double cov[6], d[3], v[9];
    sls_normals_covariance(xyz, index, n, cov);
    sls_normals_jacobi(cov, d, v);
    sls_normals_select(d, v, p, viewpoint, normal, eigenvalues);
    return n;
}

#endif /* SLS_NORMALS_MATH_H */
