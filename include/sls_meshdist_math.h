/*
 * sls_meshdist_math.h — the arithmetic of the exact point-to-mesh distance (sls_mesh_distance) and of the error colours
 * (sls_error_colors), shared by the HIP kernels and by any CPU checker that wants to reproduce their results bit for bit.
 *
 * Distance of a query q to a triangle (a, b, c), all float32, worked in the QUERY's frame: the first step is
 * A = a - q, B = b - q, C = c - q (one rounding each), so every later quantity scales with the local geometry and not
 * with the map's coordinates; the wanted number is the distance of the origin to (A, B, C).
 *
 * It is NOT the textbook seven-region classification: in float32 the cancelling cross-product terms of that test send
 * about 1 case in 100 000 to the wrong region, with an error of up to 0.79 of the scale on slivers, which marching
 * tetrahedra emits wherever the surface passes near a cube corner.  Here the squared distance is the MINIMUM over
 * candidate points that all lie ON the triangle:
 *
 *   1-3. the closest points of the three edge segments AB, BC, CA: t = -(P . e) / (e . e) clamped to [0, 1], t = 0 for
 *        a zero-length edge, point = fmaf(t, e, P) per axis;
 *   4.   the point of normalised barycentric weights va/s, vb/s, vc/s, s = va + vb + vc, used only where all three of
 *        va, vb, vc are > 0.  With n = (B - A) x (C - A): va = n . (B x (C - B)), vb = n . (C x (A - C)),
 *        vc = n . (A x (B - A)) — each cross product has an EDGE as one factor, so its rounding error scales with
 *        scale * size and not with scale^2.
 *
 * A wrong interior decision then costs at most the sliver's height, a zero-area face degenerates to its segments or its
 * point by itself (n = 0: no weight is > 0) and nothing divides by zero.  Where all three weights are > 0 each of va/s,
 * vb/s, vc/s lies in (0, 1], so candidate 4 is a convex combination up to rounding.  Among candidates of equal d2 the
 * first in the order above supplies the closest point.  Measured against float64: DESIGN.md section 7.
 *
 * d2 >= +0, so (d2, face) packs as sls_nn_key(d2, face) (sls_nn_math.h): the lowest face index wins among equal d2 BITS.
 *
 * Error colour of a squared distance: t = sqrtf(d2) / truncation in float32 (both correctly rounded),
 * L = t >= 1 ? 255 : (int)(t * 256.0f); L <= 127 gives (2 L, 255, 0), otherwise (255, 2 (255 - L), 0): green is good,
 * yellow is at half the truncation, red at or beyond it.  A NaN (or negative) d2 gives (0, 0, 255).
 *
 * Rules for users of this header: every product feeds an explicit fmaf or stands alone as an fmaf addend, and every
 * function sets FP_CONTRACT OFF for its body (see below), so the contraction setting does not matter; no fast-math;
 * HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_MESHDIST_MATH_H
#define SLS_MESHDIST_MATH_H

#include <math.h>
#include <stdint.h>

#ifndef SLS_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define SLS_HD __host__ __device__ __forceinline__
#else
#define SLS_HD static inline
#endif
#endif

/* The sums below ADD to fmaf results (va + vb, query frame + q).  A compiler that may contract across statements fuses
 * such a sum into the fmaf chain that feeds it (hipcc's default for device code does), so every function here switches
 * contraction off for its own body: with that the header gives the same bits under any -ffp-contract setting. */
SLS_HD float sls_md_dot(float ax, float ay, float az, float bx, float by, float bz)
{
#pragma STDC FP_CONTRACT OFF
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

/* One component of a cross product: u0 * v1 - u1 * v0, the second product rounded on its own. */
SLS_HD float sls_md_det(float u0, float v1, float u1, float v0)
{
#pragma STDC FP_CONTRACT OFF
    return fmaf(u0, v1, -(u1 * v0));
}

/* Candidate on the segment P + t e, t in [0, 1]: the point p[3] and its squared distance to the origin. */
SLS_HD float sls_md_segment(float px, float py, float pz, float ex, float ey, float ez, float *p)
{
#pragma STDC FP_CONTRACT OFF
    const float ee = sls_md_dot(ex, ey, ez, ex, ey, ez);
    float t = 0.0f;
    if (ee > 0.0f) {
        t = -sls_md_dot(px, py, pz, ex, ey, ez) / ee;
        t = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;      /* (a NaN gives 0) */
    }
    p[0] = fmaf(t, ex, px);
    p[1] = fmaf(t, ey, py);
    p[2] = fmaf(t, ez, pz);
    return sls_md_dot(p[0], p[1], p[2], p[0], p[1], p[2]);
}

/* Squared distance of q to the triangle (a, b, c); closest (may be null) receives the closest point, query frame + q. */
SLS_HD float sls_meshdist_triangle(float qx, float qy, float qz, float ax, float ay, float az, float bx, float by, float bz,
                                   float cx, float cy, float cz, float *closest)
{
#pragma STDC FP_CONTRACT OFF
    const float Ax = ax - qx, Ay = ay - qy, Az = az - qz;
    const float Bx = bx - qx, By = by - qy, Bz = bz - qz;
    const float Cx = cx - qx, Cy = cy - qy, Cz = cz - qz;
    const float abx = Bx - Ax, aby = By - Ay, abz = Bz - Az;       /* the edges, from the query-frame vertices */
    const float bcx = Cx - Bx, bcy = Cy - By, bcz = Cz - Bz;
    const float cax = Ax - Cx, cay = Ay - Cy, caz = Az - Cz;
    float best[3], p[3];
    float d2 = sls_md_segment(Ax, Ay, Az, abx, aby, abz, best), e2;
    e2 = sls_md_segment(Bx, By, Bz, bcx, bcy, bcz, p);
    if (e2 < d2) { d2 = e2; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; }
    e2 = sls_md_segment(Cx, Cy, Cz, cax, cay, caz, p);
    if (e2 < d2) { d2 = e2; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; }
    {
        /* n = ab x (c - a) = ab x (-ca) */
        const float nx = sls_md_det(cay, abz, caz, aby), ny = sls_md_det(caz, abx, cax, abz), nz = sls_md_det(cax, aby, cay, abx);
        const float va = sls_md_dot(nx, ny, nz, sls_md_det(By, bcz, Bz, bcy), sls_md_det(Bz, bcx, Bx, bcz), sls_md_det(Bx, bcy, By, bcx));
        const float vb = sls_md_dot(nx, ny, nz, sls_md_det(Cy, caz, Cz, cay), sls_md_det(Cz, cax, Cx, caz), sls_md_det(Cx, cay, Cy, cax));
        const float vc = sls_md_dot(nx, ny, nz, sls_md_det(Ay, abz, Az, aby), sls_md_det(Az, abx, Ax, abz), sls_md_det(Ax, aby, Ay, abx));
        if (va > 0.0f && vb > 0.0f && vc > 0.0f) {
            const float s = (va + vb) + vc;
            const float wa = va / s, wb = vb / s, wc = vc / s;
            const float lab = sls_md_dot(abx, aby, abz, abx, aby, abz), lbc = sls_md_dot(bcx, bcy, bcz, bcx, bcy, bcz);
            const float lca = sls_md_dot(cax, cay, caz, cax, cay, caz);
            float ex = cax, ey = cay, ez = caz, ee = lca, lo = -wa, hi = wc, t;
            if (lab >= lbc && lab >= lca) { ex = abx; ey = aby; ez = abz; ee = lab; lo = -wb; hi = wa; }
            else if (lbc >= lca) { ex = bcx; ey = bcy; ez = bcz; ee = lbc; lo = -wc; hi = wb; }
            p[0] = fmaf(wc, Cx, fmaf(wb, Bx, wa * Ax));
            p[1] = fmaf(wc, Cy, fmaf(wb, By, wa * Ay));
            p[2] = fmaf(wc, Cz, fmaf(wb, Bz, wa * Az));
            t = -sls_md_dot(p[0], p[1], p[2], ex, ey, ez) / ee;
            t = t < lo ? lo : (t > hi ? hi : t);
            p[0] = fmaf(t, ex, p[0]);
            p[1] = fmaf(t, ey, p[1]);
            p[2] = fmaf(t, ez, p[2]);
            e2 = sls_md_dot(p[0], p[1], p[2], p[0], p[1], p[2]);
            if (e2 < d2) { d2 = e2; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; }
        }
    }
    if (closest) {
        closest[0] = best[0] + qx;
        closest[1] = best[1] + qy;
        closest[2] = best[2] + qz;
    }
    return d2;
}

/* The error colour of a squared distance: rgb[3]. */
SLS_HD void sls_error_color(float d2, float truncation, uint8_t *rgb)
{
#pragma STDC FP_CONTRACT OFF
    const float t = sqrtf(d2) / truncation;
    int L;
    if (!(t == t)) { rgb[0] = 0; rgb[1] = 0; rgb[2] = 255; return; }
    L = t >= 1.0f ? 255 : (int)(t * 256.0f);
    if (L <= 127) { rgb[0] = (uint8_t)(2 * L); rgb[1] = 255; rgb[2] = 0; }
    else { rgb[0] = 255; rgb[1] = (uint8_t)(2 * (255 - L)); rgb[2] = 0; }
}

#endif /* SLS_MESHDIST_MATH_H */
