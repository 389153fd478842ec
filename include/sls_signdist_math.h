/*
 * sls_signdist_math.h — the arithmetic of the SIGNED point-to-mesh distance (sls_mesh_pseudonormals,
 * sls_mesh_signed_distance, sls_signed_stats, sls_signed_error_colors), shared by the HIP kernels
 * (csrc/sls_signdist.hip, csrc/sls_metrics.hip) and by any CPU checker that wants to reproduce their results bit for bit
 * (tests/signdist_ref.py compiles this header for the host).
 *
 * The magnitude is the distance of include/sls_meshdist_math.h, untouched.  The SIGN is that of
 * (q - closest) . n with n the angle-weighted pseudo-normal of the FEATURE of the nearest face the closest point lies on —
 * the face, one of its edges or one of its vertices (Baerentzen and Aanaes, IEEE TVCG 2005).  The face normal alone gives
 * the wrong sign wherever the closest point lies on an edge or vertex with a sharp dihedral angle; the pseudo-normal is
 * right for every closed, consistently oriented mesh, and locally for an open oriented one.
 *
 * ---- the feature of the closest point ----------------------------------------------------------------------------------
 * sls_sd_triangle repeats the steps of sls_meshdist_triangle exactly — the same candidates in the same order under the
 * same strict <, so the same d2 bits — and returns rel[3], the closest point in the QUERY's frame (that header's `best`
 * before `+ q`), and which candidate won:
 *   0        the interior candidate;
 *   1, 2, 3  edge AB, BC, CA, the clamped t strictly inside (0, 1);
 *   4, 5, 6  vertex a, b, c: segment AB gives a at t == 0 and b at t == 1, BC gives b and c, CA gives c and a; a
 *            zero-length edge has t = 0 and is its start vertex.
 *
 * ---- the three tables (float64, stored as float32 rows: each component rounded once) -----------------------------------
 * Unit face normal: (b - a) x (c - a) of the float32 vertices, in float64, divided by its length.  A face whose length is 0
 * or not finite — and every face that is degenerate by sls_mesh_degenerate or has a non-finite vertex — has the ZERO
 * normal and contributes nothing anywhere.
 * Edge pseudo-normal: the corners (f, k) of the faces that are not degenerate by sls_mesh_degenerate and share the
 * undirected edge {f[k], f[(k + 1) % 3]} form a group; the edge normal is the sum, starting from +0, of the unit normals
 * of their faces in ascending corner id 3 f + k, not normalised, the same bits at every corner of the group: a boundary
 * edge has its one face's normal, an edge with three owners the sum of three, a repeated triangle counts twice.  The
 * corners of a degenerate face hold zeros.
 * Corner angle: with u, w the float64 unit directions of the two edges leaving the corner (sls_sd_unit),
 * theta = 2 atan(|u - w| / |u + w|); where the numerator exceeds the denominator the ratio is inverted and theta is
 * pi - 2 atan(|u + w| / |u - w|); theta = pi where |u + w| = 0.  This is Kahan's form: well conditioned near 0 and near
 * pi, where atan2(|u x w|, u . w) from cancelling sums is not.  The corners of a face with the zero normal have theta = 0.
 * Arctangent (sls_sd_atan, x >= 0): libm's atan differs between device and host (include/sls_ground_math.h records the
 * same of atan2), so it is this header's own, from + - * / sqrt alone: the reciprocal for x > 1 (atan x = pi/2 - atan 1/x);
 * two halvings x <- x / (1 + sqrt(1 + x x)) (atan x = 2 atan of that), which bring x to at most tan(pi / 16) = 0.199;
 * the Taylor polynomial of 12 terms x (1 - x^2 / 3 + ... - x^22 / 23) by Horner from the highest coefficient down;
 * times 4.  The truncation term is below 0.199^25 / 25 = 1.2e-19.
 * Vertex pseudo-normal: the sum, starting from +0, over the corners at v in ascending corner id of theta times the unit
 * face normal (three products, three additions per corner), not normalised; zeros for a vertex no live face references.
 *
 * ---- the sign ----------------------------------------------------------------------------------------------------------
 * With n the STORED float32 row for the feature — the face's row, the corner's edge row (corner 3 f + feature - 1), or the
 * row of vertex faces[3 f + feature - 4]:  s = -((rel[0] n[0] + rel[1] n[1]) + rel[2] n[2]) in float64; every product of
 * two float32 is exact there.  The signed distance is -sqrtf(d2) iff s < 0, else +sqrtf(d2): a point on the surface, or one
 * whose row is zero, gets the non-negative value, and +0.0f has its sign bit clear.
 *
 * ---- statistics and colours ----------------------------------------------------------------------------------------------
 * An entry takes part in sls_signed_stats iff |sd| < truncation (a NaN does not).  Colour: L = 255 for |sd| >= truncation,
 * else (int)(|sd| / truncation * 256) in float32; sd >= 0: (255, 255 - L, 255 - L), white to red, in front of the faces;
 * sd < 0: (255 - L, 255 - L, 255), white to blue, behind them; NaN: (0, 0, 0).
 *
 * Rules for users of this header, as for sls_meshdist_math.h: every float32 product feeds an explicit fmaf or stands
 * alone, every function sets FP_CONTRACT OFF for its body; no libm beyond sqrt / sqrtf / fmaf; no fast-math; HIP: keep
 * -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_SIGNDIST_MATH_H
#define SLS_SIGNDIST_MATH_H

#include "sls_meshdist_math.h"
#include "sls_mesh_math.h"

#define SLS_SD_PI 3.14159265358979323846
#define SLS_SD_HALF_PI 1.57079632679489661923

/* sls_md_segment, with the clamped parameter returned as well */
SLS_HD float sls_sd_segment(float px, float py, float pz, float ex, float ey, float ez, float *p, float *t_out)
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
    *t_out = t;
    return sls_md_dot(p[0], p[1], p[2], p[0], p[1], p[2]);
}

/* the feature of segment number seg (0: AB, 1: BC, 2: CA) at the clamped parameter t */
SLS_HD int sls_sd_segment_feature(int seg, float t)
{
    if (t == 0.0f) return 4 + seg;
    if (t == 1.0f) return seg == 2 ? 4 : 5 + seg;
    return 1 + seg;
}

/* Squared distance of q to the triangle (a, b, c): the bits of sls_meshdist_triangle; rel[3] the closest point in the
 * query frame, *feature which part of the triangle it lies on (see above). */
SLS_HD float sls_sd_triangle(const float q[3], const float a[3], const float b[3], const float c[3], float rel[3], int *feature)
{
#pragma STDC FP_CONTRACT OFF
    const float Ax = a[0] - q[0], Ay = a[1] - q[1], Az = a[2] - q[2];
    const float Bx = b[0] - q[0], By = b[1] - q[1], Bz = b[2] - q[2];
    const float Cx = c[0] - q[0], Cy = c[1] - q[1], Cz = c[2] - q[2];
    const float abx = Bx - Ax, aby = By - Ay, abz = Bz - Az;
    const float bcx = Cx - Bx, bcy = Cy - By, bcz = Cz - Bz;
    const float cax = Ax - Cx, cay = Ay - Cy, caz = Az - Cz;
    float best[3], p[3], t;
    float d2 = sls_sd_segment(Ax, Ay, Az, abx, aby, abz, best, &t), e2;
    int feat = sls_sd_segment_feature(0, t);
    e2 = sls_sd_segment(Bx, By, Bz, bcx, bcy, bcz, p, &t);
    if (e2 < d2) { d2 = e2; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; feat = sls_sd_segment_feature(1, t); }
    e2 = sls_sd_segment(Cx, Cy, Cz, cax, cay, caz, p, &t);
    if (e2 < d2) { d2 = e2; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; feat = sls_sd_segment_feature(2, t); }
    {
        const float nx = sls_md_det(cay, abz, caz, aby), ny = sls_md_det(caz, abx, cax, abz), nz = sls_md_det(cax, aby, cay, abx);
        const float va = sls_md_dot(nx, ny, nz, sls_md_det(By, bcz, Bz, bcy), sls_md_det(Bz, bcx, Bx, bcz), sls_md_det(Bx, bcy, By, bcx));
        const float vb = sls_md_dot(nx, ny, nz, sls_md_det(Cy, caz, Cz, cay), sls_md_det(Cz, cax, Cx, caz), sls_md_det(Cx, cay, Cy, cax));
        const float vc = sls_md_dot(nx, ny, nz, sls_md_det(Ay, abz, Az, aby), sls_md_det(Az, abx, Ax, abz), sls_md_det(Ax, aby, Ay, abx));
        if (va > 0.0f && vb > 0.0f && vc > 0.0f) {
            const float s = (va + vb) + vc;
            const float wa = va / s, wb = vb / s, wc = vc / s;
            const float lab = sls_md_dot(abx, aby, abz, abx, aby, abz), lbc = sls_md_dot(bcx, bcy, bcz, bcx, bcy, bcz);
            const float lca = sls_md_dot(cax, cay, caz, cax, cay, caz);
            float ex = cax, ey = cay, ez = caz, ee = lca, lo = -wa, hi = wc;
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
            if (e2 < d2) { d2 = e2; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; feat = 0; }
        }
    }
    rel[0] = best[0]; rel[1] = best[1]; rel[2] = best[2];
    *feature = feat;
    return d2;
}

/* 1 when the three coordinates are finite */
SLS_HD int sls_sd_finite3(const float p[3])
{
    return fabsf(p[0]) <= 3.402823466e+38f && fabsf(p[1]) <= 3.402823466e+38f && fabsf(p[2]) <= 3.402823466e+38f;
}

/* v / |v| in float64; returns 0 (and zeros) where the length is 0 or not finite */
SLS_HD int sls_sd_unit(double x, double y, double z, double u[3])
{
#pragma STDC FP_CONTRACT OFF
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0 && len <= 1.7976931348623157e308)) { u[0] = 0.0; u[1] = 0.0; u[2] = 0.0; return 0; }
    u[0] = x / len; u[1] = y / len; u[2] = z / len;
    return 1;
}

/* the unit normal of the face (a, b, c); returns 0 (and zeros) for a face without one */
SLS_HD int sls_sd_face_normal(const float a[3], const float b[3], const float c[3], double n[3])
{
#pragma STDC FP_CONTRACT OFF
    const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
    const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
    const double uyvz = uy * vz, uzvy = uz * vy, uzvx = uz * vx, uxvz = ux * vz, uxvy = ux * vy, uyvx = uy * vx;
    return sls_sd_unit(uyvz - uzvy, uzvx - uxvz, uxvy - uyvx, n);
}

/* atan(x) for x >= 0 (see above); a NaN stays one */
SLS_HD double sls_sd_atan(double x)
{
#pragma STDC FP_CONTRACT OFF
    const int inv = x > 1.0;
    double x2, p, r;
    if (inv) x = 1.0 / x;
    x2 = x * x; x = x / (1.0 + sqrt(1.0 + x2));
    x2 = x * x; x = x / (1.0 + sqrt(1.0 + x2));
    x2 = x * x;
    p = 1.0 / 23.0;
    p = x2 * p; p = 1.0 / 21.0 - p;
    p = x2 * p; p = 1.0 / 19.0 - p;
    p = x2 * p; p = 1.0 / 17.0 - p;
    p = x2 * p; p = 1.0 / 15.0 - p;
    p = x2 * p; p = 1.0 / 13.0 - p;
    p = x2 * p; p = 1.0 / 11.0 - p;
    p = x2 * p; p = 1.0 / 9.0 - p;
    p = x2 * p; p = 1.0 / 7.0 - p;
    p = x2 * p; p = 1.0 / 5.0 - p;
    p = x2 * p; p = 1.0 / 3.0 - p;
    p = x2 * p; p = 1.0 - p;
    r = x * p;
    r = 4.0 * r;
    return inv ? SLS_SD_HALF_PI - r : r;
}

/* the angle between the float64 directions u and w (any length); 0 where either has no direction */
SLS_HD double sls_sd_angle(const double u_in[3], const double w_in[3])
{
#pragma STDC FP_CONTRACT OFF
    double u[3], w[3], d[3], s[3], num, den, dd, ss;
    if (!sls_sd_unit(u_in[0], u_in[1], u_in[2], u) || !sls_sd_unit(w_in[0], w_in[1], w_in[2], w)) return 0.0;
    d[0] = u[0] - w[0]; d[1] = u[1] - w[1]; d[2] = u[2] - w[2];
    s[0] = u[0] + w[0]; s[1] = u[1] + w[1]; s[2] = u[2] + w[2];
    dd = d[0] * d[0]; dd = dd + d[1] * d[1]; dd = dd + d[2] * d[2];
    ss = s[0] * s[0]; ss = ss + s[1] * s[1]; ss = ss + s[2] * s[2];
    num = sqrt(dd); den = sqrt(ss);
    if (den == 0.0) return SLS_SD_PI;
    if (num > den) {
        const double r = sls_sd_atan(den / num), r2 = 2.0 * r;
        return SLS_SD_PI - r2;
    }
    return 2.0 * sls_sd_atan(num / den);
}

/* the angle of the face (a, b, c) at its corner k = 0, 1, 2 (between the edges to the next and to the previous vertex) */
SLS_HD double sls_sd_corner_angle(const float a[3], const float b[3], const float c[3], int k)
{
#pragma STDC FP_CONTRACT OFF
    const float *p0 = k == 0 ? a : k == 1 ? b : c, *p1 = k == 0 ? b : k == 1 ? c : a, *p2 = k == 0 ? c : k == 1 ? a : b;
    double u[3], w[3];
    u[0] = (double)p1[0] - (double)p0[0]; u[1] = (double)p1[1] - (double)p0[1]; u[2] = (double)p1[2] - (double)p0[2];
    w[0] = (double)p2[0] - (double)p0[0]; w[1] = (double)p2[1] - (double)p0[1]; w[2] = (double)p2[2] - (double)p0[2];
    return sls_sd_angle(u, w);
}

/* One face whole: the class for the status words — 0 live, 1 two equal indices, 2 an index outside [0, V), 3 a non-finite
 * vertex, 4 zero area — its unit normal n[3] (zeros unless live) and its three corner angles (zeros unless live). */
SLS_HD int sls_sd_face(const float *vertices, const int32_t f[3], int32_t V, double n[3], double theta[3])
{
    const int d = sls_mesh_degenerate(f, V);
    n[0] = 0.0; n[1] = 0.0; n[2] = 0.0;
    theta[0] = 0.0; theta[1] = 0.0; theta[2] = 0.0;
    if (d) return d;
    {
        const float *a = vertices + 3 * (size_t)f[0], *b = vertices + 3 * (size_t)f[1], *c = vertices + 3 * (size_t)f[2];
        const float pa[3] = { a[0], a[1], a[2] }, pb[3] = { b[0], b[1], b[2] }, pc[3] = { c[0], c[1], c[2] };
        if (!(sls_sd_finite3(pa) && sls_sd_finite3(pb) && sls_sd_finite3(pc))) return 3;
        if (!sls_sd_face_normal(pa, pb, pc, n)) return 4;
        theta[0] = sls_sd_corner_angle(pa, pb, pc, 0);
        theta[1] = sls_sd_corner_angle(pa, pb, pc, 1);
        theta[2] = sls_sd_corner_angle(pa, pb, pc, 2);
    }
    return 0;
}

/* sum += theta * n, component by component (the vertex sum's step); theta = 1: the edge sum's step is sum += n */
SLS_HD void sls_sd_accumulate(double sum[3], double theta, const double n[3])
{
#pragma STDC FP_CONTRACT OFF
    const double x = theta * n[0], y = theta * n[1], z = theta * n[2];
    sum[0] = sum[0] + x; sum[1] = sum[1] + y; sum[2] = sum[2] + z;
}

/* the signed distance from d2, rel and the stored row of the feature */
SLS_HD float sls_sd_signed(float d2, const float rel[3], const float n[3])
{
#pragma STDC FP_CONTRACT OFF
    const double x = (double)rel[0] * (double)n[0], y = (double)rel[1] * (double)n[1], z = (double)rel[2] * (double)n[2];
    const double s = -((x + y) + z);
    const float d = sqrtf(d2);
    return s < 0.0 ? -d : d;
}

/* 1 when the entry takes part in sls_signed_stats */
SLS_HD int sls_sd_stats_term(float sd, float truncation)
{
    return fabsf(sd) < truncation;
}

/* the diverging colour of a signed distance: rgb[3] */
SLS_HD void sls_signed_error_color(float sd, float truncation, uint8_t *rgb)
{
#pragma STDC FP_CONTRACT OFF
    const float m = fabsf(sd), t = m / truncation;
    int L;
    if (!(sd == sd)) { rgb[0] = 0; rgb[1] = 0; rgb[2] = 0; return; }
    L = m >= truncation ? 255 : (int)(t * 256.0f);
    if (L > 255) L = 255;
    if (sd < 0.0f) { rgb[0] = (uint8_t)(255 - L); rgb[1] = (uint8_t)(255 - L); rgb[2] = 255; }
    else { rgb[0] = 255; rgb[1] = (uint8_t)(255 - L); rgb[2] = (uint8_t)(255 - L); }
}

#endif /* SLS_SIGNDIST_MATH_H */
