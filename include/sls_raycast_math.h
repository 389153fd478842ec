/*
 * sls_raycast_math.h — the arithmetic of the first hit of a ray on a triangle mesh (sls_mesh_raycast), shared by the HIP
 * kernel and by any CPU checker that wants to reproduce its results bit for bit.  Float32, one fixed operation order, no
 * fma anywhere: every function sets FP_CONTRACT OFF for its body, and the objects that use it are built without
 * contraction.
 *
 * RAY.  Origin o, direction d (need not be unit); the point at parameter t is o + t d.  A ray is REFUSED
 * (sls_ray_valid == 0) when a component of o or d is not finite or when the direction counts as zero: its largest
 * |component| is below SLS_RAY_MIN_DIR = 2^-100.  (A direction that small has no float32 reciprocal to speak of; the
 * limit also keeps the box test below honest, see there.)
 *
 * TRIANGLE.  sls_ray_triangle is the watertight test of Woop, Benthin and Wald ("Watertight Ray/Triangle Intersection",
 * JCGT 2(1), 2013):
 *   1. kz = the axis of the largest |d| (the first of equal ones), kx, ky the two others in cyclic order, swapped when
 *      d[kz] < 0 so that the winding is kept; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];
 *   2. the vertices relative to the origin, A = a - o (one rounding per component), sheared and scaled:
 *      Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], Az = Sz * A[kz]  — the ray is now the +z axis;
 *   3. the edge functions U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax: two float32 products and
 *      their difference.  If any of the three is exactly 0, all three are recomputed in double, where the products of two
 *      floats are exact and so the sign of the difference is the true sign;
 *   4. a miss when U, V, W have strictly mixed signs (one < 0 and one > 0), or when det = (U + V) + W == 0;
 *   5. T = (U * Az + V * Bz) + W * Cz, t = T / det, u = V / det, v = W / det (of the double values where step 3 fell
 *      back, rounded to float32 once); -0 becomes +0; a hit needs t_min <= t <= t_max.
 * Both faces of a triangle hit: there is no culling.  u and v are the barycentric weights of b and c.
 *
 * WHY NO RAY SLIPS THROUGH.  A sheared vertex (step 2) depends on the vertex and the ray ALONE, not on the face it is
 * met in: two faces that share a vertex see the same three numbers for it.  The edge function of a shared edge (P, Q) is
 * fl(Qx * Py) - fl(Qy * Px) in one face and fl(Px * Qy) - fl(Py * Qx) in its neighbour, which walks the edge the other
 * way: the same two rounded products (a float product commutes), subtracted in the other order, and a float difference
 * is exactly the negative of the reversed one.  The double fall-back keeps that: exact products, reversed difference.  So
 * the neighbour's value is the exact negative, also when one face took the fall-back and the other did not (a zero is a
 * zero in both, the signs of the others are the true signs in either precision).  A ray whose sheared origin lies on the
 * inner side of the edge in one face lies on the outer side in the other and the reverse; on the edge exactly (0) it
 * counts as inside for BOTH.  The projected faces around a vertex or along an edge therefore cover the plane without a
 * gap, decided on the same numbers: a ray cannot pass between two faces that share an edge or a vertex, and a ray exactly
 * through a shared edge or vertex hits ALL the faces that share it (the lowest face index then wins by the key).  An fma
 * in step 3 would break this: fma(Qx, Py, -fl(Qy * Px)) is not the negative of fma(Px, Qy, -fl(Py * Qx)).
 * What stays approximate is t, and with it which of two faces at nearly the same depth is in front.  A ray parallel to
 * the face's plane projects it to a segment: the exact edge functions sum to 0, and in float32 a grazing ray is a hit
 * or a miss by rounding.
 *
 * KEY.  t >= +0 in every hit, so (t, face) packs as sls_nn_key(t, face) (sls_nn_math.h): the minimum is the nearest
 * hit, then the lowest face index; SLS_NN_KEY_NONE (+inf, 0xFFFFFFFF) is the miss.
 *
 * BOX.  sls_ray_box: the conservative test the traversal prunes with, see there.
 *
 * Rules for users of this header: no fast-math; HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt and build the object
 * with -ffp-contract=off.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_RAYCAST_MATH_H
#define SLS_RAYCAST_MATH_H

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "sls_nn_math.h"

#define SLS_RAY_MIN_DIR 7.888609052210118e-31f      /* 2^-100 */
#define SLS_RAY_BOX_MARGIN 1.9073486328125e-06f     /* 2^-19 */

/* The ray's frame: the permuted origin, the shear and the axes (steps 1 of the test), computed once per ray. */
typedef struct {
    float ox, oy, oz;       /* o[kx], o[ky], o[kz] */
    float Sx, Sy, Sz;
    int kx, ky, kz;
} sls_ray_frame;

SLS_HD float sls_ray_pick(const float *v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

/* The axis of the largest |d|, the first of equal ones. */
SLS_HD int sls_ray_axis(const float *d)
{
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    int kz = 0;
    float m = ax;
    if (ay > m) { kz = 1; m = ay; }
    if (az > m) kz = 2;
    return kz;
}

SLS_HD int sls_ray_valid(const float *o, const float *d)
{
    const float m = fmaxf(fabsf(d[0]), fmaxf(fabsf(d[1]), fabsf(d[2])));
    int k, ok = 1;
    for (k = 0; k < 3; ++k) ok = ok && fabsf(o[k]) <= FLT_MAX && fabsf(d[k]) <= FLT_MAX;
    return ok && m >= SLS_RAY_MIN_DIR;
}

SLS_HD void sls_ray_setup(const float *o, const float *d, sls_ray_frame *r)
{
#pragma STDC FP_CONTRACT OFF
    const int kz = sls_ray_axis(d);
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = sls_ray_pick(d, kz);
    if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r->kx = kx; r->ky = ky; r->kz = kz;
    r->ox = sls_ray_pick(o, kx); r->oy = sls_ray_pick(o, ky); r->oz = sls_ray_pick(o, kz);
    r->Sx = sls_ray_pick(d, kx) / dz;
    r->Sy = sls_ray_pick(d, ky) / dz;
    r->Sz = 1.0f / dz;
}

/* Steps 2 to 5 for a ray's frame.  1 for a hit (then *t, *u, *v are written), 0 for a miss. */
SLS_HD int sls_ray_triangle_frame(const sls_ray_frame *r, const float *a, const float *b, const float *c, float t_min,
                                  float t_max, float *t, float *u, float *v)
{
#pragma STDC FP_CONTRACT OFF
    const float Akz = sls_ray_pick(a, r->kz) - r->oz, Bkz = sls_ray_pick(b, r->kz) - r->oz, Ckz = sls_ray_pick(c, r->kz) - r->oz;
    const float Ax = (sls_ray_pick(a, r->kx) - r->ox) - r->Sx * Akz, Ay = (sls_ray_pick(a, r->ky) - r->oy) - r->Sy * Akz;
    const float Bx = (sls_ray_pick(b, r->kx) - r->ox) - r->Sx * Bkz, By = (sls_ray_pick(b, r->ky) - r->oy) - r->Sy * Bkz;
    const float Cx = (sls_ray_pick(c, r->kx) - r->ox) - r->Sx * Ckz, Cy = (sls_ray_pick(c, r->ky) - r->oy) - r->Sy * Ckz;
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const float Az = r->Sz * Akz, Bz = r->Sz * Bkz, Cz = r->Sz * Ckz;
    float tt, uu, vv;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        const double Ud = (double)Cx * (double)By - (double)Cy * (double)Bx;
        const double Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
        const double Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
        const double det = (Ud + Vd) + Wd;
        double T;
        if ((Ud < 0.0 || Vd < 0.0 || Wd < 0.0) && (Ud > 0.0 || Vd > 0.0 || Wd > 0.0)) return 0;
        if (det == 0.0) return 0;
        T = (Ud * (double)Az + Vd * (double)Bz) + Wd * (double)Cz;
        tt = (float)(T / det);
        uu = (float)(Vd / det);
        vv = (float)(Wd / det);
    } else {
        const float det = (U + V) + W;
        float T;
        if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return 0;
        if (det == 0.0f) return 0;
        T = (U * Az + V * Bz) + W * Cz;
        tt = T / det;
        uu = V / det;
        vv = W / det;
    }
    tt = tt + 0.0f;                                     /* -0 -> +0: the key orders by the bits of t */
    if (!(tt >= t_min && tt <= t_max)) return 0;        /* (a NaN misses) */
    *t = tt;
    *u = uu;
    *v = vv;
    return 1;
}

SLS_HD int sls_ray_triangle(const float *o, const float *d, const float *a, const float *b, const float *c, float t_min,
                            float t_max, float *t, float *u, float *v)
{
    sls_ray_frame r;
    sls_ray_setup(o, d, &r);
    return sls_ray_triangle_frame(&r, a, b, c, t_min, t_max, t, u, v);
}

/* 1 / d per axis, what sls_ray_box takes: +-inf for a zero (or subnormal-small) component. */
SLS_HD void sls_ray_inverse(const float *d, float *inv_d)
{
#pragma STDC FP_CONTRACT OFF
    inv_d[0] = 1.0f / d[0];
    inv_d[1] = 1.0f / d[1];
    inv_d[2] = 1.0f / d[2];
}

/*
 * The conservative test of ray against box (mn, mx): 0 only if NO triangle with all three vertices inside the box can be
 * reported by sls_ray_triangle for this (valid) ray with t_lo <= t <= t_hi.  kz = sls_ray_axis(d), inv_d from
 * sls_ray_inverse.  It is NOT the textbook "one t inside all three slabs and inside [t_lo, t_hi]", which a hit on a
 * sliver can escape; it asks two weaker things, each of which a reported hit implies:
 *   (1) the ray's LINE meets the box grown by m: the three slab intervals have a common t, whatever its value;
 *   (2) the slab interval of the DOMINANT axis kz, of the box grown by m, meets [t_lo, t_hi];
 * with m = 2^-19 R, R = the largest |mn[k] - o[k]|, |mx[k] - o[k]| over the axes (every vertex in the box is within R of
 * the origin on every axis).
 *
 * What a reported hit gives.  Steps 3 and 4 decide on the float32 sheared vertices, and they decide their signs EXACTLY:
 * a float product rounds monotonically, so fl(p) - fl(q) has the sign of p - q or is 0, and a 0 goes to double, where it
 * is exact.  So the origin of the sheared plane lies inside or on the triangle of the float32 points (Ax, Ay), (Bx, By),
 * (Cx, Cy): some convex weights l give sum l_i Ax_i = sum l_i Ay_i = 0.  Each Ax_i equals
 * (a_i[kx] - o[kx]) - (d[kx] / d[kz]) (a_i[kz] - o[kz]) up to six roundings of quantities <= R: the subtraction of o (two
 * of them, one scaled by |Sx| <= 1), Sx itself, the product, the difference.  So the point P = sum l_i a_i of the face,
 * which the box holds, lies within 6 2^-24 R of the ray's line in kx and in ky at the parameter (P[kz] - o[kz]) / d[kz]:
 * the line meets the box grown by that much.  (1) computes each slab bound as fl(fl(mn - o -+ m) * inv_d): four more
 * roundings of quantities <= R + m.  10.2 2^-24 R in all, against m = 32 2^-24 R.
 * For (2): with U, V, W of one sign, T / det is a weighted mean of Az, Bz, Cz with non-negative weights up to five
 * roundings, and Az_i is (a_i[kz] - o[kz]) / d[kz] up to three: t lies within 8 2^-24 of the largest |parameter| from
 * the range the face spans on the dominant axis, which the box's interval contains: 8 2^-24 R in position, plus the four
 * roundings of the bound, against the same m.
 * What (2) does NOT claim is that t lies inside the slabs of kx and ky: on a face whose projection is a sliver the
 * weights U, V, W are rounding noise, t is anywhere in the face's range on kz, and o + t d can leave the box sideways.
 * Such a hit is still reported by sls_ray_triangle, so the test must not prune it: hence (1) for the line, (2) for kz.
 *
 * The 0 * inf cases.  An axis with inv_d = +-inf (d[k] = 0, or below 2^-128) asks only that o[k] lie within the grown
 * box: nothing is multiplied.  That is exact for d[k] = 0; otherwise |d[k] / d[kz]| < 2^-128 / 2^-100 (sls_ray_valid), and
 * the ray moves less than 2^-28 R sideways over the box.  kz itself always has a finite inverse.  An origin ON a box
 * face gives mn[k] - o[k] = 0, grown to -m: a product of a finite inverse with it is finite.  Every comparison is written
 * so that a NaN (coordinates near FLT_MAX) passes.
 */
/* One axis of it: the interval [*a, *b] of t in which the ray is inside the slab [lo, hi] (offsets from the origin,
 * already grown); an axis the ray does not move along has the whole line or, returning 0, nothing. */
SLS_HD int sls_ray_slab(float lo, float hi, float inv, float *a, float *b)
{
#pragma STDC FP_CONTRACT OFF
    const float t1 = lo * inv, t2 = hi * inv;
    if (fabsf(inv) > FLT_MAX) {
        *a = -INFINITY;
        *b = INFINITY;
        return !(lo > 0.0f || hi < 0.0f);
    }
    *a = t1 < t2 ? t1 : t2;
    *b = t1 < t2 ? t2 : t1;
    return 1;
}

SLS_HD int sls_ray_box(const float *o, const float *inv_d, int kz, const float *mn, const float *mx, float t_lo, float t_hi)
{
#pragma STDC FP_CONTRACT OFF
    const float lx = mn[0] - o[0], hx = mx[0] - o[0], ly = mn[1] - o[1], hy = mx[1] - o[1], lz = mn[2] - o[2], hz = mx[2] - o[2];
    const float R = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
    const float m = R * SLS_RAY_BOX_MARGIN;
    float ax, bx, ay, by, az, bz, near, far, zlo, zhi;
    const int in_x = sls_ray_slab(lx - m, hx + m, inv_d[0], &ax, &bx);
    const int in_y = sls_ray_slab(ly - m, hy + m, inv_d[1], &ay, &by);
    const int in_z = sls_ray_slab(lz - m, hz + m, inv_d[2], &az, &bz);
    near = ax;                                          /* (a NaN bound is skipped: it then rejects nothing) */
    if (ay > near) near = ay;
    if (az > near) near = az;
    far = bx;
    if (by < far) far = by;
    if (bz < far) far = bz;
    zlo = kz == 0 ? ax : (kz == 1 ? ay : az);
    zhi = kz == 0 ? bx : (kz == 1 ? by : bz);
    return in_x && in_y && in_z && !(near > far) && !(zlo > t_hi) && !(zhi < t_lo);
}

#endif /* SLS_RAYCAST_MATH_H */
