/*
 * sls_cloud_math.h — the arithmetic of the voxel down-sampling (sls_voxel_downsample) and of the mesh sampling
 * (sls_mesh_sample), shared by the HIP kernels and by any CPU checker that wants to reproduce their results
 * (tests/cloud_ref.py restates it in NumPy).  Both operations restate what Open3D documents for voxel_down_sample and
 * sample_points_uniformly; where Open3D leaves something open (the order of the output rows, the random stream) this
 * header defines it.
 *
 * ---- voxel down-sampling -------------------------------------------------------------------------------------------
 *   mn_a  = the float32 minimum of axis a over the cloud
 *   o_a   = (double)mn_a - 0.5 * voxel_size                     one product, one subtraction, float64
 *   i_a   = floor(((double)p_a - o_a) / voxel_size)             an IEEE subtraction and DIVISION, not a reciprocal
 *   key   = ix | iy << 21 | iz << 42                            every index in [0, 2^21)
 * p_a >= mn_a, so i_a >= 0.  A point with an index >= 2^21 (or a quotient that is not below 2^21 at all: +inf) is
 * counted and gets key 0; a point with a non-finite coordinate never reaches this arithmetic.  Output row v is the voxel
 * of the v-th smallest key; its coordinate is (float)(sum_a / (double)count) with sum_a the float64 sum of the voxel's
 * (double)p_a.  The order of that sum is fixed by the kernel (sls_cloud.hip), not by this header; where the coordinates
 * are multiples of 1/16 of magnitude <= 64 every partial sum of up to 2^42 points is exact and the order does not matter.
 *
 * ---- mesh sampling --------------------------------------------------------------------------------------------------
 * Face area, float64 from the float32 vertices, every operation rounded once, no fma:
 *   e1 = v1 - v0, e2 = v2 - v0                                  (componentwise)
 *   cx = e1y e2z - e1z e2y,  cy = e1z e2x - e1x e2z,  cz = e1x e2y - e1y e2x
 *   A  = 0.5 * sqrt((cx cx + cy cy) + cz cz)
 * A face has weight 0 when a vertex index is outside [0, V), when A is not finite, or when a crop box is given and one
 * of its vertices lies outside the CLOSED box (float32 comparisons; a NaN coordinate is outside).  Otherwise
 *   w  = (uint64)floor(A / A_max * 4294967296.0)                A_max = the largest area: w <= 2^32
 * so the prefix sum C of the weights is an integer, exact in any order, and W = C[F - 1] < 2^63.  Faces below 2^-32 of
 * the largest one get w = 0 and are NEVER drawn — next to the largest face they would be hit by fewer than one sample in
 * four billion.
 * Sample i: (r0, r1, r2, r3) = Philox4x32-10 of counter (i, 2, 0, 0) under key (seed low word, seed high word) — the 2
 * keeps the stream disjoint from the densify draw (0) and the surface samples (1), include/sls_draw_math.h;
 *   t    = mulhi64(r0 | r1 << 32, W)                             uniform in [0, W)
 *   face = the first f with C[f] > t                             (its weight is > 0)
 *   u1 = sls_draw_uniform(r2), u2 = sls_draw_uniform(r3);  s = sqrtf(u1)
 *   a = 1 - s,  b = s (1 - u2),  c = s u2;   p_k = (a v0_k + b v1_k) + c v2_k        float32, this order
 *
 * Rules for users of this header, as for sls_det_math.h: compile with -ffp-contract=off, no fast-math; HIP: keep
 * -fhip-fp32-correctly-rounded-divide-sqrt (float64 division and square root are correctly rounded as they are).
 * Plain C99 / HIP device compatible.
 */
#ifndef SLS_CLOUD_MATH_H
#define SLS_CLOUD_MATH_H

#include <math.h>
#include <stdint.h>

#include "sls_draw_math.h"

#define SLS_VOXEL_INDEX_BITS 21
#define SLS_VOXEL_INDEX_LIMIT 2097152.0   /* 2^21 */
#define SLS_MESH_STREAM 2u                /* word 1 of the Philox counter */

/* o_a */
SLS_HD double sls_voxel_origin(float mn, double voxel_size)
{
    return (double)mn - 0.5 * voxel_size;
}

/* i_a as a double (an integer value, +inf or — never for p >= mn — negative); the caller compares it with the limit */
SLS_HD double sls_voxel_index(float p, double origin, double voxel_size)
{
    return floor(((double)p - origin) / voxel_size);
}

/* 1 and the key when all three indices are in [0, 2^21), 0 (key 0) otherwise */
SLS_HD int sls_voxel_key(float px, float py, float pz, double ox, double oy, double oz, double voxel_size, uint64_t *key)
{
    const double ix = sls_voxel_index(px, ox, voxel_size), iy = sls_voxel_index(py, oy, voxel_size),
                 iz = sls_voxel_index(pz, oz, voxel_size);
    *key = 0u;
    if (!(ix >= 0.0 && ix < SLS_VOXEL_INDEX_LIMIT && iy >= 0.0 && iy < SLS_VOXEL_INDEX_LIMIT && iz >= 0.0 &&
          iz < SLS_VOXEL_INDEX_LIMIT))
        return 0;
    *key = (uint64_t)ix | ((uint64_t)iy << 21) | ((uint64_t)iz << 42);
    return 1;
}

SLS_HD float sls_voxel_centroid(double sum, uint32_t count)
{
    return (float)(sum / (double)count);
}

/* A of one face */
SLS_HD double sls_mesh_face_area(const float v0[3], const float v1[3], const float v2[3])
{
    const double e1x = (double)v1[0] - (double)v0[0], e1y = (double)v1[1] - (double)v0[1], e1z = (double)v1[2] - (double)v0[2];
    const double e2x = (double)v2[0] - (double)v0[0], e2y = (double)v2[1] - (double)v0[1], e2z = (double)v2[2] - (double)v0[2];
    const double cx = e1y * e2z - e1z * e2y;
    const double cy = e1z * e2x - e1x * e2z;
    const double cz = e1x * e2y - e1y * e2x;
    return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

/* 1 when the vertex lies inside the closed box {min xyz, max xyz} */
SLS_HD int sls_mesh_inside(const float v[3], const float box[6])
{
    return v[0] >= box[0] && v[0] <= box[3] && v[1] >= box[1] && v[1] <= box[4] && v[2] >= box[2] && v[2] <= box[5];
}

/* w of a face of area A (finite, >= 0; 0 for a dropped face) under the largest area A_max */
SLS_HD uint64_t sls_mesh_weight(double area, double area_max)
{
    if (!(area > 0.0) || !(area_max > 0.0)) return 0u;
    return (uint64_t)floor(area / area_max * 4294967296.0);
}

/* the high 64 bits of a * b, in 32-bit pieces (the same on every compiler) */
SLS_HD uint64_t sls_mulhi64(uint64_t a, uint64_t b)
{
    const uint64_t a0 = a & 0xFFFFFFFFu, a1 = a >> 32, b0 = b & 0xFFFFFFFFu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFu) + (p10 & 0xFFFFFFFFu);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

/* the four random words of sample i */
SLS_HD void sls_mesh_words(uint32_t sample, uint64_t seed, uint32_t r[4])
{
    r[0] = sample; r[1] = SLS_MESH_STREAM; r[2] = 0u; r[3] = 0u;
    sls_philox4x32_10(r, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32));
}

/* t in [0, W) */
SLS_HD uint64_t sls_mesh_target(const uint32_t r[4], uint64_t W)
{
    return sls_mulhi64((uint64_t)r[0] | ((uint64_t)r[1] << 32), W);
}

/* the sampled point of a face */
SLS_HD void sls_mesh_point(const uint32_t r[4], const float v0[3], const float v1[3], const float v2[3], float p[3])
{
    const float u1 = sls_draw_uniform(r[2]), u2 = sls_draw_uniform(r[3]);
    const float s = sqrtf(u1);
    const float a = 1.0f - s, b = s * (1.0f - u2), c = s * u2;
    for (int k = 0; k < 3; ++k) p[k] = (a * v0[k] + b * v1[k]) + c * v2[k];
}

#endif /* SLS_CLOUD_MATH_H */
