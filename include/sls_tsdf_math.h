/*
 * sls_tsdf_math.h — the arithmetic of the sparse TSDF volume (sls_tsdf_blocks, sls_tsdf_integrate, sls_tsdf_extract),
 * shared by the HIP kernels (csrc/sls_tsdf.hip) and by any CPU checker that wants to reproduce their results
 * (tests/tsdf_ref.py restates it in NumPy).  DESIGN.md section 2, "TSDF volume", states the contract.
 *
 * ---- the volume ----------------------------------------------------------------------------------------------------
 * A block is 8 x 8 x 8 voxels of edge voxel_size.  Block b (int32 x 3, |b_a| < 2^20) covers
 * origin + 8 voxel_size [b, b + 1); its voxel l = x | y << 3 | z << 6 lives at slot 512 k + l of block k and has the
 * global voxel coordinate g = 8 b + (x, y, z).  The centre of global voxel coordinate g_a along axis a is
 *   c_a = (float)(origin_a + ((double)g_a + 0.5) * voxel_size)     float64: one product, one sum; rounded once
 * Blocks are kept in ascending order of the key  kx | ky << 21 | kz << 42,  k_a = b_a + 2^20  (every k_a in (0, 2^21):
 * a key is never 0, which marks "no block" in the key stream).
 *
 * ---- which blocks exist (sls_tsdf_blocks) ---------------------------------------------------------------------------
 * A point p (float32) with margin m = trunc + voxel_size (float64; m <= 8 voxel_size is an argument condition) names
 * every block the box [p - m, p + m] touches.  Per axis
 *   lo_a  = floor((((double)p_a - m) - origin_a) / (8.0 * voxel_size)),  hi_a likewise with + m      float64, IEEE division
 *   mid_a = floor(((double)p_a - origin_a) / (8.0 * voxel_size))
 * lo <= mid <= hi (every operation is monotone) and hi - lo <= 2 (the box is at most two blocks wide), so {lo, mid, hi}
 * is the whole range: 27 candidate keys per point, candidate j = jx + 3 jy + 9 jz taking lo / mid / hi for j_a = 0 / 1 / 2.
 * (The corners of the box alone are not enough: with 2 m > 8 voxel_size — the default trunc = 4 voxel_size gives 10 — a
 * point in the middle of a block has lo = mid - 1 and hi = mid + 1, and a wall through the middle of a row of blocks
 * would leave exactly the blocks it runs through unnamed.)  A point with a non-finite coordinate names nothing and is
 * counted; a point one of whose lo / hi is not inside (-2^20, 2^20) names nothing and is counted.
 *
 * ---- one keyframe into the volume (sls_tsdf_integrate) -------------------------------------------------------------
 * Float32, every operation rounded once, no fma except inside sls_atan2 / sls_asin01 (include/sls_det_math.h):
 *   q   = ((R0 cx + R1 cy) + R2 cz) + t   per row of Rvw / tvw        rho = sqrt((qx qx + qy qy) + qz qz)
 *   skip if !(rho >= near_cut)
 *   az  = sls_atan2(qy, qx);  s = qz / rho;  el = copysign(sls_asin01(min(|s|, 1)), s)
 *   u   = fx az + cx,  v = fy el + cy;   c = floor(u + 1),  r = floor(v + 1);   c mod W where the camera wraps
 *   skip if (c, r) is outside the image;  pixel valid iff !(alpha < min_opacity) && !(dist > max_depth_dist)
 *   depth = (alpha > 0 ? D / alpha : D) (1 - depth_ratio) + median depth_ratio          (the rule of sls_surface.hip)
 *   skip if the pixel is invalid or !(depth > 0);   sdf = depth - rho;   skip if !(sdf >= -trunc)
 *   t = min(1, sdf / trunc);   tsdf <- (tsdf weight + t) / (weight + 1);   weight <- weight + 1
 *
 * ---- the zero surface (sls_tsdf_extract) ---------------------------------------------------------------------------
 * Marching tetrahedra over the Freudenthal split.  The cube at global voxel g has the corners g + (dx, dy, dz), corner
 * index dx | dy << 1 | dz << 2.  Tetrahedron t = 0..5 is the t-th permutation (a, b, c) of the axes in lexicographic
 * order, with the corners v0 = 0, v1 = 1 << a, v2 = v1 | 1 << b, v3 = 7: det(v1 - v0, v2 - v0, v3 - v0) is the sign of
 * the permutation, + for t = 0, 3, 4.  A corner is inside iff tsdf < 0.  With the tetrahedron positively oriented and
 * "ij" the vertex on the edge between its corners i and j:
 *   one corner i inside        (ia, ib, ic)           (i, a, b, c) the even permutation of (0, 1, 2, 3) that starts with
 *                                                     i: (0,1,2,3) (1,0,3,2) (2,0,1,3) (3,0,2,1)
 *   one corner i outside       (ia, ic, ib)
 *   two corners i < j inside   (ik, il, jl), (ik, jl, jk)      (i, j, k, l) the even permutation: (0,1,2,3) (0,2,3,1)
 *                                                     (0,3,1,2) (1,2,0,3) (1,3,2,0) (2,3,0,1)
 * and a negatively oriented tetrahedron swaps the last two vertices of each triangle: every normal points to the
 * positive side.  sls_tet_case holds these 16 cases as packed words; tests/test_tsdf_math.py rebuilds them from the
 * rule above and checks the orientation of every case against the gradient of the linear interpolant.
 * The vertex on the edge between cube corners A < B (corner indices: A is the corner of the lower global voxel
 * coordinate in (z, y, x) order) is  s = tA / (tA - tB),  p_a = cA_a + s (cB_a - cA_a)  in float32 — the same bits from
 * every tetrahedron and every cube that shares the edge.
 *
 * Rules for users of this header, as for sls_det_math.h: compile with -ffp-contract=off, no fast-math; HIP: keep
 * -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_TSDF_MATH_H
#define SLS_TSDF_MATH_H

#include <math.h>
#include <stdint.h>

#include "sls_det_math.h"

#define SLS_TSDF_BLOCK 8
#define SLS_TSDF_BLOCK_VOXELS 512
#define SLS_TSDF_KEY_BIAS 1048576         /* 2^20 */
#define SLS_TSDF_KEY_LIMIT 1048576.0      /* |b_a| < 2^20 */
#define SLS_TSDF_KEY_BITS 63
#define SLS_TSDF_POINT_KEYS 27            /* candidate keys per point: {lo, mid, hi}^3 */

/* floor((c - origin) / (8 voxel_size)) as a double (an integer value, or not finite) */
SLS_HD double sls_tsdf_block_index(double c, double origin, double voxel_size)
{
    return floor((c - origin) / (8.0 * voxel_size));
}

/* 1 when the index lies inside (-2^20, 2^20) */
SLS_HD int sls_tsdf_index_ok(double b)
{
    return b > -SLS_TSDF_KEY_LIMIT && b < SLS_TSDF_KEY_LIMIT;
}

/* the key of block (bx, by, bz), every |b_a| < 2^20 */
SLS_HD uint64_t sls_tsdf_key(int32_t bx, int32_t by, int32_t bz)
{
    return (uint64_t)(uint32_t)(bx + SLS_TSDF_KEY_BIAS) | ((uint64_t)(uint32_t)(by + SLS_TSDF_KEY_BIAS) << 21) |
           ((uint64_t)(uint32_t)(bz + SLS_TSDF_KEY_BIAS) << 42);
}

SLS_HD void sls_tsdf_key_block(uint64_t key, int32_t b[3])
{
    b[0] = (int32_t)(key & 0x1FFFFFu) - SLS_TSDF_KEY_BIAS;
    b[1] = (int32_t)((key >> 21) & 0x1FFFFFu) - SLS_TSDF_KEY_BIAS;
    b[2] = (int32_t)((key >> 42) & 0x1FFFFFu) - SLS_TSDF_KEY_BIAS;
}

/* The 27 candidate keys of a point: 1 and keys[0..27), or 0 (keys all 0) when one of its indices is out of range.
 * The caller has checked that p is finite.  margin = trunc + voxel_size. */
SLS_HD int sls_tsdf_point_keys(const float p[3], const double origin[3], double voxel_size, double margin,
                               uint64_t keys[SLS_TSDF_POINT_KEYS])
{
    int32_t b[3][3];
    int ok = 1;
    for (int a = 0; a < 3; ++a) {
        const double l = sls_tsdf_block_index((double)p[a] - margin, origin[a], voxel_size);
        const double m = sls_tsdf_block_index((double)p[a], origin[a], voxel_size);
        const double h = sls_tsdf_block_index((double)p[a] + margin, origin[a], voxel_size);
        if (sls_tsdf_index_ok(l) && sls_tsdf_index_ok(h)) { b[a][0] = (int32_t)l; b[a][1] = (int32_t)m; b[a][2] = (int32_t)h; }
        else { b[a][0] = b[a][1] = b[a][2] = 0; ok = 0; }
    }
    for (int j = 0; j < SLS_TSDF_POINT_KEYS; ++j)
        keys[j] = ok ? sls_tsdf_key(b[0][j % 3], b[1][(j / 3) % 3], b[2][j / 9]) : 0u;
    return ok;
}

/* c_a of the global voxel coordinate g */
SLS_HD float sls_tsdf_centre(int32_t g, double origin, double voxel_size)
{
    return (float)(origin + ((double)g + 0.5) * voxel_size);
}

/* view-frame position of a voxel centre and its range */
SLS_HD float sls_tsdf_view(const float R[9], const float t[3], const float c[3], float q[3])
{
    for (int k = 0; k < 3; ++k) q[k] = ((R[3 * k] * c[0] + R[3 * k + 1] * c[1]) + R[3 * k + 2] * c[2]) + t[k];
    return sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
}

/* the row-major pixel a view-frame point falls into, -1 when it is outside the image (rho > 0) */
SLS_HD int32_t sls_tsdf_pixel(const float q[3], float rho, float fx, float fy, float cx, float cy, int32_t H, int32_t W,
                              int wrap)
{
    const float az = sls_atan2(q[1], q[0]);
    const float s = q[2] / rho;
    const float e = sls_asin01(fminf(fabsf(s), 1.0f));
    const float el = s < 0.0f ? -e : e;
    const float u = fx * az + cx, v = fy * el + cy;
    const float cf = floorf(u + 1.0f), rf = floorf(v + 1.0f);
    if (!(fabsf(cf) < 1.0e9f) || !(rf >= 0.0f) || !(rf < (float)H)) return -1;
    int32_t c = (int32_t)cf;
    const int32_t r = (int32_t)rf;
    if (wrap) {
        c %= W;
        if (c < 0) c += W;
    }
    if (c < 0 || c >= W) return -1;
    return r * W + c;
}

/* One observation of a voxel at range rho by the pixel (D, alpha, median, dist): 1 when *tsdf / *weight were updated */
SLS_HD int sls_tsdf_update(float D, float alpha, float median, float dist, float rho, float min_opacity,
                           float max_depth_dist, float depth_ratio, float trunc, float *tsdf, float *weight)
{
    if (alpha < min_opacity || dist > max_depth_dist) return 0;
    const float Dh = alpha > 0.0f ? D / alpha : D;
    const float depth = Dh * (1.0f - depth_ratio) + median * depth_ratio;
    if (!(depth > 0.0f)) return 0;
    const float sdf = depth - rho;
    if (!(sdf >= -trunc)) return 0;
    const float t = fminf(1.0f, sdf / trunc);
    const float w = *weight;
    *tsdf = (*tsdf * w + t) / (w + 1.0f);
    *weight = w + 1.0f;
    return 1;
}

/* cube corners (dx | dy << 1 | dz << 2) of tetrahedron t = 0..5; returns 1 when it is positively oriented */
SLS_HD int sls_tet_corners(int t, int v[4])
{
    const int a = t >> 1;
    const int b = (t & 1) ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);
    v[0] = 0; v[1] = 1 << a; v[2] = v[1] | (1 << b); v[3] = 7;
    return t == 0 || t == 3 || t == 4;
}

/* Case `mask` (bit i: corner i of the tetrahedron is inside) of a positively oriented tetrahedron: bits 0-1 the number
 * of triangles, then six vertices of four bits (bit 4 + 4 n: vertex n), each the edge (i | j << 2) it lies on. */
SLS_HD uint32_t sls_tet_case(int mask)
{
    switch (mask & 15) {
    case 1: return 0x0000C841u;
    case 2: return 0x00009D11u;
    case 3: return 0x09D8DC82u;
    case 4: return 0x0000E621u;
    case 5: return 0x0E6C64C2u;
    case 6: return 0x02E1ED12u;
    case 7: return 0x0000B731u;
    case 8: return 0x00007B31u;
    case 9: return 0x07B4B842u;
    case 10: return 0x0B393192u;
    case 11: return 0x00006E21u;
    case 12: return 0x03727622u;
    case 13: return 0x0000D911u;
    case 14: return 0x00008C41u;
    default: return 0u;
    }
}

/* The vertex on the edge between the cube corners A and B (any order) with the corner values tA, tB (one < 0, the
 * other >= 0); c0 / c1: the centres of the global voxel coordinates g and g + 1 per axis */
SLS_HD void sls_tsdf_edge_vertex(int A, int B, float tA, float tB, const float c0[3], const float c1[3], float p[3])
{
    if (A > B) {
        const int i = A; A = B; B = i;
        const float f = tA; tA = tB; tB = f;
    }
    const float s = tA / (tA - tB);
    for (int k = 0; k < 3; ++k) {
        const float pa = ((A >> k) & 1) ? c1[k] : c0[k], pb = ((B >> k) & 1) ? c1[k] : c0[k];
        p[k] = pa + s * (pb - pa);
    }
}

SLS_HD float sls_tsdf_sel8(const float f[8], int i)
{
    return i == 0 ? f[0] : i == 1 ? f[1] : i == 2 ? f[2] : i == 3 ? f[3] : i == 4 ? f[4] : i == 5 ? f[5] : i == 6 ? f[6] : f[7];
}

/* The triangles of one cube whose eight corners are observed: f the corner values, c0 / c1 as above.  Returns their
 * number (0..12); out: null (count only), or room for 9 floats per triangle, written tetrahedron by tetrahedron. */
SLS_HD int sls_tsdf_cube(const float f[8], const float c0[3], const float c1[3], float *out)
{
    int n = 0;
    for (int t = 0; t < 6; ++t) {
        int v[4];
        const int positive = sls_tet_corners(t, v);
        int mask = 0;
        for (int i = 0; i < 4; ++i) mask |= (sls_tsdf_sel8(f, v[i]) < 0.0f) ? 1 << i : 0;
        const uint32_t code = sls_tet_case(mask);
        const int ntri = (int)(code & 3u);
        if (out) {
            for (int tri = 0; tri < ntri; ++tri)
                for (int k = 0; k < 3; ++k) {
                    const int kk = positive ? k : (k == 0 ? 0 : 3 - k);       /* negative: swap the last two */
                    const uint32_t e = (code >> (4 + 4 * (3 * tri + kk))) & 15u;
                    const int A = v[e & 3u], B = v[e >> 2];
                    sls_tsdf_edge_vertex(A, B, sls_tsdf_sel8(f, A), sls_tsdf_sel8(f, B), c0, c1, out + 9 * (n + tri) + 3 * k);
                }
        }
        n += ntri;
    }
    return n;
}

#endif /* SLS_TSDF_MATH_H */
