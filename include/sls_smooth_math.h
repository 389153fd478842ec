/*
 * sls_smooth_math.h — the rules of mesh smoothing over the edge graph (sls_mesh_adjacency, sls_mesh_smooth), shared by the
 * HIP kernels (csrc/sls_smooth.hip) and by any CPU checker that wants to reproduce their results (tests/smooth_ref.py
 * compiles this header and restates it in NumPy).  DESIGN.md section 2, "Mesh smoothing", states the contract.  It restates
 * what Open3D documents for filter_smooth_simple, filter_smooth_laplacian and filter_smooth_taubin; where that leaves
 * something open (the order of a vertex's neighbours, the order of the sums) this header defines it.
 *
 * Inputs: vertices V x 3 float32, faces T x 3 int32, method (SLS_SMOOTH_SIMPLE / _LAPLACIAN / _TAUBIN), weights
 * (SLS_SMOOTH_UNIFORM / _INVERSE_DISTANCE), iterations n >= 0, lambda and mu (float64, finite), fix_boundary.
 *
 * ---- 1. adjacency ----------------------------------------------------------------------------------------------------
 * A triangle is degenerate by sls_mesh_degenerate (two equal indices, or an index outside [0, V); rows of -1 included: the
 * stage runs behind sls_mesh_filter and sls_mesh_simplify at capacity) and takes no part.  Every edge (a, b) of a
 * non-degenerate triangle makes a and b neighbours of each other.  nbr(v) is the set of DISTINCT neighbours of v in
 * ascending index: a repeated triangle, the opposite orientation and a non-manifold edge add nothing twice.  In CSR form:
 * offsets[v] (V + 1 entries) and neighbours (2 E entries, E = the number of distinct undirected edges), nbr(v) =
 * neighbours[offsets[v] .. offsets[v + 1]).  The construction: the directed pairs (a, b) of both directions of all three
 * edges (sls_smooth_face_pair), sorted by a, then b — the order of the keys  a << bits | b  (sls_smooth_key, bits =
 * sls_mesh_index_bits(V); never 0, because a != b); the distinct pairs in that order are the neighbour lists of all
 * vertices one after the other.
 * A vertex is LIVE iff nbr(v) is not empty.  A vertex is a BOUNDARY VERTEX iff it is an end of an edge that exactly one
 * non-degenerate triangle owns (the boundary edge of sls_mesh_math.h): the key (a, b) then appears exactly once.
 * The adjacency, the live set and the boundary set are those of the input mesh for all steps.
 *
 * ---- 2. one step with factor f: positions P (float32) to P' (float32) ------------------------------------------------
 * A vertex that is not live is copied bit for bit; with fix_boundary a boundary vertex is PINNED and copied bit for bit.
 * Every other vertex i, with neighbours n_0 < n_1 < ... < n_{N-1}:
 *   w_k = 1.0                                                          (uniform)
 *   w_k = 1.0 / ((double)d + 1e-12),  d = sqrtf((dx dx + dy dy) + dz dz),  dx, dy, dz = the float32 differences
 *         P[n_k] - P[i]                                                (inverse distance: sls_smooth_weight)
 *   S_a = sum_k w_k (double)P[n_k]_a  (the product rounded once, then added),  W = sum_k w_k      (sls_smooth_add)
 *   P'[i]_a = (float)((double)P[i]_a + f (S_a / W - (double)P[i]_a))                              (sls_smooth_step)
 * The distance is float32 on purpose: sqrtf is correctly rounded on both sides (-fhip-fp32-correctly-rounded-divide-sqrt;
 * sls_mesh_normalise relies on it too).  Two coincident neighbours (d = 0) weigh 1e12.
 * The SIMPLE step (filter_smooth_simple) is its own rule, with w_k = 1.0:
 *   P'[i]_a = (float)(((double)P[i]_a + S_a) / (double)(N + 1))                                    (sls_smooth_simple)
 *
 * ---- the order of every float64 sum ----------------------------------------------------------------------------------
 * The rule of sls_simplify_math.h, stated again.  The four words (S_x, S_y, S_z, W) of a row of N <= SLS_SMOOTH_LONG (64)
 * neighbours are added one after the other in ascending k, starting from +0.0.  A longer row is split over 64 lanes: lane
 * l adds the items l, l + 64, l + 128, ... one after the other starting from +0.0, then for off = 32, 16, 8, 4, 2, 1 every
 * lane l replaces its partial sum by part[l] + part[l ^ off] (all lanes at once: a butterfly; a + b == b + a, so every
 * lane ends with the same bits).  Every word follows that order on its own.
 *
 * ---- 3. methods ------------------------------------------------------------------------------------------------------
 *   simple:    n simple steps.
 *   laplacian: n steps with f = lambda.
 *   taubin:    n times (a step with f = lambda, then a step with f = mu).
 * Positions are rounded to float32 between all steps; n = 0 copies the input.  Open3D's defaults: lambda 0.5, mu -0.53.
 *
 * Status: [live vertices, E, boundary vertices, live vertices with a non-finite coordinate (of the INPUT positions; 0 from
 * sls_mesh_adjacency, which sees no positions), degenerate triangles (both kinds), those of them with an index outside
 * [0, V), the largest row length, 1].  Where the non-finite count is not 0 the positions are unspecified.
 *
 * Rules for users of this header, as for sls_mesh_math.h: compile with -ffp-contract=off, no fast-math; HIP: keep
 * -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_SMOOTH_MATH_H
#define SLS_SMOOTH_MATH_H

#include <math.h>
#include <stdint.h>

#include "sls_mesh_math.h"

#define SLS_SMOOTH_LONG 64         /* a row of more neighbours is summed by 64 lanes and a butterfly */

#define SLS_SMOOTH_SIMPLE 0
#define SLS_SMOOTH_LAPLACIAN 1
#define SLS_SMOOTH_TAUBIN 2

#define SLS_SMOOTH_UNIFORM 0
#define SLS_SMOOTH_INVERSE_DISTANCE 1

SLS_HD int sls_smooth_finite(float v)
{
    return fabsf(v) <= 3.402823466e+38f;
}

/* the directed key of neighbour b in the row of a (a != b, both inside [0, V)): never 0 */
SLS_HD uint64_t sls_smooth_key(int32_t a, int32_t b, int bits)
{
    return ((uint64_t)(uint32_t)a << bits) | (uint64_t)(uint32_t)b;
}

/* the directed pair j = 0 .. 5 of a non-degenerate triangle: edge j / 2 (corners e, (e + 1) % 3), forwards then backwards */
SLS_HD void sls_smooth_face_pair(const int32_t f[3], int j, int32_t *a, int32_t *b)
{
    const int e = j >> 1;
    const int32_t p = e == 0 ? f[0] : e == 1 ? f[1] : f[2];
    const int32_t q = e == 0 ? f[1] : e == 1 ? f[2] : f[0];
    *a = (j & 1) ? q : p;
    *b = (j & 1) ? p : q;
}

/* ... and its key */
SLS_HD uint64_t sls_smooth_face_key(const int32_t f[3], int j, int bits)
{
    int32_t a, b;
    sls_smooth_face_pair(f, j, &a, &b);
    return sls_smooth_key(a, b, bits);
}

/* the weight of neighbour pn for vertex pi */
SLS_HD double sls_smooth_weight(const float pi[3], const float pn[3], int weights)
{
    if (weights == SLS_SMOOTH_UNIFORM) return 1.0;
    const float dx = pn[0] - pi[0], dy = pn[1] - pi[1], dz = pn[2] - pi[2];
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    return 1.0 / ((double)d + 1e-12);
}

/* one item of a row's sums: acc = (S_x, S_y, S_z, W) */
SLS_HD void sls_smooth_add(double acc[4], double w, const float pn[3])
{
    const double x = w * (double)pn[0], y = w * (double)pn[1], z = w * (double)pn[2];
    acc[0] += x; acc[1] += y; acc[2] += z; acc[3] += w;
}

/* the position after a step with factor f */
SLS_HD void sls_smooth_step(const float pi[3], const double acc[4], double f, float out[3])
{
    const double x = (double)pi[0], y = (double)pi[1], z = (double)pi[2];
    out[0] = (float)(x + f * (acc[0] / acc[3] - x));
    out[1] = (float)(y + f * (acc[1] / acc[3] - y));
    out[2] = (float)(z + f * (acc[2] / acc[3] - z));
}

/* the position after a simple step over N neighbours (acc from uniform weights) */
SLS_HD void sls_smooth_simple(const float pi[3], const double acc[4], uint32_t N, float out[3])
{
    const double c = (double)(N + 1u);
    out[0] = (float)(((double)pi[0] + acc[0]) / c);
    out[1] = (float)(((double)pi[1] + acc[1]) / c);
    out[2] = (float)(((double)pi[2] + acc[2]) / c);
}

#endif /* SLS_SMOOTH_MATH_H */
