/*
 * sls_fill_math.h — the rules of hole filling (sls_mesh_boundary_loops, sls_mesh_fill_holes), shared by the HIP kernels
 * (csrc/sls_fill.hip) and by any CPU checker that wants to reproduce their results (tests/fill_ref.py compiles this header
 * and restates it in NumPy).  DESIGN.md section 2, "Mesh hole filling", states the contract.  The stage finds the closed
 * boundary loops of a mesh and closes the small ones with a fan over their centroid: no refinement, no fairing.
 *
 * Inputs: vertices V x 3 float32 and faces T x 3 int32 at capacity, optionally the device pair in_counts = [V_live, T_live]
 * (each clamped to V and T; absent: V and T), max_edges >= 3, max_size >= 0 (float64, finite; 0: no limit), and the rows of
 * the two output buffers, cap_vertices >= V and cap_triangles >= T.
 *
 * ---- 1. live range ---------------------------------------------------------------------------------------------------
 * Rows beyond the live counts are ignored and not copied: the stage runs behind sls_mesh_filter, which writes its counts
 * on the device only.  A triangle is degenerate by sls_mesh_degenerate AGAINST V_live (two equal indices, or an index
 * outside [0, V_live); rows of -1 included) and takes no part.
 *
 * ---- 2. boundary half-edges ------------------------------------------------------------------------------------------
 * A non-degenerate live triangle (f0, f1, f2) owns the directed half-edges f0 -> f1, f1 -> f2, f2 -> f0
 * (sls_fill_half_edge).  A half-edge a -> b is a BOUNDARY HALF-EDGE iff its undirected key (sls_mesh_edge_key) is owned by
 * exactly one non-degenerate live triangle: a repeated triangle makes none, an edge with three owners makes none.  They
 * are listed in ascending order of the directed key  a << bits | b  (sls_fill_key; any bits that hold every index give the
 * same order: the order of (a, b)).  B is their number; half-edge h is the h-th of that list.
 *
 * ---- 3. simple and complex vertices ----------------------------------------------------------------------------------
 * A vertex is SIMPLE iff exactly one boundary half-edge leaves it and exactly one enters it (sls_fill_simple).  Any other
 * vertex that a boundary half-edge touches is COMPLEX: two holes pinched at one vertex, a rim next to a non-manifold fin,
 * a rim along a flipped triangle.
 *
 * ---- 4. loops --------------------------------------------------------------------------------------------------------
 * Every boundary half-edge whose head is simple is joined to the one boundary half-edge that leaves that head.  A
 * connected component in which every tail and every head is simple is a LOOP: a cycle h_0 .. h_{L-1} with L >= 3 (L = 2
 * would be an edge with two owners).  Every other boundary half-edge is OPEN, carries the loop number -1 and is never
 * filled.  Loops are numbered in ascending order of their lowest vertex (all tails of a loop differ, and the list is in
 * ascending tail: that is the order of a loop's lowest half-edge).
 *
 * ---- 5. which loops are filled ---------------------------------------------------------------------------------------
 * A loop is filled iff (sls_fill_verdict, the first failing reason counts, in this order)
 *   L <= max_edges                                                                         (else SLS_FILL_SKIP_EDGES)
 *   none of its vertices holds a non-finite coordinate                                     (else SLS_FILL_SKIP_NONFINITE)
 *   max_size == 0, or (dx dx + dy dy) + dz dz <= max_size max_size in float64, dx, dy, dz the float64 differences of the
 *   float32 maxima and minima of the loop's vertices: independent of any order             (else SLS_FILL_SKIP_SIZE)
 *
 * ---- 6. the fill -----------------------------------------------------------------------------------------------------
 * L = 3: with a the loop's lowest vertex, n1 the head of a's half-edge and n2 the head of n1's, the single triangle
 * (a, n2, n1) is written; no vertex is added.
 * L > 3: one vertex c is added, c_k = (float)(S_k / (double)L) (sls_fill_centroid), S_k the float64 sum of coordinate k of
 * the loop's vertices in ASCENDING VERTEX INDEX; for every half-edge a -> b of the loop, in ascending a, the triangle
 * (b, a, c) is written: the orientation of the rim's own triangles.
 *
 * ---- the order of every float64 sum ----------------------------------------------------------------------------------
 * The rule of sls_simplify_math.h and sls_smooth_math.h, stated again.  The three words (S_x, S_y, S_z) of a loop of
 * L <= SLS_FILL_LONG (64) vertices are added one after the other in ascending vertex index, starting from +0.0.  A longer
 * loop is split over 64 lanes: lane l adds the items l, l + 64, l + 128, ... one after the other starting from +0.0, then
 * for off = 32, 16, 8, 4, 2, 1 every lane l replaces its partial sum by part[l] + part[l ^ off] (all lanes at once: a
 * butterfly; a + b == b + a, so every lane ends with the same bits).  Every word follows that order on its own.
 *
 * ---- 7. output -------------------------------------------------------------------------------------------------------
 * Vertices: the V_live input rows copied bit for bit, then the new vertices in loop order (V' rows; rows beyond them are
 * not written).  Faces: the T_live input rows as they are, degenerate rows included, then the new triangles in loop order
 * (T' rows); the remaining rows up to cap_triangles are -1.
 * Room: both needs, V' and T', are always computed and reported.  Where either exceeds its room NOTHING is filled: the
 * output is the live input copied, and the overflow word is 1.
 *
 * Status (16 words): [V', T', B, loops, filled loops, loops skipped for max_edges, skipped for max_size, skipped for a
 * non-finite vertex, open half-edges, complex vertices, degenerate live triangles (both kinds), those of them with an index
 * outside the live vertices, needed vertices, needed triangles, overflow, 1].  On overflow words 0, 1 and 4 are V_live,
 * T_live and 0; words 5 to 7 keep the verdicts.  sls_mesh_boundary_loops fills no hole: its words 0, 1, 4 to 7 and 12 to 14
 * are 0.
 *
 * Rules for users of this header, as for sls_mesh_math.h: compile with -ffp-contract=off, no fast-math.  Plain C99 / HIP
 * device compatible.
 */
#ifndef SLS_FILL_MATH_H
#define SLS_FILL_MATH_H

#include <math.h>
#include <stdint.h>

#include "sls_mesh_math.h"

#define SLS_FILL_LONG 64           /* a loop of more vertices is summed by 64 lanes and a butterfly */

#define SLS_FILL_FILLED 0
#define SLS_FILL_SKIP_EDGES 1
#define SLS_FILL_SKIP_NONFINITE 2
#define SLS_FILL_SKIP_SIZE 3

/* the status words */
#define SLS_FILL_W_VERTICES 0
#define SLS_FILL_W_TRIANGLES 1
#define SLS_FILL_W_HALFEDGES 2
#define SLS_FILL_W_LOOPS 3
#define SLS_FILL_W_FILLED 4
#define SLS_FILL_W_SKIP_EDGES 5
#define SLS_FILL_W_SKIP_SIZE 6
#define SLS_FILL_W_SKIP_NONFINITE 7
#define SLS_FILL_W_OPEN 8
#define SLS_FILL_W_COMPLEX 9
#define SLS_FILL_W_DEGENERATE 10
#define SLS_FILL_W_RANGE 11
#define SLS_FILL_W_NEED_VERTICES 12
#define SLS_FILL_W_NEED_TRIANGLES 13
#define SLS_FILL_W_OVERFLOW 14
#define SLS_FILL_W_WRITTEN 15

SLS_HD int sls_fill_finite(float v)
{
    return fabsf(v) <= 3.402823466e+38f;
}

SLS_HD int sls_fill_finite3(const float p[3])
{
    return sls_fill_finite(p[0]) && sls_fill_finite(p[1]) && sls_fill_finite(p[2]);
}

/* a live count: the word of in_counts clamped to the capacity */
SLS_HD int32_t sls_fill_live(uint32_t count, int32_t capacity)
{
    return count < (uint32_t)capacity ? (int32_t)count : capacity;
}

/* the half-edge e = 0, 1, 2 of a non-degenerate triangle: corner e -> corner (e + 1) % 3 */
SLS_HD void sls_fill_half_edge(const int32_t f[3], int e, int32_t *a, int32_t *b)
{
    *a = e == 0 ? f[0] : e == 1 ? f[1] : f[2];
    *b = e == 0 ? f[1] : e == 1 ? f[2] : f[0];
}

/* the directed key of a -> b (a != b, both inside [0, V)): never 0 */
SLS_HD uint64_t sls_fill_key(int32_t a, int32_t b, int bits)
{
    return ((uint64_t)(uint32_t)a << bits) | (uint64_t)(uint32_t)b;
}

/* a vertex that `out` boundary half-edges leave and `in` enter */
SLS_HD int sls_fill_simple(uint32_t out, uint32_t in)
{
    return out == 1u && in == 1u;
}

/* one vertex of a loop: the bounding box (float32) and whether every coordinate so far was finite */
SLS_HD void sls_fill_box(float lo[3], float hi[3], const float p[3])
{
    lo[0] = p[0] < lo[0] ? p[0] : lo[0]; lo[1] = p[1] < lo[1] ? p[1] : lo[1]; lo[2] = p[2] < lo[2] ? p[2] : lo[2];
    hi[0] = p[0] > hi[0] ? p[0] : hi[0]; hi[1] = p[1] > hi[1] ? p[1] : hi[1]; hi[2] = p[2] > hi[2] ? p[2] : hi[2];
}

/* one item of a loop's sums */
SLS_HD void sls_fill_add(double acc[3], const float p[3])
{
    acc[0] += (double)p[0]; acc[1] += (double)p[1]; acc[2] += (double)p[2];
}

/* rule 5; lo and hi are read only where all_finite */
SLS_HD int sls_fill_verdict(uint32_t L, int all_finite, const float lo[3], const float hi[3], uint32_t max_edges, double max_size)
{
    if (L > max_edges) return SLS_FILL_SKIP_EDGES;
    if (!all_finite) return SLS_FILL_SKIP_NONFINITE;
    if (max_size != 0.0) {
        const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
        if (!((dx * dx + dy * dy) + dz * dz <= max_size * max_size)) return SLS_FILL_SKIP_SIZE;
    }
    return SLS_FILL_FILLED;
}

/* the new vertex of a filled loop of L > 3 vertices */
SLS_HD void sls_fill_centroid(const double acc[3], uint32_t L, float c[3])
{
    const double n = (double)L;
    c[0] = (float)(acc[0] / n); c[1] = (float)(acc[1] / n); c[2] = (float)(acc[2] / n);
}

/* the vertices and triangles a loop adds */
SLS_HD uint32_t sls_fill_new_vertices(uint32_t L, int verdict)
{
    return (verdict == SLS_FILL_FILLED && L > 3u) ? 1u : 0u;
}

SLS_HD uint32_t sls_fill_new_triangles(uint32_t L, int verdict)
{
    return verdict != SLS_FILL_FILLED ? 0u : (L > 3u ? L : 1u);
}

#endif /* SLS_FILL_MATH_H */
