/*
 * sls_mesh_math.h — the rules of the mesh cleaning stage (sls_mesh_weld, sls_mesh_clusters, sls_mesh_filter,
 * sls_mesh_vertex_normals), shared by the HIP kernels (csrc/sls_mesh.hip) and by any CPU checker that wants to reproduce
 * their results (tests/mesh_ref.py compiles this header and restates it in NumPy).  DESIGN.md section 2, "Mesh
 * cleaning", states the contract.
 *
 * ---- weld ------------------------------------------------------------------------------------------------------------
 * A soup row is three float32 words, read as integers: two rows are the same vertex iff all three words are equal
 * (-0.0 and 0.0 stay apart, NaN payloads are compared as bits).  The unique rows leave in ascending lexicographic order
 * of (x, y, z) as SIGNED int32 — what torch.unique(dim=0) gives on the int32 view — and index[r] is the rank of row r.
 * sls_mesh_word_key flips the sign bit: unsigned order of the keys = signed order of the words, so three stable LSD
 * sorts over the keys of z, then y, then x leave the rows in that order.
 *
 * ---- the triangle graph ----------------------------------------------------------------------------------------------
 * A triangle (a, b, c) over V vertices is degenerate iff two of its indices are equal or one lies outside [0, V); the
 * second kind is counted on its own as well (status word "out_of_range" is a subset of "degenerate").  A degenerate
 * triangle has no edges, belongs to no cluster and carries the label -1.  Edge e = 0, 1, 2 of a triangle joins its
 * corners (e, (e + 1) % 3); its key is  min << bits | max  with bits = sls_mesh_index_bits(V): never 0, because
 * min < max.  Two non-degenerate triangles are joined iff they own an edge of the same key (a shared vertex is not
 * enough; every triangle of an edge with more than two is joined).  Clusters are the connected components, numbered
 * 0 .. C-1 in ascending order of their lowest triangle; cluster_count[c] is the number of triangles of cluster c.
 * An edge key owned by exactly one triangle is a boundary edge, by more than two a non-manifold edge; a mesh with
 * neither is closed.
 *
 * ---- selection -------------------------------------------------------------------------------------------------------
 *   k = min(keep_clusters, C);  kth = k > 0 ? the k-th largest cluster_count : 0      (keep_clusters <= 0: no such term)
 *   n_min = max(max(min_triangles, 0), kth)                                           (min_triangles <= 0: no floor)
 * A triangle is kept iff its label is >= 0 and cluster_count[label] >= n_min (ties at the threshold are all kept).  Kept
 * triangles stay in input order; the vertices a kept triangle references stay in input order, all others leave, and the
 * faces are re-indexed.
 *
 * ---- vertex normals --------------------------------------------------------------------------------------------------
 * The normal of vertex v: the sum, in ascending triangle index, of (p1 - p0) x (p2 - p0) (sls_mesh_face_normal:
 * float32, every operation rounded once) over the non-degenerate triangles that reference v, divided by its length
 * (sls_mesh_normalise).  A vertex without such a triangle, or whose sum has a length that is zero or not finite (NaN,
 * an infinity, or an overflow of the squared length), gets (0, 0, 0).
 *
 * Rules for users of this header, as for sls_tsdf_math.h: compile with -ffp-contract=off, no fast-math; HIP: keep
 * -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_MESH_MATH_H
#define SLS_MESH_MATH_H

#include <math.h>
#include <stdint.h>

#include "sls_det_math.h"

/* the sort key of one float32 word read as a signed integer: unsigned order of the keys = signed order of the words */
SLS_HD uint32_t sls_mesh_word_key(uint32_t word)
{
    return word ^ 0x80000000u;
}

/* 1 when the two rows (three words each) are the same vertex */
SLS_HD int sls_mesh_same_row(const uint32_t a[3], const uint32_t b[3])
{
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
}

/* the number of bits that hold every index of [0, V): at least 1, at most 31 */
SLS_HD int sls_mesh_index_bits(int32_t V)
{
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < (int64_t)V) ++bits;
    return bits;
}

/* 0: a triangle with three different indices inside [0, V); 1: two indices are equal; 2: an index is outside */
SLS_HD int sls_mesh_degenerate(const int32_t f[3], int32_t V)
{
    if (f[0] < 0 || f[0] >= V || f[1] < 0 || f[1] >= V || f[2] < 0 || f[2] >= V) return 2;
    return (f[0] == f[1] || f[1] == f[2] || f[2] == f[0]) ? 1 : 0;
}

/* the key of edge e = 0, 1, 2 of a non-degenerate triangle: min << bits | max, never 0 */
SLS_HD uint64_t sls_mesh_edge_key(const int32_t f[3], int e, int bits)
{
    const int32_t a = e == 0 ? f[0] : e == 1 ? f[1] : f[2];
    const int32_t b = e == 0 ? f[1] : e == 1 ? f[2] : f[0];
    const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
    return ((uint64_t)lo << bits) | (uint64_t)hi;
}

/* (the twins of this rule for the clusters of a cloud: sls_cluster_n_min / sls_cluster_keep_rank, include/sls_cluster_math.h) */
/* n_min from the two arguments and the k-th largest cluster count (0 where there is no such term) */
SLS_HD uint32_t sls_mesh_n_min(int32_t min_triangles, uint32_t kth)
{
    const uint32_t floor_ = min_triangles > 0 ? (uint32_t)min_triangles : 0u;
    return floor_ > kth ? floor_ : kth;
}

/* k of the k-th-largest term: min(keep_clusters, C), 0 when there is no such term */
SLS_HD uint32_t sls_mesh_keep_rank(int32_t keep_clusters, uint32_t C)
{
    if (keep_clusters <= 0) return 0u;
    return (uint32_t)keep_clusters < C ? (uint32_t)keep_clusters : C;
}

/* (p1 - p0) x (p2 - p0): twice the triangle's area along its normal */
SLS_HD void sls_mesh_face_normal(const float p0[3], const float p1[3], const float p2[3], float n[3])
{
    const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const float vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    n[0] = uy * vz - uz * vy;
    n[1] = uz * vx - ux * vz;
    n[2] = ux * vy - uy * vx;
}

/* s / |s|, or zeros when the length is zero or not finite */
SLS_HD void sls_mesh_normalise(const float s[3], float n[3])
{
    const float len = sqrtf((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    if (len > 0.0f && len <= 3.402823466e+38f) { n[0] = s[0] / len; n[1] = s[1] / len; n[2] = s[2] / len; }
    else { n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f; }
}

#endif /* SLS_MESH_MATH_H */
