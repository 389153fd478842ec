/*
 * sls_cluster_math.h — the rule of the density clustering of a point cloud (sls_cloud_dbscan) and of the selection of its
 * large clusters (sls_cloud_select), shared by the HIP kernels, by a host program and by the NumPy restatement
 * (tests/cluster_ref.py), which reproduce the kernels' results bit for bit.
 *
 * WHAT THIS IS: DBSCAN (Ester, Kriegel, Sander, Xu, KDD 1996) with the border rule of Open3D's cluster_dbscan AS RESTATED
 * HERE from its documented behaviour.  Open3D is not a dependency and was not at hand: nothing here was compared with it and
 * no parity is claimed; the rule is pinned against the NumPy restatement and the serial routine below.
 *
 * Inputs: a cloud of M finite float32 points, eps (finite, > 0, eps * eps finite), min_points >= 1.
 *
 * Radius test.  r2 = eps * eps, ONE float32 product; d2 = sls_nn_dist2(q, t), the expression every search here uses; t is a
 *   NEIGHBOUR of q iff d2 <= r2.  A point is its own neighbour (d2 = +0) and an exact copy is a neighbour.  Where Open3D puts
 *   its boundary (< or <=) was not verified.  d2 is symmetric to the bit (the differences only change sign), so "neighbour"
 *   is a symmetric relation.
 * Core.  Point i is CORE iff at least min_points points, itself included, are its neighbours.  A count may stop at
 *   min_points: only `count >= min_points` is ever read.
 * Clusters.  The connected components of the graph on the CORE points with an edge per neighbouring pair, numbered
 *   0 .. C-1 in ascending order of their lowest CORE index — not of their lowest member.
 * Border.  A non-core point with at least one core neighbour takes the LOWEST cluster number among its core neighbours'
 *   clusters.  A border point joins nothing: two clusters that touch only through it stay two.
 * Noise.  Any other point: label -1.
 * counts[c] = the points labelled c, cores and borders alike.
 * status[8] = C, cores, borders, noise, the largest count (0 for C = 0), M, 0, 1.
 *
 * Selection — the rule of sls_mesh_filter (include/sls_mesh_math.h), word for word:
 *   n_min = max(max(min_cluster_points, 0), the min(keep, C)-th largest count), the second term 0 for keep <= 0 or C = 0;
 *   a point is kept iff its label is >= 0 and counts[label] >= n_min.  Clusters that tie at the K-th place all stay.  Kept
 *   rows stay in ascending original index.  status[4] = kept, n_min, M, 1.
 *
 * Everything is integers and one float32 comparison, so a device search that shows every neighbour once equals the brute
 * force over all pairs below BIT FOR BIT on any finite input, not only on lattices.
 *
 * Rules for users of this header: as sls_nn_math.h — the fmaf calls are explicit, no fast-math.  Plain C99 / HIP device
 * compatible; the serial routines are host code.
 */
#ifndef SLS_CLUSTER_MATH_H
#define SLS_CLUSTER_MATH_H

#include "sls_nn_math.h"

#ifndef SLS_CLUSTER_STATUS_WORDS
#define SLS_CLUSTER_STATUS_WORDS 8      /* (include/sls_abi.h defines the same) */
#define SLS_CLUSTER_SELECT_STATUS_WORDS 4
#endif
#define SLS_CLUSTER_NONE 0xFFFFFFFFu    /* the root of a point that belongs to no cluster */

SLS_HD float sls_cluster_r2(float eps) { return eps * eps; }

/* eps and its square as the calls accept them */
SLS_HD int sls_cluster_eps_ok(float eps)
{
    const float r2 = sls_cluster_r2(eps);
    return eps > 0.0f && eps <= 3.4028234663852886e38f && r2 <= 3.4028234663852886e38f;
}

SLS_HD int sls_cluster_near(float d2, float r2) { return d2 <= r2; }

SLS_HD int sls_cluster_core(int32_t count, int32_t min_points) { return count >= min_points; }

/* The squared distance beyond which a target cannot matter to a point that counts its neighbours: r2 until the count has
 * reached min_points, and after that a value no squared distance or gap (>= 0) passes. */
SLS_HD float sls_cluster_count_bound(int32_t count, int32_t min_points, float r2)
{
    return sls_cluster_core(count, min_points) ? -1.0f : r2;
}

/* (the twins of this rule for the clusters of a mesh: sls_mesh_keep_rank / sls_mesh_n_min, include/sls_mesh_math.h) */
/* k of the k-th-largest term: min(keep, C), 0 when there is no such term */
SLS_HD uint32_t sls_cluster_keep_rank(int32_t keep, uint32_t C)
{
    if (keep <= 0) return 0u;
    return (uint32_t)keep < C ? (uint32_t)keep : C;
}

/* n_min from the floor and the k-th largest cluster count (0 where there is no such term) */
SLS_HD uint32_t sls_cluster_n_min(int32_t min_cluster_points, uint32_t kth)
{
    const uint32_t floor_ = min_cluster_points > 0 ? (uint32_t)min_cluster_points : 0u;
    return floor_ > kth ? floor_ : kth;
}

SLS_HD int sls_cluster_keep(int32_t label, const int32_t *counts, uint32_t C, uint32_t n_min)
{
    return label >= 0 && (uint32_t)label < C && (uint32_t)counts[label] >= n_min;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* ---- the serial reference: all pairs, O(M^2) -------------------------------------------------------------------------
 * labels [M], counts [room for M; the entries from C on are left unspecified], status [8], work [M] words.
 * Returns 0, or 1 for arguments the calls refuse. */
static inline uint32_t sls_cluster_find_host(uint32_t *parent, uint32_t x)
{
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

static inline int sls_cluster_dbscan_host(int32_t M, const float *xyz, float eps, int32_t min_points, int32_t *labels,
                                          int32_t *counts, uint32_t *status, uint32_t *work)
{
    if (M < 0 || !sls_cluster_eps_ok(eps) || min_points < 1) return 1;
    const float r2 = sls_cluster_r2(eps);
    uint32_t *parent = work;
    uint32_t C = 0u, cores = 0u, borders = 0u, noise = 0u, largest = 0u;
    /* core flags, in labels */
    for (int32_t i = 0; i < M; ++i) {
        int32_t n = 0;
        for (int32_t j = 0; j < M && !sls_cluster_core(n, min_points); ++j)
            n += sls_cluster_near(sls_nn_dist2(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]), r2);
        labels[i] = sls_cluster_core(n, min_points);
        parent[i] = (uint32_t)i;
    }
    /* components of the cores: the larger root under the smaller, so a root is its component's lowest core */
    for (int32_t i = 0; i < M; ++i) {
        if (!labels[i]) continue;
        for (int32_t j = 0; j < i; ++j) {
            if (!labels[j]) continue;
            if (!sls_cluster_near(sls_nn_dist2(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]), r2))
                continue;
            const uint32_t a = sls_cluster_find_host(parent, (uint32_t)i), b = sls_cluster_find_host(parent, (uint32_t)j);
            if (a < b) parent[b] = a; else if (b < a) parent[a] = b;
        }
    }
    for (int32_t i = 0; i < M; ++i)
        if (labels[i]) parent[i] = sls_cluster_find_host(parent, (uint32_t)i);
    /* borders: the lowest root among the core neighbours (the roots of non-core points are read by nobody) */
    for (int32_t i = 0; i < M; ++i) {
        if (labels[i]) continue;
        uint32_t best = SLS_CLUSTER_NONE;
        for (int32_t j = 0; j < M; ++j) {
            if (!labels[j]) continue;
            if (sls_cluster_near(sls_nn_dist2(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]), r2))
                best = parent[j] < best ? parent[j] : best;
        }
        parent[i] = best;
    }
    /* numbers in ascending order of the root (counts serves as the map root -> number first), labels, counts */
    for (int32_t i = 0; i < M; ++i)
        if (labels[i] && parent[i] == (uint32_t)i) counts[i] = (int32_t)C++;
    for (int32_t i = 0; i < M; ++i) {
        if (labels[i]) ++cores; else if (parent[i] != SLS_CLUSTER_NONE) ++borders; else ++noise;
        labels[i] = parent[i] == SLS_CLUSTER_NONE ? -1 : counts[parent[i]];
    }
    for (uint32_t c = 0; c < C; ++c) counts[c] = 0;
    for (int32_t i = 0; i < M; ++i)
        if (labels[i] >= 0) ++counts[labels[i]];
    for (uint32_t c = 0; c < C; ++c) largest = (uint32_t)counts[c] > largest ? (uint32_t)counts[c] : largest;
    status[0] = C; status[1] = cores; status[2] = borders; status[3] = noise; status[4] = largest; status[5] = (uint32_t)M;
    status[6] = 0u; status[7] = 1u;
    return 0;
}

/* out_index [room for M]: the kept rows, ascending; status [4] */
static inline int sls_cluster_select_host(int32_t M, const int32_t *labels, const int32_t *counts, uint32_t C, int32_t keep,
                                          int32_t min_cluster_points, int32_t *out_index, uint32_t *status)
{
    if (M < 0 || C > (uint32_t)M) return 1;
    const uint32_t k = sls_cluster_keep_rank(keep, C);
    uint32_t kth = 0u, kept = 0u;
    if (k > 0u) {       /* the largest v with at least k counts >= v */
        uint32_t lo = 1u, hi = (uint32_t)M;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            uint32_t n = 0u;
            for (uint32_t c = 0; c < C; ++c) n += (uint32_t)counts[c] >= mid;
            if (n >= k) lo = mid; else hi = mid - 1u;
        }
        kth = lo;
    }
    const uint32_t n_min = sls_cluster_n_min(min_cluster_points, kth);
    for (int32_t i = 0; i < M; ++i)
        if (sls_cluster_keep(labels[i], counts, C, n_min)) out_index[kept++] = i;
    status[0] = kept; status[1] = n_min; status[2] = (uint32_t)M; status[3] = 1u;
    return 0;
}
#endif

#endif /* SLS_CLUSTER_MATH_H */
