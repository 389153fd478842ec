/*
 * sls_outlier_math.h — the arithmetic of the exact k-nearest-neighbour query (sls_nn_query_k) and of the two outlier
 * filters built on it (sls_outlier_statistical, sls_outlier_radius), shared by the HIP kernels, by a host program and by
 * the NumPy restatement (tests/outlier_ref.py), which reproduce the kernels' results bit for bit.
 *
 * Neighbour list.  For a query q the list is the min(k, Mt) smallest keys sls_nn_key(sls_nn_dist2(q, t), index(t)) over
 * ALL targets t, ascending: nearer first, then lower index.  A target that is the query's own copy (a self-query) is a
 * target like any other, d2 = 0.  Slots beyond Mt hold SLS_NN_KEY_NONE.  The list is built by sls_knn_insert alone.
 *
 * Mean distance of a list: mean = (sum over the list, in list order, of (double)sqrtf(d2_j)) / min(k, Mt) — float32
 * square roots, correctly rounded, a float64 sum, one division.
 *
 * Statistical rule — Open3D's remove_statistical_outlier as RESTATED here from its documented behaviour; Open3D is not a
 * dependency and the rule is pinned against the NumPy restatement, not against Open3D itself.  With mean_i the mean
 * distance of point i's list in a self-query of the cloud (so the point itself, at distance 0, is one of its k) and n = M:
 *
 *     cloud_mean = sum over {mean_i > 0} of mean_i / n
 *     std        = sqrt(sum over {mean_i > 0} of (mean_i - cloud_mean)^2 / (n - 1))
 *     thr        = cloud_mean + std_ratio * std
 *     keep i  iff  mean_i > 0 && mean_i < thr
 *
 * Three consequences: a point whose k - 1 nearest others are exact copies of it has mean 0 and is REMOVED; k = 1 gives
 * every point the mean 0 and removes everything; M = 1 removes the point (0 / (n - 1) is NaN and a comparison with NaN is
 * false).
 *
 * Radius rule — this project's: keep i iff MORE than nb_points targets, the point itself included, have
 * d2 <= radius * radius (one float32 product).  Equivalently M > nb_points and the key at 0-based rank nb_points of the
 * (nb_points + 1)-list has d2 <= r2; hence nb_points <= SLS_NN_K_MAX - 1.  Whether Open3D's remove_radius_outlier puts its
 * boundary at < or <= was not verified.
 *
 * Rules for users of this header: as sls_nn_math.h — no fast-math, -ffp-contract=off where bit equality of std and thr
 * with another build matters (the neighbour lists, the means and both keep rules hold no contractible expression),
 * HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_OUTLIER_MATH_H
#define SLS_OUTLIER_MATH_H

#include "sls_nn_math.h"

#ifndef SLS_NN_K_MAX
#define SLS_NN_K_MAX 32     /* (include/sls_abi.h defines the same) */
#endif

#if defined(__HIPCC__) || defined(__HIP__)
#define SLS_UNROLL _Pragma("unroll")
#else
#define SLS_UNROLL
#endif

/* The list length the kernels are instantiated for: the smallest of 4, 8, 16, 32 that is >= k (1 <= k <= 32). */
SLS_HD int sls_knn_list_length(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

/* Insertion of `key` into the ascending list[0 .. K): afterwards the list holds the K smallest of its former entries and
 * the key, ascending.  K is a compile-time constant at every call site: the loop unrolls fully and the list stays in
 * registers.  Whole keys are compared, never the distances alone.  (A key equal to an entry is inserted again: a caller
 * presents every target once.) */
SLS_HD void sls_knn_insert(uint64_t *list, const int K, uint64_t key)
{
    SLS_UNROLL
    for (int j = 0; j < K; ++j) {
        const uint64_t e = list[j];
        const int below = key < e;
        list[j] = below ? key : e;
        key = below ? e : key;
    }
}

/* Mean distance of the entries list[first .. first + n) of a list of length K (n >= 1), in list order. */
SLS_HD double sls_knn_mean(const uint64_t *list, const int K, int first, int n)
{
    double sum = 0.0;
    SLS_UNROLL
    for (int j = 0; j < K; ++j)
        if (j >= first && j < first + n) sum += (double)sqrtf(sls_nn_key_dist2(list[j]));
    return sum / (double)n;
}

/* Statistical rule: does mean_i take part in the sums? */
SLS_HD int sls_outlier_counts(double mean) { return mean > 0.0; }

/* cloud_mean from the sum of the counted means */
SLS_HD double sls_outlier_cloud_mean(double sum, int M) { return sum / (double)M; }

/* one counted point's term of the second sum */
SLS_HD double sls_outlier_dev2(double mean, double cloud_mean)
{
    const double d = mean - cloud_mean;
    return d * d;
}

/* std and thr from the second sum */
SLS_HD double sls_outlier_std(double dev2_sum, int M) { return sqrt(dev2_sum / (double)(M - 1)); }
SLS_HD double sls_outlier_threshold(double cloud_mean, double std, double std_ratio) { return cloud_mean + std_ratio * std; }

SLS_HD int sls_outlier_keep_statistical(double mean, double thr) { return mean > 0.0 && mean < thr; }

/* Radius rule: rank_key = the key at rank nb_points of the point's (nb_points + 1)-list (SLS_NN_KEY_NONE: the cloud holds
 * no more than nb_points points). */
SLS_HD int sls_outlier_keep_radius(uint64_t rank_key, float radius)
{
    const float r2 = radius * radius;
    return rank_key != SLS_NN_KEY_NONE && sls_nn_key_dist2(rank_key) <= r2;
}

#endif /* SLS_OUTLIER_MATH_H */
