/*
 * sls_nn_math.h — the arithmetic of the nearest-neighbour query (sls_nn_query) and of the distance statistics
 * (sls_nn_stats), shared by the HIP kernels and by any CPU checker that wants to reproduce their results bit for bit.
 *
 * Squared distance of a query q to a target t, all float32:
 *
 *     d* = t.* - q.*                          (one rounding each)
 *     d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))  (three roundings)
 *
 * the expression sls_knn.hip has always used.  d2 >= +0 (a sum of squares never gives -0), so its bit pattern grows
 * with its value and the pair (d2, target index) orders as ONE unsigned 64-bit key, bits(d2) in the high word: the
 * minimum of the keys is the nearest target, the lowest index among equal distances.
 *
 * Where the coordinates are multiples of 1/16 of magnitude <= 64, every difference is a multiple of 1/16, at most 2^11
 * sixteenths and every square and sum an integer count of 1/256 below 2^24: all of it exact, d2 equals the float64 value.
 *
 * sls_nn_stats: an entry is KEPT when d2 < truncation * truncation (one float32 product); a kept entry contributes
 * d = sqrtf(d2) (correctly rounded), any other one contributes d = truncation or nothing; d counts as "below" when
 * d < threshold in float32; the sum adds (double)d.
 *
 * Rules for users of this header: the fmaf calls are explicit, so the contraction setting does not matter; no
 * fast-math; HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_NN_MATH_H
#define SLS_NN_MATH_H

#include <math.h>
#include <stdint.h>

#ifndef SLS_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define SLS_HD __host__ __device__ __forceinline__
#else
#define SLS_HD static inline
#endif
#endif

SLS_HD float sls_nn_dist2(float qx, float qy, float qz, float tx, float ty, float tz)
{
    const float dx = tx - qx, dy = ty - qy, dz = tz - qz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

SLS_HD uint32_t sls_nn_float_bits(float f)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    return bits;
}

SLS_HD float sls_nn_bits_float(uint32_t bits)
{
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

/* (d2, index) as one key: smaller key = nearer, then lower index. */
SLS_HD uint64_t sls_nn_key(float d2, uint32_t index)
{
    return ((uint64_t)sls_nn_float_bits(d2) << 32) | (uint64_t)index;
}
SLS_HD float sls_nn_key_dist2(uint64_t key) { return sls_nn_bits_float((uint32_t)(key >> 32)); }
SLS_HD uint32_t sls_nn_key_index(uint64_t key) { return (uint32_t)(key & 0xFFFFFFFFu); }

/* The key no target beats: +inf, index 0xFFFFFFFF. */
#define SLS_NN_KEY_NONE 0x7F800000FFFFFFFFull

/* sls_nn_stats, one entry: returns 1 and the contribution *d when the entry contributes, 0 otherwise. */
SLS_HD int sls_nn_stats_term(float d2, float truncation, int include_truncated, float *d)
{
    const float tau2 = truncation * truncation;
    if (d2 < tau2) { *d = sqrtf(d2); return 1; }
    *d = truncation;
    return include_truncated != 0;
}

#endif /* SLS_NN_MATH_H */
