/*
 * sls_draw_math.h — the arithmetic of the seeded densify draw (sls_densify_draw), shared by the HIP kernel and by any
 * CPU checker that wants to reproduce the drawn pixel set bit for bit.
 *
 * The draw is weighted sampling without replacement as an exponential race (Efraimidis–Spirakis): pixel p of
 * weight w > 0 gets the key E / w with E = -ln(u) a unit exponential variate, and the k smallest keys are drawn —
 * the distribution of torch.multinomial(w, k, replacement=False).  The variate is a pure function of
 * (pixel, seed, draw index):
 *
 *     r   = first output word of Philox4x32-10, counter (pixel, 0, draw_index, 0), key (seed low word, seed high word)
 *     u   = (2 (r >> 9) + 1) 2^-24            an odd 24-bit numerator: exact in float32, never 0 or 1
 *     E   = -ln(u)                           sls_draw_neg_log below
 *     key = E / w  (w > 0),  +inf  (w == 0)
 *
 * sls_draw_neg_log uses only what IEEE-754 rounds exactly (+ - * /, no fma) and integer operations on the bit
 * pattern, in a fixed order: u = 2^e m with m folded into [1/sqrt 2, sqrt 2), ln m = 2 t (1 + s/3 + s^2/5 + s^3/7 +
 * s^4/9), t = (m - 1) / (m + 1), s = t t (|t| <= 0.1716: the first dropped term is 2.0e-9 relative), and
 * E = (-e) ln2 - ln m with ln2 split in a 16-bit head (its product with |e| <= 24 is exact) and a tail.  For
 * u >= 1/sqrt 2 the exponent term vanishes, so E keeps its relative accuracy down to u = 1 - 2^-24 (E = 2^-24).
 * Relative error against float64 <= 1e-6 over all 2^23 values of u (measured: 2.1e-7), E > 0 everywhere:
 * tests/test_densify_draw_math.py.
 *
 * Rules for users of this header (both sides), as for sls_det_math.h: compile with -ffp-contract=off, no fast-math;
 * HIP: keep -fhip-fp32-correctly-rounded-divide-sqrt.  Plain C99 / HIP device compatible.
 */
#ifndef SLS_DRAW_MATH_H
#define SLS_DRAW_MATH_H

#include <stdint.h>

#ifndef SLS_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define SLS_HD __host__ __device__ __forceinline__
#else
#define SLS_HD static inline
#endif
#endif

#define SLS_PHILOX_M0 0xD2511F53u
#define SLS_PHILOX_M1 0xCD9E8D57u
#define SLS_PHILOX_W0 0x9E3779B9u
#define SLS_PHILOX_W1 0xBB67AE85u

/* Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ctr[4] <- the four output words. */
SLS_HD void sls_philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1)
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)SLS_PHILOX_M0 * (uint64_t)c0;
        const uint64_t p1 = (uint64_t)SLS_PHILOX_M1 * (uint64_t)c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += SLS_PHILOX_W0;
        k1 += SLS_PHILOX_W1;
    }
    ctr[0] = c0; ctr[1] = c1; ctr[2] = c2; ctr[3] = c3;
}

/* The draw's random word of a pixel. */
SLS_HD uint32_t sls_draw_word(uint32_t pixel, uint64_t seed, uint32_t draw_index)
{
    uint32_t c[4];
    c[0] = pixel; c[1] = 0u; c[2] = draw_index; c[3] = 0u;
    sls_philox4x32_10(c, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32));
    return c[0];
}

/* The surface sampler's random word of sample j of keyframe frame_id (sls_surface_samples; DESIGN.md section 2,
 * "Surface samples"): counter (j, 1, frame_id, 0) — the 1 keeps the stream disjoint from the densify draw's
 * (pixel, 0, draw_index, 0) under the same seed. */
SLS_HD uint32_t sls_sample_word(uint32_t sample, uint64_t seed, uint32_t frame_id)
{
    uint32_t c[4];
    c[0] = sample; c[1] = 1u; c[2] = frame_id; c[3] = 0u;
    sls_philox4x32_10(c, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32));
    return c[0];
}

/* A rank in [0, n) from a random word by multiply-shift: floor(r n / 2^32).  Uniform with replacement, as
 * np.random.choice(n, k) is, up to the multiply-shift bias: a rank is hit by floor(2^32 / n) or that + 1 words, so the
 * probabilities differ from 1 / n by at most n / 2^32 relative (<= 6.2e-5 at n = 2^18, the largest image served). */
SLS_HD uint32_t sls_sample_index(uint32_t r, uint32_t n)
{
    return (uint32_t)(((uint64_t)r * (uint64_t)n) >> 32);
}

SLS_HD float sls_draw_bits_float(uint32_t bits)
{
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

SLS_HD uint32_t sls_draw_float_bits(float f)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    return bits;
}

/* u in (0, 1): (2 (r >> 9) + 1) 2^-24 (the integer is below 2^24: its conversion and the scaling are exact). */
SLS_HD float sls_draw_uniform(uint32_t r)
{
    return (float)(2u * (r >> 9) + 1u) * 5.9604644775390625e-08f;
}

/* -ln(u) for u = sls_draw_uniform(r) (any normal float in (0, 1) works). */
SLS_HD float sls_draw_neg_log(float u)
{
    const uint32_t bits = sls_draw_float_bits(u);
    int e = (int)(bits >> 23) - 127;
    uint32_t frac = bits & 0x007FFFFFu;
    uint32_t mbits = frac | 0x3F800000u;                 /* m in [1, 2) */
    if (frac > 0x003504F3u) {                            /* m > sqrt 2 (0x3FB504F3): m / 2, exactly */
        mbits = frac | 0x3F000000u;
        e += 1;
    }
    const float m = sls_draw_bits_float(mbits);
    const float t = (m - 1.0f) / (m + 1.0f);
    const float s = t * t;
    float p = s * 0.111111111f;
    p = (p + 0.142857143f) * s;
    p = (p + 0.2f) * s;
    p = (p + 0.333333333f) * s;
    p = p + 1.0f;
    const float lnm = (t + t) * p;
    const float ne = (float)(-e);                        /* 0 .. 24 */
    return (ne * 0.693145751953125f - lnm) + ne * 1.42860682030941723e-06f;
}

/* The race key of a pixel of weight w (>= 0, finite) and random word r. */
SLS_HD float sls_draw_key(float w, uint32_t r)
{
    if (!(w > 0.0f)) return sls_draw_bits_float(0x7F800000u);
    return sls_draw_neg_log(sls_draw_uniform(r)) / w;
}

#endif /* SLS_DRAW_MATH_H */
