/*
 * sls_ground_math.h — the rule of the ground segmentation of a LiDAR scan (sls_ground_segment), shared by the HIP kernels,
 * by a host program and by the NumPy restatement (tests/ground_ref.py), which reproduce the kernels' results bit for bit.
 *
 * WHAT THIS IS: a region-wise ground-plane fit in the manner of Patchwork (Lim, Oh, Myung: "Patchwork: Concentric Zone-based
 * Region-wise Ground Segmentation with Ground Likelihood Estimation Using a 3D LiDAR Sensor", RA-L 2021) — a concentric zone
 * model, seeds from the lowest points of every bin, an iterated PCA plane fit, uprightness / elevation / flatness tests per
 * bin — RESTATED FROM THE PAPER so that device and host agree bit for bit.  Neither patchwork nor patchwork++ nor
 * pypatchworkpp is a dependency or was at hand: nothing here was compared with either implementation and no parity with them
 * is claimed.  The default parameters are a judgement recalled from the paper's public defaults, not verified; they are
 * parameters.  Not here: Patchwork++'s reflected-noise removal, region-wise vertical plane fitting, adaptive thresholds,
 * temporal ground revert, and sensor-height estimation.
 *
 * THE RULE that makes bit equality possible: + - * / sqrt and floor alone, every sum in one fixed order, no implicit fma
 * (-ffp-contract=off), and NO atan2 — device and host libm differ — so sectors are cut in the diamond angle.
 *
 * Bins.  A point p = (x, y, z), float32, sensor frame, z up; all of the following in float64:
 *   rho = sqrt(x*x + y*y).  A point with a non-finite coordinate, or rho < min_range, or rho >= max_range, or
 *   |x| + |y| == 0 has no bin.
 *   Zone boundaries (Patchwork's CZM, from the two ranges): r0 = min, r1 = (7 min + max) / 8, r2 = (3 min + max) / 4,
 *   r3 = (min + max) / 2, r4 = max.  Zone z holds r_z <= rho < r_{z+1}; rings per zone R = {2, 4, 4, 4}, sectors per zone
 *   S = {16, 32, 54, 32}: 32 + 128 + 216 + 128 = SLS_GROUND_BINS = 504 bins.
 *   ring = min(floor((rho - r_z) / ((r_{z+1} - r_z) / R_z)), R_z - 1).
 *   Diamond angle: a = y / (|x| + |y|); if x < 0, a = 2 - a; else if y < 0, a = 4 + a.  Monotone in the true azimuth, in
 *   [0, 4] (4 itself only by rounding).  sector = min(floor(a * (S_z / 4.0)), S_z - 1).  Sectors are therefore equal in
 *   diamond angle, NOT in azimuth: their widths in azimuth differ by up to about 2x (narrowest on the diagonals, widest on
 *   the axes), which is harmless for a per-bin plane fit.
 *   bin = base_z + ring * S_z + sector, base = {0, 32, 160, 376}.  The concentric index c of a bin is its ring counted over
 *   all zones, 0 ... 13.
 *
 * Order inside a bin: ascending by the ordered word of z (sls_ground_ord: the f2ord mapping of the device code, so -0.0
 * comes before +0.0), ties by the original row index.  One 64-bit key: bin << 32 | ord(z); bin SLS_GROUND_BINS = "no bin".
 * The bin's n points in that order are its ENTRIES 0 ... n - 1.
 *
 * Per bin (Patchwork's R-GPF + GLE):
 *   1. n == 0: EMPTY.  n < num_min_pts: FEW.  Nothing is ground.
 *   2. Noise skip, zone 0 only: skip = the number of leading entries with (double)z < -((double)noise_margin *
 *      (double)sensor_height) (the bin is sorted, so they lead); 0 in the other zones.
 *   3. lpr = the float64 mean of z over the first min(num_lpr, n - skip) entries from `skip` on, summed one after the
 *      other in order.  (n == skip: no seeds.)
 *   4. Seeds: the entries e >= skip with (double)z < lpr + (double)th_seeds — a contiguous run, the bin being sorted.
 *   5. Plane fit of a set of m members:
 *        sums by 64 LANES: lane l takes the set's members among the entries l, l + 64, ... in ascending order, starting
 *        from +0.0, a non-member skipped; the 64 partial sums are added by the xor butterfly with offsets 32, 16, ..., 1
 *        (a + b == b + a: every lane ends with the same bits).  At EVERY size: there is no separate short-row rule.
 *        mean = the three coordinate sums / m;  C = the six sums of products of ((double)p - mean), xx xy xz yy yz zz, / m
 *        (the formulas of sls_normals_covariance);  sls_normals_jacobi on C;
 *        normal = the column under the smallest diagonal entry (ties to the lowest index), normalised in float64, flipped
 *        if nz < 0;  d = -(nx*mx + ny*my + nz*mz);  eigenvalues = the diagonal, ascending.
 *        m < 3, or (l0 + l1) + l2 not above 0: DEGENERATE, nothing is ground, the fit stops.
 *   6. Fit the seeds; then num_iter times: the set becomes EVERY entry of the bin (the skipped ones too) with
 *      nx*x + ny*y + nz*z + d < (double)th_dist (float64, summed left to right), and is fitted again.  After the last
 *      round that set is the candidate ground — membership is judged by the plane of the round BEFORE the last fit — and
 *      the last fit's plane, mean and eigenvalues are the bin's.
 *   7. nz < uprightness_thr: NOT_UPRIGHT.  Otherwise, if c < 4 and mean_z > -sensor_height + elevation_thr[c]: GROUND if
 *      l0 / ((l0 + l1) + l2) < flatness_thr[c], else ELEVATED_ROUGH.  Otherwise GROUND.  Only in state GROUND are the
 *      candidates labelled ground.
 *
 * Record of a bin: plane[8] = nx, ny, nz, d, mean_z, l0, l1, l2 (float64; zeros in EMPTY, FEW and DEGENERATE) and
 * info[4] = n, seeds, candidates (the members of the last set that was counted), state.
 *
 * Rules for users of this header: no fast-math, -ffp-contract=off, coordinates of a point with a bin are finite by the bin
 * rule.  Plain C99 / HIP device compatible; on the device sls_ground_fit is called by all 64 lanes of a wave together.
 */
#ifndef SLS_GROUND_MATH_H
#define SLS_GROUND_MATH_H

#include <stddef.h>

#include "sls_normals_math.h"

#define SLS_GROUND_BINS 504     /* (include/sls_abi.h defines the same) */
#define SLS_GROUND_LANES 64

#ifndef SLS_GROUND_PARAMS_DEFINED
#define SLS_GROUND_PARAMS_DEFINED
typedef struct SlsGroundParams {    /* (include/sls_abi.h defines the same) */
    float sensor_height, min_range, max_range, th_seeds, th_dist, uprightness_thr, noise_margin, elevation_thr[4],
        flatness_thr[4];
    int32_t num_lpr, num_iter, num_min_pts;
} SlsGroundParams;
#endif

enum { SLS_GROUND_EMPTY = 0, SLS_GROUND_FEW = 1, SLS_GROUND_DEGENERATE = 2, SLS_GROUND_NOT_UPRIGHT = 3,
       SLS_GROUND_ELEVATED_ROUGH = 4, SLS_GROUND_GROUND = 5 };

/* the defaults (a judgement: see above) */
SLS_HD void sls_ground_defaults(SlsGroundParams *p)
{
    p->sensor_height = 1.723f; p->min_range = 2.7f; p->max_range = 80.0f; p->th_seeds = 0.5f; p->th_dist = 0.125f;
    p->uprightness_thr = 0.707f; p->noise_margin = 1.1f;
    p->elevation_thr[0] = 0.523f; p->elevation_thr[1] = 0.746f; p->elevation_thr[2] = 0.879f; p->elevation_thr[3] = 1.125f;
    p->flatness_thr[0] = 5.0e-4f; p->flatness_thr[1] = 7.25e-4f; p->flatness_thr[2] = 1.0e-3f; p->flatness_thr[3] = 1.0e-3f;
    p->num_lpr = 20; p->num_iter = 3; p->num_min_pts = 10;
}

SLS_HD int sls_ground_finite(float v) { return v - v == 0.0f; }     /* (inf - inf and NaN - NaN are NaN) */

/* the monotone float -> uint mapping of the device code's f2ord */
SLS_HD uint32_t sls_ground_ord(float z)
{
    const uint32_t u = sls_nn_float_bits(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

/* the bin of a point, or -1 */
SLS_HD int sls_ground_bin(float x, float y, float z, const SlsGroundParams *p)
{
    if (!(sls_ground_finite(x) && sls_ground_finite(y) && sls_ground_finite(z))) return -1;
    const double dx = (double)x, dy = (double)y, mn = (double)p->min_range, mx = (double)p->max_range;
    const double rho = sqrt(dx * dx + dy * dy);
    const double ax = dx < 0.0 ? -dx : dx, ay = dy < 0.0 ? -dy : dy, l1 = ax + ay;
    if (rho < mn || rho >= mx || l1 == 0.0) return -1;
    const double r1 = (7.0 * mn + mx) / 8.0, r2 = (3.0 * mn + mx) / 4.0, r3 = (mn + mx) / 2.0;
    double lo, hi, rings, sectors;
    int base, nr, ns;
    if (rho < r1)      { lo = mn; hi = r1; rings = 2.0; sectors = 16.0; base = 0;   nr = 2; ns = 16; }
    else if (rho < r2) { lo = r1; hi = r2; rings = 4.0; sectors = 32.0; base = 32;  nr = 4; ns = 32; }
    else if (rho < r3) { lo = r2; hi = r3; rings = 4.0; sectors = 54.0; base = 160; nr = 4; ns = 54; }
    else               { lo = r3; hi = mx; rings = 4.0; sectors = 32.0; base = 376; nr = 4; ns = 32; }
    int ring = (int)floor((rho - lo) / ((hi - lo) / rings));
    if (ring > nr - 1) ring = nr - 1;
    double a = dy / l1;
    if (dx < 0.0) a = 2.0 - a;
    else if (dy < 0.0) a = 4.0 + a;
    int sector = (int)floor(a * (sectors / 4.0));
    if (sector > ns - 1) sector = ns - 1;
    return base + ring * ns + sector;
}

SLS_HD uint64_t sls_ground_key(int bin, float z)
{
    return ((uint64_t)(uint32_t)(bin < 0 ? SLS_GROUND_BINS : bin) << 32) | (uint64_t)sls_ground_ord(z);
}

/* zone and concentric index of a bin in [0, SLS_GROUND_BINS) */
SLS_HD void sls_ground_bin_place(int bin, int *zone, int *concentric)
{
    if (bin < 32)       { *zone = 0; *concentric = bin / 16; }
    else if (bin < 160) { *zone = 1; *concentric = 2 + (bin - 32) / 32; }
    else if (bin < 376) { *zone = 2; *concentric = 6 + (bin - 160) / 54; }
    else                { *zone = 3; *concentric = 10 + (bin - 376) / 32; }
}

/* A bin's entries: rows of four floats, x y z and the original row index as bits, in the bin's order. */
#if defined(__HIPCC__) || defined(__HIP__)
#define SLS_GROUND_ROW(rows4, e, x, y, z) \
    do { const float4 r_ = ((const float4 *)(rows4))[e]; x = r_.x; y = r_.y; z = r_.z; } while (0)
#define SLS_GROUND_UNROLL _Pragma("unroll 4")       /* four rows' loads in flight; the sums keep their order */
#else
#define SLS_GROUND_UNROLL
#define SLS_GROUND_ROW(rows4, e, x, y, z) \
    do { const float *r_ = (rows4) + 4 * (size_t)(e); x = r_[0]; y = r_[1]; z = r_[2]; } while (0)
#endif

SLS_HD float sls_ground_z(const float *rows4, int e) { return rows4[4 * (size_t)e + 2]; }

/* A set of entries: the seeds (plane == 0: e >= from and z below zthr) or the points near a plane (plane == 1). */
typedef struct SlsGroundSet {
    int plane, from;
    double zthr, nx, ny, nz, d, th;
} SlsGroundSet;

SLS_HD int sls_ground_member(const SlsGroundSet *s, int e, float x, float y, float z)
{
    if (s->plane) return s->nx * (double)x + s->ny * (double)y + s->nz * (double)z + s->d < s->th;
    return e >= s->from && (double)z < s->zthr;
}

/* lane l's share of the set: its count and its three coordinate sums */
SLS_HD int sls_ground_lane_sums(const float *rows4, int n, int lane, const SlsGroundSet *s, double *sum3)
{
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int m = 0;
    SLS_GROUND_UNROLL
    for (int e = lane; e < n; e += SLS_GROUND_LANES) {
        float x, y, z;
        SLS_GROUND_ROW(rows4, e, x, y, z);
        /* (a member adds, a non-member keeps the sum: selects, so that the loop has no branch and its loads run ahead) */
        const int in = sls_ground_member(s, e, x, y, z);
        sx = in ? sx + (double)x : sx; sy = in ? sy + (double)y : sy; sz = in ? sz + (double)z : sz;
        m += in;
    }
    sum3[0] = sx; sum3[1] = sy; sum3[2] = sz;
    return m;
}

/* lane l's share of the six sums about the mean (the membership test is made again: nothing is stored per entry) */
SLS_HD void sls_ground_lane_cov(const float *rows4, int n, int lane, const SlsGroundSet *s, const double *mean3, double *cov6)
{
    const double mx = mean3[0], my = mean3[1], mz = mean3[2];
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    SLS_GROUND_UNROLL
    for (int e = lane; e < n; e += SLS_GROUND_LANES) {
        float x, y, z;
        SLS_GROUND_ROW(rows4, e, x, y, z);
        const int in = sls_ground_member(s, e, x, y, z);
        const double dx = (double)x - mx, dy = (double)y - my, dz = (double)z - mz;
        xx = in ? xx + dx * dx : xx; xy = in ? xy + dx * dy : xy; xz = in ? xz + dx * dz : xz;
        yy = in ? yy + dy * dy : yy; yz = in ? yz + dy * dz : yz; zz = in ? zz + dz * dz : zz;
    }
    cov6[0] = xx; cov6[1] = xy; cov6[2] = xz; cov6[3] = yy; cov6[4] = yz; cov6[5] = zz;
}

/* The sums of a set over all 64 lanes.  Device: this lane's share, then the xor butterfly (offsets 32 ... 1) — every lane
 * of the wave calls it and gets the same bits.  Host: the 64 shares one after the other, then the tree that gives lane 0
 * of the butterfly its value: lane 0 adds lane 32's, then lane 16's (which has added lane 48's), ... */
#if defined(__HIP_DEVICE_COMPILE__)
SLS_HD int sls_ground_set_sums(const float *rows4, int n, int lane, const SlsGroundSet *s, double *sum3)
{
    int m = sls_ground_lane_sums(rows4, n, lane, s, sum3);
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; ++k) sum3[k] += __shfl_xor(sum3[k], off, 64);
        m += __shfl_xor(m, off, 64);
    }
    return m;
}
SLS_HD void sls_ground_set_cov(const float *rows4, int n, int lane, const SlsGroundSet *s, const double *mean3, double *cov6)
{
    sls_ground_lane_cov(rows4, n, lane, s, mean3, cov6);
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 6; ++k) cov6[k] += __shfl_xor(cov6[k], off, 64);
}
#else
SLS_HD void sls_ground_tree(double part[SLS_GROUND_LANES][6], int width, double *out)
{
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l)
            for (int k = 0; k < width; ++k) part[l][k] += part[l + off][k];
    for (int k = 0; k < width; ++k) out[k] = part[0][k];
}
SLS_HD int sls_ground_set_sums(const float *rows4, int n, int lane, const SlsGroundSet *s, double *sum3)
{
    double part[SLS_GROUND_LANES][6];
    int m = 0;
    (void)lane;
    for (int l = 0; l < SLS_GROUND_LANES; ++l) m += sls_ground_lane_sums(rows4, n, l, s, part[l]);
    sls_ground_tree(part, 3, sum3);
    return m;
}
SLS_HD void sls_ground_set_cov(const float *rows4, int n, int lane, const SlsGroundSet *s, const double *mean3, double *cov6)
{
    double part[SLS_GROUND_LANES][6];
    (void)lane;
    for (int l = 0; l < SLS_GROUND_LANES; ++l) sls_ground_lane_cov(rows4, n, l, s, mean3, part[l]);
    sls_ground_tree(part, 6, cov6);
}
#endif

/* Step 5: the plane of a set.  plane8: nx ny nz d mean_z l0 l1 l2.  Returns the member count m; *ok = 0: degenerate. */
SLS_HD int sls_ground_fit_set(const float *rows4, int n, int lane, const SlsGroundSet *s, double *plane8, int *ok)
{
    double sum[3], mean[3], cov[6], dg[3], v[9];
    const int m = sls_ground_set_sums(rows4, n, lane, s, sum);
    *ok = 0;
    if (m < 3) return m;
    const double dm = (double)m;
    mean[0] = sum[0] / dm; mean[1] = sum[1] / dm; mean[2] = sum[2] / dm;
    sls_ground_set_cov(rows4, n, lane, s, mean, cov);
    for (int k = 0; k < 6; ++k) cov[k] = cov[k] / dm;
    sls_normals_jacobi(cov, dg, v);
    /* (every element is read before one is chosen: a choice between scalars, not between addresses) */
    const double d0 = dg[0], d1 = dg[1], d2 = dg[2];
    const double v00 = v[0], v01 = v[1], v02 = v[2], v10 = v[3], v11 = v[4], v12 = v[5], v20 = v[6], v21 = v[7], v22 = v[8];
    double lo = d0, nx = v00, ny = v10, nz = v20;
    if (d1 < lo) { lo = d1; nx = v01; ny = v11; nz = v21; }
    if (d2 < lo) { lo = d2; nx = v02; ny = v12; nz = v22; }
    double e0 = d0, e1 = d1, e2 = d2, sw;
    if (e1 < e0) { sw = e0; e0 = e1; e1 = sw; }
    if (e2 < e1) { sw = e1; e1 = e2; e2 = sw; }
    if (e1 < e0) { sw = e0; e0 = e1; e1 = sw; }
    if (!((e0 + e1) + e2 > 0.0)) return m;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    nx = nx / len; ny = ny / len; nz = nz / len;
    if (nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    plane8[0] = nx; plane8[1] = ny; plane8[2] = nz;
    plane8[3] = -(nx * mean[0] + ny * mean[1] + nz * mean[2]);
    plane8[4] = mean[2]; plane8[5] = e0; plane8[6] = e1; plane8[7] = e2;
    *ok = 1;
    return m;
}

/* Step 7 */
SLS_HD int sls_ground_classify(const double *plane8, int concentric, const SlsGroundParams *p)
{
    if (plane8[2] < (double)p->uprightness_thr) return SLS_GROUND_NOT_UPRIGHT;
    if (concentric < 4 && plane8[4] > -(double)p->sensor_height + (double)p->elevation_thr[concentric]) {
        const double flat = plane8[5] / ((plane8[5] + plane8[6]) + plane8[7]);
        return flat < (double)p->flatness_thr[concentric] ? SLS_GROUND_GROUND : SLS_GROUND_ELEVATED_ROUGH;
    }
    return SLS_GROUND_GROUND;
}

/* A bin whole (steps 1 - 7): its n entries, its number -> plane8, info4 and the set whose members are the candidates
 * (labelled ground iff info4[3] == SLS_GROUND_GROUND).  Device: called by the 64 lanes of a wave with the same arguments
 * but `lane`; every lane returns the same values. */
SLS_HD void sls_ground_fit(const float *rows4, int n, int bin, int lane, const SlsGroundParams *p, double *plane8,
                           int32_t *info4, SlsGroundSet *set)
{
    int zone, c, ok;
    sls_ground_bin_place(bin, &zone, &c);
    for (int k = 0; k < 8; ++k) plane8[k] = 0.0;
    info4[0] = n; info4[1] = 0; info4[2] = 0;
    set->plane = 0; set->from = 0; set->zthr = 0.0; set->nx = 0.0; set->ny = 0.0; set->nz = 0.0; set->d = 0.0;
    set->th = (double)p->th_dist;
    if (n < p->num_min_pts || n == 0) { info4[3] = n == 0 ? SLS_GROUND_EMPTY : SLS_GROUND_FEW; return; }
    /* 2: the noise skip.  The bin ascends in z, so the entries below the limit lead and their number is the first position
     * that is not below it: a bisection, about log2(n) reads, which every lane of a wave makes alike. */
    int skip = 0;
    if (zone == 0) {
        const double limit = -((double)p->noise_margin * (double)p->sensor_height);
        int hi = n;
        while (skip < hi) {
            const int mid = skip + ((hi - skip) >> 1);
            if ((double)sls_ground_z(rows4, mid) < limit) skip = mid + 1; else hi = mid;
        }
    }
    /* 3: the lowest point representative: min(num_lpr, n - skip) dependent reads and adds, one after the other as the rule
     * demands, and on the device by every lane alike — the one part of a bin's work that 64 lanes do not share; a num_lpr
     * in the thousands makes it the bin's cost */
    const int n_lpr = n - skip < p->num_lpr ? n - skip : p->num_lpr;
    double zsum = 0.0;
    for (int j = 0; j < n_lpr; ++j) zsum += (double)sls_ground_z(rows4, skip + j);
    /* 4 - 6 */
    double fit[8];
    int m = 0;
    ok = 0;
    if (n_lpr > 0) {
        set->from = skip;
        set->zthr = zsum / (double)n_lpr + (double)p->th_seeds;
        m = sls_ground_fit_set(rows4, n, lane, set, fit, &ok);
        info4[1] = m;
    }
    for (int it = 0; ok && it < p->num_iter; ++it) {
        set->plane = 1; set->nx = fit[0]; set->ny = fit[1]; set->nz = fit[2]; set->d = fit[3];
        m = sls_ground_fit_set(rows4, n, lane, set, fit, &ok);
    }
    info4[2] = m;
    if (!ok) { info4[3] = SLS_GROUND_DEGENERATE; return; }
    for (int k = 0; k < 8; ++k) plane8[k] = fit[k];
    info4[3] = sls_ground_classify(plane8, c, p);
}

/* ---- the whole cloud on the host, serially: the 64 lanes emulated (the host test, tools/ground_bench.py) -------------- */
#if !defined(__HIPCC__) && !defined(__HIP__)
#include <stdlib.h>

typedef struct SlsGroundItem { uint64_t key; uint32_t row; } SlsGroundItem;

static int sls_ground_item_cmp(const void *a, const void *b)
{
    const SlsGroundItem *p = (const SlsGroundItem *)a, *q = (const SlsGroundItem *)b;
    if (p->key != q->key) return p->key < q->key ? -1 : 1;
    return p->row < q->row ? -1 : (p->row > q->row ? 1 : 0);
}

/* out_label [M], out_bin [M] (-1: none), out_planes [BINS x 8], out_info [BINS x 4], out_status [8] as sls_ground_segment
 * writes them.  Returns 0, or 1 when memory is short. */
static int sls_ground_segment_host(int M, const float *xyz, const SlsGroundParams *p, uint8_t *out_label, int32_t *out_bin,
                                   double *out_planes, int32_t *out_info, uint32_t *out_status)
{
    for (int k = 0; k < 8; ++k) out_status[k] = 0u;
    out_status[7] = 1u;
    if (M <= 0) return 0;
    SlsGroundItem *items = (SlsGroundItem *)malloc(sizeof(SlsGroundItem) * (size_t)M);
    float *rows4 = (float *)malloc(16 * (size_t)M);
    if (!items || !rows4) { free(items); free(rows4); return 1; }
    for (int i = 0; i < M; ++i) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        const int bin = sls_ground_bin(x, y, z, p);
        if (!(sls_ground_finite(x) && sls_ground_finite(y) && sls_ground_finite(z))) out_status[2] += 1u;
        items[i].key = sls_ground_key(bin, z);
        items[i].row = (uint32_t)i;
        out_label[i] = 0;
        out_bin[i] = bin;
    }
    qsort(items, (size_t)M, sizeof(SlsGroundItem), sls_ground_item_cmp);
    for (int q = 0; q < M; ++q) {
        const size_t i = items[q].row;
        rows4[4 * (size_t)q] = xyz[3 * i]; rows4[4 * (size_t)q + 1] = xyz[3 * i + 1]; rows4[4 * (size_t)q + 2] = xyz[3 * i + 2];
        rows4[4 * (size_t)q + 3] = sls_nn_bits_float((uint32_t)i);
    }
    int lo = 0;
    for (int bin = 0; bin < SLS_GROUND_BINS; ++bin) {
        int hi = lo;
        while (hi < M && (int)(items[hi].key >> 32) == bin) ++hi;
        SlsGroundSet set;
        sls_ground_fit(rows4 + 4 * (size_t)lo, hi - lo, bin, 0, p, out_planes + 8 * bin, out_info + 4 * bin, &set);
        out_status[0] += (uint32_t)(hi - lo);
        if (out_info[4 * bin + 3] == SLS_GROUND_GROUND) {
            out_status[3] += 1u;
            for (int e = 0; e < hi - lo; ++e) {
                const float *r = rows4 + 4 * (size_t)(lo + e);
                if (sls_ground_member(&set, e, r[0], r[1], r[2])) { out_label[items[lo + e].row] = 1; out_status[1] += 1u; }
            }
        }
        lo = hi;
    }
    free(items); free(rows4);
    return 0;
}
#endif

#endif /* SLS_GROUND_MATH_H */
