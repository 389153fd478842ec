"""NumPy restatement of the exact k-nearest-neighbour query and of the two outlier filters (include/sls_outlier_math.h,
sls_nn_query_k / sls_outlier_statistical / sls_outlier_radius, splat_loam_amd/evaluation.py): brute-force keys
(bits(d2) << 32) | index, sorted; the mean distance in float64 from float32 square roots, in list order; both keep rules.

Open3D is not installed where this project is developed: the statistical rule is Open3D's remove_statistical_outlier as
RESTATED in the header from its documented behaviour, and the device code is pinned against this file, not against Open3D.

As in nn_ref.py, on inputs whose coordinates are multiples of 1/16 with magnitude <= 64 the kernel's float32 squared
distance is exact, so the float64 brute force, rounded to float32, gives its bits.
"""
from __future__ import annotations

import numpy as np

import nn_ref

KEY_NONE = np.uint64(0x7F800000FFFFFFFF)


def keys_k(target, query, k, chunk=256):
    """(Mq, k) uint64: every query's min(k, Mt) smallest keys, ascending; SLS_NN_KEY_NONE in the slots beyond Mt."""
    target = np.asarray(target, np.float32).reshape(-1, 3)
    query = np.asarray(query, np.float32).reshape(-1, 3)
    Mt, Mq = len(target), len(query)
    out = np.full((Mq, k), KEY_NONE, np.uint64)
    n = min(k, Mt)
    idx = np.arange(Mt, dtype=np.uint64)[None, :]
    step = max(1, min(chunk, (1 << 21) // max(Mt, 1)))
    for a in range(0, Mq, step):
        d2 = nn_ref.dist2_matrix(query[a:a + step], target).astype(np.float32)
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
        if n < Mt:
            keys = np.partition(keys, n - 1, axis=1)[:, :n]
        out[a:a + step, :n] = np.sort(keys, axis=1)
    return out


def split(keys):
    """(dist2 float32, index int32) of a key array: +inf and -1 for SLS_NN_KEY_NONE."""
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return d2, index


def nearest_k(target, query, k):
    return split(keys_k(target, query, k))


def means(keys, Mt):
    """float64 (Mq,): (sum in list order of (double)sqrtf(d2_j)) / min(k, Mt)."""
    n = min(keys.shape[1], Mt)
    d = np.sqrt(split(keys[:, :n])[0]).astype(np.float64)     # float32 roots, correctly rounded
    total = np.zeros(len(keys), np.float64)
    for j in range(n):                                        # in list order
        total += d[:, j]
    return total / float(n)


def statistical(points, k, std_ratio):
    """dict(keep bool (M,), mean (M,), cloud_mean, std, thr, zero_mean, margin): the statistical rule on the self-query.
    margin = min_i |mean_i - thr| / thr: how far the nearest mean is from the threshold (NaN where thr is)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    M = len(points)
    mean = means(keys_k(points, points, k), M)
    counted = mean > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        cloud_mean = mean[counted].sum() / np.float64(M)
        std = np.sqrt(np.square(mean[counted] - cloud_mean).sum() / np.float64(M - 1))
        thr = cloud_mean + np.float64(std_ratio) * std
        keep = counted & (mean < thr)
        margin = float(np.abs(mean - thr).min() / thr) if M else float("nan")
    return {"keep": keep, "mean": mean, "cloud_mean": float(cloud_mean), "std": float(std), "thr": float(thr),
            "zero_mean": int((~counted).sum()), "margin": margin}


def radius(points, nb_points, radius_):
    """keep bool (M,): more than nb_points points, the point itself included, with d2 <= radius * radius (float32)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    keys = keys_k(points, points, nb_points + 1)
    r = np.float32(radius_)
    r2 = np.float32(r * r)
    rank = keys[:, nb_points]
    return (rank != KEY_NONE) & (split(rank)[0] <= r2)


def filter_cloud(M, seed):
    """The issue's test cloud: a thin slab on the 1/16 lattice, max(3, M // 25) far points, shuffled, row 5 a copy of row 9."""
    rng = np.random.default_rng(seed)
    n_far = max(3, M // 25)
    slab = rng.integers(-64, 65, (M - n_far, 3)) / 16.0
    slab[:, 2] = rng.integers(-2, 3, M - n_far) / 16.0
    far = rng.integers(-1024, 1025, (n_far, 3)) / 16.0
    pts = np.concatenate([slab, far]).astype(np.float32)
    pts = pts[rng.permutation(M)]
    pts[5] = pts[9]
    return pts
