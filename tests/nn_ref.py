"""NumPy restatement of the two-cloud nearest-neighbour query and of the cloud metrics (splat_loam_amd/evaluation.py,
sls_nn_query / sls_nn_stats): float64 brute force in chunks, np.argmin for the lowest index among equal distances, and
the metric block of the reference's evaluate_recon (utils/eval_utils.py:122-153).

On inputs whose coordinates are multiples of 1/16 with magnitude <= 64 every difference, square and sum of the
kernel's float32 expression is exact (include/sls_nn_math.h), so the float64 values here, rounded to float32, ARE the
kernel's bits: no emulation of fmaf is needed.
"""
from __future__ import annotations

import numpy as np


def dist2_matrix(query, target):
    """(len(query), len(target)) float64 squared distances of the float32 inputs."""
    q = np.asarray(query, np.float32).astype(np.float64)
    t = np.asarray(target, np.float32).astype(np.float64)
    out = np.square(t[None, :, 0] - q[:, None, 0])
    for k in (1, 2):
        d = t[None, :, k] - q[:, None, k]
        d *= d
        out += d
    return out


def nearest(target, query, chunk=512):
    """(dist2 float64 (Mq,), index int32 (Mq,)): the minimum and the LOWEST target index attaining it."""
    query = np.asarray(query, np.float32).reshape(-1, 3)
    target = np.asarray(target, np.float32).reshape(-1, 3)
    if len(target) == 0:
        raise ValueError("the target cloud is empty")
    dist2 = np.empty(len(query), np.float64)
    index = np.empty(len(query), np.int32)
    step = max(1, min(chunk, (1 << 22) // max(len(target), 1)))
    for a in range(0, len(query), step):
        d = dist2_matrix(query[a:a + step], target)
        i = np.argmin(d, axis=1)                    # first occurrence = lowest index
        index[a:a + step] = i
        dist2[a:a + step] = d[np.arange(len(i)), i]
    return dist2, index


def _stats_terms(dist2, truncation, include_truncated):
    """(d float32 (M,), counted bool (M,)): every entry's term and whether sls_nn_stats counts it"""
    d2 = np.asarray(dist2, np.float32)
    tau = np.float32(truncation)
    tau2 = np.float32(tau * tau)
    kept = d2 < tau2
    with np.errstate(invalid="ignore"):
        d = np.where(kept, np.sqrt(np.where(kept, d2, np.float32(0))), tau).astype(np.float32)
    return d, (np.ones_like(kept) if include_truncated else kept)


def stats(dist2, truncation, threshold, include_truncated):
    """(n, n_below, float64 sum, M) as sls_nn_stats defines them: float32 comparisons and roots, a float64 sum (in NumPy's
    order, not the device's: stats_device_order)."""
    d, counted = _stats_terms(dist2, truncation, include_truncated)
    d = d[counted]
    return int(d.size), int((d < np.float32(threshold)).sum()), float(d.astype(np.float64).sum()), int(counted.size)


STATS_THREADS, STATS_MAX_BLOCKS = 256, 1024     # a block's threads; SLS_NN_STATS_SCRATCH_BYTES / 32 bytes a partial


BUTTERFLY, WAVES = (32, 16, 8, 4, 2, 1), (0, 1, 2, 3)      # the device's order; the tests perturb them to show they matter


def _block_sum(v, butterfly=BUTTERFLY, waves=WAVES):
    """(..., 256) float64 -> (...): what thread 0 of a block holds — the 64 lanes of each wave by v[l] += v[l ^ off] for
    off = 32 .. 1, then the waves 0 .. 3 in order"""
    w = v.reshape(v.shape[:-1] + (STATS_THREADS // 64, 64))
    lanes = np.arange(64)
    for off in butterfly:
        w = w + w[..., lanes ^ off]
    s = w[..., waves[0], 0]
    for k in waves[1:]:
        s = s + w[..., k, 0]
    return s


def _strided_sum(v, lanes):
    """(n,) float64 -> (lanes,): entry l sums v[l], v[l + lanes], ... one after the other from 0.0"""
    rounds = -(-len(v) // lanes)
    v = np.concatenate([v, np.zeros(rounds * lanes - len(v))]).reshape(rounds, lanes)
    acc = np.zeros(lanes)
    for r in range(rounds):
        acc = acc + v[r]
    return acc


def device_sum(values, butterfly=BUTTERFLY, waves=WAVES):
    """The float64 sum of sls_nn_stats and sls_signed_stats in the DEVICE's order, the contract of their word 2:
    blocks = min(ceil(M / 256), 1024); thread t of block b adds its terms b * 256 + t, + blocks * 256, ... one after the
    other from 0.0; the block's 256 sums by _block_sum; one block then treats the partials the same way, thread t adding
    the partials t, t + 256, ...  `values`: float64 (M,), 0.0 where the entry is not counted — a thread skips such an
    entry, and adding +0.0 changes no bit of a sum that starts at +0.0 (such a sum is never -0.0)."""
    values = np.asarray(values, np.float64)
    blocks = min(-(-len(values) // STATS_THREADS), STATS_MAX_BLOCKS)
    if blocks == 0:
        return 0.0
    partials = _block_sum(_strided_sum(values, blocks * STATS_THREADS).reshape(blocks, STATS_THREADS), butterfly, waves)
    return float(_block_sum(_strided_sum(partials, STATS_THREADS), butterfly, waves))


STATS_ORDER_SIZES = (1, 65, 257, 1000, 262145 + 18655)     # the last: 1024 blocks whose threads stride, four partials a thread
# Seeds (distances, signed) of the data below.  Sums of float32 terms in float64 are so accurate that two orders often
# end on the same double whatever the data: these seeds are the first at which the documented order differs from NumPy's,
# from a left-to-right sum, from the butterfly run upwards and (from three waves on) from the waves added 3 .. 0 — found
# with device_sum alone, on the CPU, and asserted by tests/test_nn_host.py::test_order_tests_data_tells_orders_apart.
STATS_ORDER_SEEDS = {1: (0, 0), 65: (19, 3), 257: (229, 2), 1000: (224, 28), 262145 + 18655: (42, 2)}


def stats_order_dist2(M):
    """float32 squared distances for the tests of the ORDER: log-uniform over 36 decades (their roots, the terms, over 18),
    all below the truncation 0.5, and every seventh entry beyond it (0.5 each with include_truncated).  A float32 term
    more than 2^29 times smaller than the float64 sum it joins is rounded, so with terms this far apart most additions
    round and another order can give other bits (STATS_ORDER_SEEDS: does)."""
    rng = np.random.default_rng(STATS_ORDER_SEEDS[M][0])
    d2 = (10.0 ** rng.uniform(-37.0, -0.7, M)).astype(np.float32)
    d2[5::7] = np.float32(1.0)
    d2[0] = np.float32(0.0625)                      # (M = 1: an entry that counts either way)
    return d2


def stats_order_signed(M):
    """float32 signed distances for the same purpose: magnitudes log-uniform over 1e-30 .. 0.4, 85 % negative (so that the
    sum is a good part of the sum of magnitudes: well conditioned), every 97th entry beyond the truncation 0.5"""
    rng = np.random.default_rng(STATS_ORDER_SEEDS[M][1])
    sd = (np.where(rng.uniform(0, 1, M) < 0.85, -1.0, 1.0) * 10.0 ** rng.uniform(-30.0, -0.4, M)).astype(np.float32)
    sd[3::97] = np.float32(0.75)
    sd[0] = np.float32(-0.25)
    return sd


def stats_device_order(dist2, truncation, threshold, include_truncated):
    """stats with the sum in the device's order: all four words of sls_nn_stats, bit for bit"""
    d, counted = _stats_terms(dist2, truncation, include_truncated)
    n, below, _, M = stats(dist2, truncation, threshold, include_truncated)
    return n, below, device_sum(np.where(counted, d.astype(np.float64), 0.0)), M


def cloud_metrics(reference, estimate, threshold=0.2, truncation_acc=0.5, truncation_com=0.5):
    """The metric block for two point clouds, keys as evaluation.cloud_metrics.  The squared distances are rounded to
    float32 first, as the device's are (exact on lattice inputs)."""
    d_acc = nearest(reference, estimate)[0].astype(np.float32)
    d_com = nearest(estimate, reference)[0].astype(np.float32)
    n_acc, below_acc, sum_acc, _ = stats(d_acc, truncation_acc, threshold, False)
    n_com, below_com, sum_com, _ = stats(d_com, truncation_com, threshold, True)
    accuracy = sum_acc / n_acc if n_acc else float("nan")
    precision = below_acc / n_acc if n_acc else float("nan")
    completeness, recall = sum_com / n_com, below_com / n_com
    pr = precision + recall
    return {
        "accuracy_m": accuracy, "completeness_m": completeness, "chamfer_l1_m": 0.5 * (accuracy + completeness),
        "precision": precision, "recall": recall, "fscore": 2.0 * precision * recall / pr if pr != 0 else 0.0,
        "n_accuracy": n_acc, "n_completeness": n_com,
        "threshold": float(threshold), "truncation_acc": float(truncation_acc), "truncation_com": float(truncation_com),
    }


def crop_union_mask(reference, estimate, threshold_dist=1.2):
    d2 = nearest(estimate, reference)[0].astype(np.float32)
    t = np.float32(threshold_dist)
    return d2 < np.float32(t * t)
