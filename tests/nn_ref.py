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


def stats(dist2, truncation, threshold, include_truncated):
    """(n, n_below, float64 sum, M) as sls_nn_stats defines them: float32 comparisons and roots, a float64 sum."""
    d2 = np.asarray(dist2, np.float32)
    tau = np.float32(truncation)
    tau2 = np.float32(tau * tau)
    kept = d2 < tau2
    with np.errstate(invalid="ignore"):
        d = np.where(kept, np.sqrt(np.where(kept, d2, np.float32(0))), tau).astype(np.float32)
    if not include_truncated:
        d = d[kept]
    return int(d.size), int((d < np.float32(threshold)).sum()), float(d.astype(np.float64).sum()), int(d2.size)


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
