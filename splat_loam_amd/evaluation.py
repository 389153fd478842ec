"""Reconstruction metrics between two point clouds, on the device.

The reference answers "how good is the map" in utils/eval_utils.py (`evaluate_recon`, `nn_correspondance`,
`crop_union`) with an Open3D KD-tree queried one point at a time from Python.  Here the nearest-neighbour search
is one native call (sls_nn_query: the spatial index of `distCUDA2`, queried by a second cloud) and the metric block
(eval_utils.py:122-153) two more (sls_nn_stats) plus ONE host read of eight words.  Device tensors only; there is no
CPU path.

Not done here: reading or sampling triangle meshes, the bounding-box crop of a mesh and the voxel
down-sampling `evaluate_recon` applies to both clouds first.
"""
from __future__ import annotations

import math
import struct

import torch

from . import _abi


def _cloud(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    t = t.detach()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be (M,3)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _scratch(lib, Mt: int, Mq: int, device) -> tuple[torch.Tensor, int, int]:
    nbytes = int(lib.sls_nn_scratch_bytes(Mt, Mq))
    buf = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    return buf, (buf.data_ptr() + 255) & ~255, nbytes


def _query(lib, target, query, want_index, scratch, st):
    Mt, Mq = int(target.shape[0]), int(query.shape[0])
    dist2 = torch.empty((Mq,), dtype=torch.float32, device=target.device)
    index = torch.empty((Mq,), dtype=torch.int32, device=target.device) if want_index else None
    if Mq:
        _, aligned, nbytes = scratch
        _abi.check(lib.sls_nn_query(Mt, target.data_ptr(), Mq, query.data_ptr(), dist2.data_ptr(),
                                    index.data_ptr() if want_index else None, aligned, nbytes, st), "sls_nn_query")
    return dist2, index


def nearest(target: torch.Tensor, query: torch.Tensor, return_index: bool = True):
    """For every row of `query` (Mq,3) its nearest row of `target` (Mt,3): `(dist2 (Mq,) float32, index (Mq,) int32)`,
    or `(dist2, None)` with `return_index=False`.  dist2 is fmaf(dz,dz,fmaf(dy,dy,dx*dx)) of the float32 differences
    (include/sls_nn_math.h) and index the lowest target row attaining it, bit for bit."""
    target, query = _cloud(target, "target"), _cloud(query, "query")
    if query.device != target.device:
        raise ValueError("target and query must live on the same device")
    if target.shape[0] == 0:
        raise ValueError("the target cloud is empty")
    lib = _abi.lib()
    with torch.cuda.device(target.device):
        st = torch.cuda.current_stream(target.device).cuda_stream
        scratch = _scratch(lib, int(target.shape[0]), int(query.shape[0]), target.device)
        return _query(lib, target, query, return_index, scratch, st)


def crop_union_mask(reference: torch.Tensor, estimate: torch.Tensor, threshold_dist: float = 1.2) -> torch.Tensor:
    """bool (Mref,): the reference points with an estimate point nearer than `threshold_dist` — `crop_union`
    (eval_utils.py:202-250) after its mesh sampling; `estimate` is the merged cloud of all methods.  The comparison is
    dist2 < threshold_dist² in float32, on the device."""
    dist2, _ = nearest(estimate, reference, return_index=False)
    t = torch.tensor(float(threshold_dist), dtype=torch.float32)
    return dist2 < float(t * t)


def cloud_metrics(reference: torch.Tensor, estimate: torch.Tensor, threshold: float = 0.2, truncation_acc: float = 0.5,
                  truncation_com: float = 0.5) -> dict:
    """The metric block of `evaluate_recon` (eval_utils.py:122-153) for two point clouds, in metres and fractions.

    Accuracy: every estimate point against the reference cloud, points farther than `truncation_acc` dropped.
    Completeness: every reference point against the estimate cloud, points farther than `truncation_com` counted as
    `truncation_com`.  precision / recall: the fraction of either set below `threshold`.  An empty accuracy set gives
    NaN for `accuracy_m` and `precision` (the reference's mean of an empty array); `fscore` is 0.0 when
    precision + recall is 0."""
    reference, estimate = _cloud(reference, "reference"), _cloud(estimate, "estimate")
    if reference.device != estimate.device:
        raise ValueError("reference and estimate must live on the same device")
    Mr, Me = int(reference.shape[0]), int(estimate.shape[0])
    if Mr == 0 or Me == 0:
        raise ValueError("both clouds need at least one point")
    lib = _abi.lib()
    dev = reference.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        scratch = _scratch(lib, max(Mr, Me), max(Mr, Me), dev)
        _, aligned, nbytes = scratch
        words = torch.empty((8,), dtype=torch.int64, device=dev)
        d_acc, _ = _query(lib, reference, estimate, False, scratch, st)
        _abi.check(lib.sls_nn_stats(Me, d_acc.data_ptr(), float(truncation_acc), float(threshold), 0, words.data_ptr(),
                                    aligned, nbytes, st), "sls_nn_stats")
        d_com, _ = _query(lib, estimate, reference, False, scratch, st)
        _abi.check(lib.sls_nn_stats(Mr, d_com.data_ptr(), float(truncation_com), float(threshold), 1,
                                    words.data_ptr() + 32, aligned, nbytes, st), "sls_nn_stats")
        w = words.cpu().tolist()                                  # the one host read
    bits = lambda v: struct.unpack("<d", struct.pack("<q", v))[0]
    n_acc, below_acc, sum_acc = w[0], w[1], bits(w[2])
    n_com, below_com, sum_com = w[4], w[5], bits(w[6])
    accuracy = sum_acc / n_acc if n_acc else math.nan
    precision = below_acc / n_acc if n_acc else math.nan
    completeness = sum_com / n_com
    recall = below_com / n_com
    pr = precision + recall
    fscore = 2.0 * precision * recall / pr if pr != 0 else 0.0
    return {
        "accuracy_m": accuracy, "completeness_m": completeness, "chamfer_l1_m": 0.5 * (accuracy + completeness),
        "precision": precision, "recall": recall, "fscore": fscore,
        "n_accuracy": int(n_acc), "n_completeness": int(n_com),
        "threshold": float(threshold), "truncation_acc": float(truncation_acc), "truncation_com": float(truncation_com),
    }
