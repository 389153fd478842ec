#!/usr/bin/env python3
"""Reconstruction metrics between two point clouds (splat_loam_amd.evaluation.cloud_metrics), one JSON line:

    python tools/eval_cloud.py REFERENCE.ply ESTIMATE.ply [--threshold T] [--truncation-acc A] [--truncation-com C]
                               [--voxel RES]

Both files: binary little-endian PLY with `x y z` as float or double (what tools/sample_surface.py writes and what scan
exports usually are).  The metric block is the reference's `evaluate_recon` from the point it holds two vertex arrays
(utils/eval_utils.py:122-153), in metres and fractions.  --voxel RES voxel-down-samples both clouds at RES metres first
(evaluation.voxel_down_sample; the reference uses 0.02); the default 0 compares the clouds as they are.  For an
estimated MESH, and the reference's own dictionary, see tools/eval_recon.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import evaluation, ply_io


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reference_ply")
    ap.add_argument("estimate_ply")
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--truncation-acc", type=float, default=0.5)
    ap.add_argument("--truncation-com", type=float, default=0.5)
    ap.add_argument("--voxel", type=float, default=0.0, help="voxel size of a down-sampling of both clouds (0: none)")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    reference = torch.from_numpy(ply_io.load_point_cloud(a.reference_ply)[0]).to(dev)
    estimate = torch.from_numpy(ply_io.load_point_cloud(a.estimate_ply)[0]).to(dev)
    if a.voxel > 0:
        reference = evaluation.voxel_down_sample(reference, a.voxel)
        estimate = evaluation.voxel_down_sample(estimate, a.voxel)
    print(json.dumps(evaluation.cloud_metrics(reference, estimate, threshold=a.threshold, truncation_acc=a.truncation_acc,
                                              truncation_com=a.truncation_com)))


if __name__ == "__main__":
    main()
