#!/usr/bin/env python3
"""Register one cloud or mesh onto a cloud on the device (splat_loam_amd.evaluation.register_icp) and write it moved:

    python tools/cloud_align.py SOURCE.ply TARGET.ply OUT.ply --max-distance D [--init 12 numbers] [--method point]
                                [--iterations 30] [--max-points 200000] [--seed 0]

SOURCE.ply: a binary little-endian PLY point cloud, or a triangle mesh (its vertices are registered, its faces kept).
TARGET.ply: a point cloud; with --method plane (the default) its normals `nx ny nz` are used where the file has them and
estimated otherwise (evaluation.estimate_normals, radius 0.5, 30 neighbours, viewpoint at the origin).  Gauss-Newton ICP
on exact nearest neighbours, pairs farther apart than D ignored, no robust weight (include/sls_icp_math.h).  It is NOT a
global registration: --init (row-major 3x4 target_T_source, default the identity) must bring the source within D of the
target.  A source of more than --max-points rows is registered on a seeded draw of that many; every row is moved.
OUT.ply holds the source moved by the pose found (normals of a cloud rotated with it).  Prints one JSON line (fitness,
inlier_rmse, inliers, updates, flags) and, as the LAST line, the pose in KITTI order: 12 numbers, the row-major 3x4
target_T_source."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from splat_loam_amd import evaluation, ply_io


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source_ply")
    ap.add_argument("target_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--max-distance", type=float, required=True, help="the gate, in the clouds' unit")
    ap.add_argument("--init", type=float, nargs=12, default=None, help="row-major 3x4 target_T_source")
    ap.add_argument("--method", choices=("plane", "point"), default="plane")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--max-points", type=int, default=evaluation.ALIGN_MAX_POINTS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    evaluation._check_icp_args(a.max_distance, a.iterations, a.method, a.init, {})      # before the files are read
    dev = torch.device(a.device)
    faces = normals = None
    try:
        points, faces = ply_io.load_mesh(a.source_ply)
    except ValueError:
        points, normals = ply_io.load_point_cloud(a.source_ply)
    target, target_normals = ply_io.load_point_cloud(a.target_ply)
    points, target = torch.from_numpy(points).to(dev), torch.from_numpy(target).to(dev)
    if target_normals is not None and a.method == "plane":
        target_normals = torch.from_numpy(target_normals).to(dev)
    else:
        target_normals = None
    # the bounded subset and the call are evaluate_recon(align=)'s
    res = evaluation._align_vertices(target, points, dict(max_distance=a.max_distance, iterations=a.iterations, method=a.method,
                                                          init=a.init, target_normals=target_normals, max_points=a.max_points,
                                                          seed=a.seed))
    pose = res.pop("target_T_source")
    moved = evaluation.transform_points(points, pose)
    if faces is not None:
        ply_io.save_mesh(a.out_ply, moved, faces)
    else:
        rot = pose.clone()
        rot[:3, 3] = 0.0
        turned = evaluation.transform_points(torch.from_numpy(normals).to(dev), rot) if normals is not None else torch.zeros_like(moved)
        ply_io.save_point_cloud(a.out_ply, moved, turned)
    res.update(source_rows=int(points.shape[0]), target_rows=int(target.shape[0]), method=a.method, max_distance=a.max_distance,
               out=a.out_ply)
    print(json.dumps(res))
    print(" ".join(repr(float(v)) for v in pose[:3].reshape(-1).tolist()))


if __name__ == "__main__":
    main()
