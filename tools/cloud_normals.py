#!/usr/bin/env python3
"""Normals of a point cloud by PCA on the device (splat_loam_amd.evaluation.estimate_normals), one JSON line:

    python tools/cloud_normals.py IN.ply OUT.ply --radius 0.5 --max-nn 30 [--viewpoint x y z]

IN.ply: binary little-endian PLY with `x y z` as float or double (normals it may hold are replaced); OUT.ply holds the same
rows in the same order as `x y z nx ny nz`.  This is Open3D's
`estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))` + `orient_normals_towards_camera_location(viewpoint)` as
restated in include/sls_normals_math.h: the neighbourhood of a point is the part of its --max-nn nearest points, itself
included, within --radius (1 <= max-nn <= 64; --radius 0 or less: the max-nn nearest whatever their distance); a point
with fewer than three neighbours gets unit(viewpoint - point).  A cloud for the Poisson hand-off of tools/sample_surface.py
or for tools/eval_cloud.py that arrives without normals gets them this way."""
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
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--radius", type=float, default=0.5, help="the neighbourhood's radius in the cloud's unit (<= 0: none)")
    ap.add_argument("--max-nn", type=int, default=30, help="at most this many neighbours, the point itself included (1..64)")
    ap.add_argument("--viewpoint", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"),
                    help="the normals are flipped towards this point")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    radius = a.radius if a.radius > 0 else None
    evaluation._check_normals_args(radius, a.max_nn, a.viewpoint)              # before the file is read
    points, _ = ply_io.load_point_cloud(a.in_ply)
    points = torch.from_numpy(points).to(torch.device(a.device))
    normals, count, eig = evaluation.estimate_normals(points, radius, a.max_nn, a.viewpoint, return_details=True)
    ply_io.save_point_cloud(a.out_ply, points, normals)
    M = int(points.shape[0])
    line = {"points": M, "radius": radius, "max_nn": a.max_nn, "viewpoint": list(a.viewpoint),
            "fallback_points": int((count < 3).sum()) if M else 0,
            "mean_neighbours": float(count.double().mean()) if M else 0.0, "out": a.out_ply}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
