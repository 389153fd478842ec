#!/usr/bin/env python3
"""Outlier removal of a point cloud on the device (splat_loam_amd.evaluation), one JSON line:

    python tools/cloud_filter.py IN.ply OUT.ply --nb 20 [--std 2.0]
    python tools/cloud_filter.py IN.ply OUT.ply --radius R --min-points N

IN.ply: binary little-endian PLY with `x y z` as float or double, optionally `nx ny nz` (what tools/sample_surface.py
writes and what scan exports usually are); OUT.ply holds the kept rows in their order with their normals (zeros where IN has
none: the writer's layout is `x y z nx ny nz`).  --nb K [--std S] is Open3D's `remove_statistical_outlier(nb_neighbors=K, std_ratio=S)` as restated in
include/sls_outlier_math.h (the point itself is one of its K neighbours; 1 <= K <= 32); --radius R --min-points N keeps
the points with MORE than N points, themselves included, within R (0 <= N <= 31).  A cloud for tools/eval_cloud.py can
be cleaned this way on either side."""
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
    ap.add_argument("--nb", type=int, default=None, help="statistical filter: neighbours, the point itself included (1..32)")
    ap.add_argument("--std", type=float, default=2.0, help="statistical filter: the threshold in standard deviations")
    ap.add_argument("--radius", type=float, default=None, help="radius filter: the radius in the cloud's unit")
    ap.add_argument("--min-points", type=int, default=None, help="radius filter: keep a point with MORE than this many within the radius (0..31)")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    statistical = a.nb is not None
    if statistical == (a.radius is not None):
        ap.error("give either --nb K [--std S] or --radius R --min-points N")
    if not statistical and a.min_points is None:
        ap.error("--radius needs --min-points")
    dev = torch.device(a.device)
    points, normals = ply_io.load_point_cloud(a.in_ply)
    points = torch.from_numpy(points).to(dev)
    normals = torch.from_numpy(normals).to(dev) if normals is not None else None
    if statistical:
        res = evaluation.remove_statistical_outlier(points, a.nb, a.std, normals=normals, details=True)
        line = {"filter": "statistical", "nb_neighbors": a.nb, "std_ratio": a.std}
    else:
        res = evaluation.remove_radius_outlier(points, a.min_points, a.radius, normals=normals, details=True)
        line = {"filter": "radius", "nb_points": a.min_points, "radius": a.radius}
    kept_points, kept_normals = res[0], (res[1] if normals is not None else None)
    ply_io.save_point_cloud(a.out_ply, kept_points, kept_normals if kept_normals is not None else torch.zeros_like(kept_points))
    line.update(res[-1], points=int(points.shape[0]), out=a.out_ply)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
