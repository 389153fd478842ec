#!/usr/bin/env python3
"""The large pieces of a point cloud on the device (splat_loam_amd.evaluation), one JSON line:

    python tools/cloud_cluster.py IN.ply OUT.ply --eps E --min-points N [--keep K] [--min-cluster S] [--labels]

IN.ply: binary little-endian PLY with `x y z` as float or double, optionally `nx ny nz` (what tools/sample_surface.py and
tools/cloud_ground.py write).  DBSCAN over exact radius neighbours (include/sls_cluster_math.h): a point with at least N
points, itself included, within E is core; clusters are the connected components of the cores; a non-core point within E of
a core is a border of the lowest-numbered such cluster; the rest is noise.  E is meant to be a few point spacings: the cost
grows with the number of pairs within E.  OUT.ply holds the points of the K largest clusters (default 1) and of every
cluster of at least S points, in their order, with their normals (zeros where IN has none).  With --labels OUT.ply holds the
WHOLE cloud instead, coloured by label — noise grey, cluster c a colour that is a fixed function of c — for a viewer.  The
classical next step after tools/cloud_ground.py: the Euclidean clusters of what is not ground."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import evaluation, ply_io


def label_colors(labels: torch.Tensor) -> torch.Tensor:
    """(M,3) uint8: grey for noise, otherwise three bytes of a multiplicative hash of the label, kept away from black"""
    h = (labels.long() + 1) * 2654435761 % (1 << 32)
    rgb = torch.stack([(h >> 24) & 255, (h >> 14) & 255, (h >> 4) & 255], 1) // 2 + 96
    rgb[labels < 0] = 128
    return rgb.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--eps", type=float, required=True, help="the neighbour radius in the cloud's unit: a few point spacings")
    ap.add_argument("--min-points", type=int, required=True, help="neighbours within eps, itself included, that make a point core")
    ap.add_argument("--keep", type=int, default=1, help="keep the K largest clusters (ties at the K-th place all stay; 0: the floor alone)")
    ap.add_argument("--min-cluster", type=int, default=0, help="... and every cluster of at least this many points")
    ap.add_argument("--labels", action="store_true", help="write the whole cloud coloured by label instead of the kept rows")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    points, normals = ply_io.load_point_cloud(a.in_ply)
    points = torch.from_numpy(points).to(dev)
    normals = torch.from_numpy(normals).to(dev) if normals is not None else None
    line = {"eps": a.eps, "min_points": a.min_points, "points": int(points.shape[0]), "out": a.out_ply}
    if a.labels:
        labels, counts, det = evaluation.cluster_dbscan(points, a.eps, a.min_points, return_counts=True, details=True)
        ply_io.save_point_cloud(a.out_ply, points, normals if normals is not None else torch.zeros_like(points),
                                colors=label_colors(labels).cpu().numpy())
        line.update(det, largest_counts=counts.sort(descending=True).values[:8].tolist())
    else:
        res = evaluation.keep_clusters(points, a.eps, a.min_points, keep=a.keep, min_cluster_points=a.min_cluster, normals=normals,
                                       details=True)
        kept_points, kept_normals = res[0], (res[1] if normals is not None else None)
        ply_io.save_point_cloud(a.out_ply, kept_points, kept_normals if kept_normals is not None else torch.zeros_like(kept_points))
        line.update(res[-1], keep=a.keep, min_cluster=a.min_cluster)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
