#!/usr/bin/env python3
"""The ground of a LiDAR scan on the device (splat_loam_amd.evaluation.segment_ground / ground_normals), one JSON line:

    python tools/cloud_ground.py IN.ply OUT.ply --sensor-height 1.723 [--split] [--max-range 80 ...]

IN.ply: binary little-endian PLY with `x y z` as float or double, in the SENSOR frame with z up, the sensor --sensor-height
above the ground (normals it may hold are replaced).  OUT.ply holds the same rows in the same order as `x y z nx ny nz`: a
ground point carries its bin's plane normal (unit, nz >= 0), every other point zeros — the zero normal is the label.  With
--split OUT.ply holds the ground rows only and OUT_rest.ply the others.

This is a region-wise ground-plane fit in the manner of Patchwork (Lim et al., RA-L 2021) restated from the paper
(include/sls_ground_math.h): concentric zones with sectors cut in the diamond angle, seeds from the lowest points of every
bin, an iterated PCA plane fit, uprightness / elevation / flatness tests.  It is not Patchwork or Patchwork++ themselves and
claims no parity with them; the defaults are a judgement."""
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
    ap.add_argument("--sensor-height", type=float, required=True, help="the sensor's height above the ground, cloud units")
    ap.add_argument("--split", action="store_true", help="OUT.ply: the ground rows; OUT_rest.ply: the others")
    for name, default in evaluation.GROUND_DEFAULTS.items():
        if isinstance(default, tuple):
            ap.add_argument("--" + name.replace("_", "-"), type=float, nargs=4, default=default)
        else:
            ap.add_argument("--" + name.replace("_", "-"), type=type(default), default=default)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    params = {name: getattr(a, name) for name in evaluation.GROUND_DEFAULTS}
    evaluation._check_ground_args(a.sensor_height, params)                     # before the file is read
    points, _ = ply_io.load_point_cloud(a.in_ply)
    points = torch.from_numpy(points).to(torch.device(a.device))
    mask, bins, planes, info, status = evaluation.segment_ground(points, a.sensor_height, return_details=True, **params)
    normals = evaluation.plane_normals(mask, bins, planes)
    outs = [a.out_ply]
    if a.split:
        stem, ext = os.path.splitext(a.out_ply)
        outs.append(stem + "_rest" + ext)
        ply_io.save_point_cloud(outs[0], points[mask], normals[mask])
        ply_io.save_point_cloud(outs[1], points[~mask], normals[~mask])
    else:
        ply_io.save_point_cloud(a.out_ply, points, normals)
    words = [int(w) for w in status.tolist()]
    states = torch.bincount(info[:, 3].long(), minlength=len(evaluation.GROUND_STATES)).tolist()
    line = {"points": int(points.shape[0]), "sensor_height": a.sensor_height, "with_bin": words[0], "ground": words[1],
            "non_finite": words[2], "bins": dict(zip(evaluation.GROUND_STATES, states)), "out": outs}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
