#!/usr/bin/env python3
"""The range image of a triangle mesh from a pose, on the device (splat_loam_amd.evaluation.render_mesh); one JSON line
of statistics:

    python tools/mesh_render.py MESH.ply OUT.npz --pose 12 numbers --height H --width W [--vfov LO HI]

MESH.ply: binary little-endian PLY with a `vertex` element and one `face` element of triangles.  --pose: world_T_sensor
as 12 numbers, 3x4 row-major (the sensor's x axis looks along azimuth 0, z is up).  The sensor is the spherical one of the
rest of the tree: W columns over 360 degrees of azimuth, H rows from --vfov LO to HI degrees of elevation (default
-24.8 2.0, row 0 the top beam), pixel (c, r) along image coordinate (c - 0.5, r - 0.5).  OUT.npz: `range` (H,W) float32, 0 where nothing is
hit; `face` (H,W) int32, -1 there; `normal` (3,H,W) float32 in the sensor frame, towards the sensor; `K` (3,3), `pose` (4,4)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from splat_loam_amd import evaluation, ply_io, synth
from splat_loam_amd.scene import Camera


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh_ply")
    ap.add_argument("out_npz")
    ap.add_argument("--pose", type=float, nargs=12, required=True, metavar="P")
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--width", type=int, required=True)
    ap.add_argument("--vfov", type=float, nargs=2, default=(synth.EL_MIN_DEG, synth.EL_MAX_DEG), metavar=("LO", "HI"))
    ap.add_argument("--t-max", type=float, default=math.inf)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    H, W = a.height, a.width
    pose = np.vstack([np.asarray(a.pose, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    K = synth.spherical_K(H, W, a.vfov[0], a.vfov[1])
    vertices, faces = ply_io.load_mesh(a.mesh_ply)
    zero = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
    cam = Camera(K, zero, None, None, world_T_lidar=pose, data_device=dev)
    out = evaluation.render_mesh(torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev), cam, t_max=a.t_max)
    rng = out["range"].cpu().numpy()
    np.savez(a.out_npz, range=rng, face=out["face"].cpu().numpy(), normal=out["normal"].cpu().numpy(), K=np.asarray(K, np.float32),
             pose=pose)
    hit = rng > 0
    print(json.dumps({"faces": int(len(faces)), "height": H, "width": W, "hit": int(hit.sum()), "miss": int((~hit).sum()),
                      "mean_range_m": float(rng[hit].mean()) if hit.any() else None}))


if __name__ == "__main__":
    main()
