#!/usr/bin/env python3
"""The exact distance of every point of a cloud to a triangle mesh, on the device
(splat_loam_amd.evaluation.point_to_mesh), written as a coloured cloud; one JSON line of statistics:

    python tools/mesh_distance.py POINTS.ply MESH.ply OUT.ply --truncation T [--signed]

POINTS.ply: binary little-endian PLY with `x y z` as float or double.  MESH.ply: binary little-endian PLY with a `vertex`
element and one `face` element of triangles.  OUT.ply: the points with `uchar red green blue` — green on the surface,
yellow at T / 2 metres from it, red at T metres or beyond (evaluation.error_colors); the normals of POINTS.ply are kept
where it has them, zeros otherwise.  The distance is unsigned: a point inside a closed mesh is as red as one outside.
--signed gives it the sign of the mesh's pseudo-normals (evaluation.signed_distance) and the diverging colours of
evaluation.signed_error_colors instead: white on the surface, red at T metres in FRONT of the faces (the side they look to;
for a mesh of mesh_tsdf / mesh_poisson the observed, free-space side), blue at T metres BEHIND them; the line then also
holds `signed_mean_m` and `share_behind` over the points within T, and the facts about the mesh the sign depends on."""
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
    ap.add_argument("points_ply")
    ap.add_argument("mesh_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--truncation", type=float, required=True, metavar="T", help="the distance in metres that is fully red")
    ap.add_argument("--signed", action="store_true", help="signed distances, diverging colours, the signed mean")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    evaluation._check_truncation(a.truncation)                                 # before the files are read
    dev = torch.device(a.device)
    points, normals = ply_io.load_point_cloud(a.points_ply)
    vertices, faces = ply_io.load_mesh(a.mesh_ply)
    pts = torch.from_numpy(points).to(dev)
    vt, ft = torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev)
    extra = {}
    if a.signed:
        pn, details = evaluation.mesh_pseudonormals(vt, ft, return_details=True)
        sdist = evaluation.signed_distance(pts, vt, ft, pseudonormals=pn)
        dist2 = sdist.double().square()
        colors = evaluation.signed_error_colors(sdist, a.truncation)
        within = sdist[sdist.abs() < a.truncation].double()
        extra = {"signed_mean_m": float(within.mean()) if len(within) else None,
                 "share_behind": float((within < 0).double().mean()) if len(within) else None, "n_within": int(len(within)), **details}
    else:
        dist2, face = evaluation.point_to_mesh(pts, vt, ft)
        colors = evaluation.error_colors(dist2, a.truncation)
    ply_io.save_point_cloud(a.out_ply, points, normals if normals is not None else np.zeros_like(points), colors)
    d = dist2.double().sqrt()
    print(json.dumps({"points": int(len(points)), "faces": int(len(faces)), "truncation": a.truncation,
                      "mean_m": float(d.mean()) if len(points) else None, "max_m": float(d.max()) if len(points) else None,
                      "beyond_truncation": int((d >= a.truncation).sum()), **extra}))


if __name__ == "__main__":
    main()
