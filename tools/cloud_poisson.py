#!/usr/bin/env python3
"""Any oriented cloud to a triangle mesh by screened Poisson reconstruction on the device
(splat_loam_amd.poisson.reconstruct; DESIGN.md section 2, "Poisson volume"), one JSON line:

    python tools/cloud_poisson.py IN.ply OUT.ply --voxel 0.1 [--margin M] [--screening A] [--iterations N] [--tol T]
                                  [--min-density D] [--density-sweeps S] [--weld]
                                  [--radius 0.5 --max-nn 30 --viewpoint x y z]

IN.ply: binary little-endian PLY with `x y z` and `nx ny nz`; the normals must point to free space for the mesh's normals
to do so.  A cloud WITHOUT normals gets them from `evaluation.estimate_normals(--radius, --max-nn, --viewpoint)` first (PCA,
flipped towards the viewpoint), and the JSON line says so (`normals: "estimated"`).  A uniform band of --voxel voxels,
trilinear splats, a screened least-squares fit: not Open3D's octree solver, no parity with it is claimed.  The defaults of
--margin (3 voxels), --screening, --iterations, --tol and --density-sweeps are judgements."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import evaluation, ply_io, poisson


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--voxel", type=float, required=True, help="edge of a voxel in the cloud's unit")
    ap.add_argument("--margin", type=float, default=None, help="half width of the band around the points (default 3 voxels)")
    ap.add_argument("--screening", type=float, default=4.0)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--min-density", type=float, default=None, help="keep only cubes whose corners have this smoothed density")
    ap.add_argument("--density-sweeps", type=int, default=2)
    ap.add_argument("--weld", action="store_true", help="merge bit-equal vertices before writing")
    ap.add_argument("--radius", type=float, default=0.5, help="normal estimation, for a cloud without normals: the radius")
    ap.add_argument("--max-nn", type=int, default=30, help="... and the most neighbours")
    ap.add_argument("--viewpoint", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"), help="... flipped towards this point")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    points, normals = ply_io.load_point_cloud(a.in_ply)
    points = torch.from_numpy(points).to(dev)
    estimated = normals is None
    if estimated:
        normals = evaluation.estimate_normals(points, a.radius if a.radius > 0 else None, a.max_nn, a.viewpoint)
    else:
        normals = torch.from_numpy(normals).to(dev)
    vertices, faces, det = poisson.reconstruct(points, normals, a.voxel, a.margin, screening=a.screening, iterations=a.iterations, tol=a.tol,
                                               min_density=a.min_density, density_sweeps=a.density_sweeps, weld=a.weld, details=True)
    ply_io.save_mesh(a.out_ply, vertices, faces)
    print(json.dumps({"points": int(points.shape[0]), "normals": "estimated" if estimated else "given", "blocks": det["blocks"],
                      "splat": det["splat"], "solve": det["solve"], "triangles": int(faces.shape[0]), "vertices": int(vertices.shape[0]),
                      "out": a.out_ply}))


if __name__ == "__main__":
    main()
