#!/usr/bin/env python3
"""Smooth a triangle mesh on disk over its edge graph, on the device (splat_loam_amd.mesh_ops.smooth; DESIGN.md section 2,
"Mesh smoothing"):

    python tools/mesh_smooth.py IN.ply OUT.ply --iterations N [--method laplacian|simple] [--weights uniform]
                                [--lambda L] [--mu M] [--fix-boundary] [--normals]

IN.ply is read with `ply_io.load_mesh`, OUT.ply written with `ply_io.save_mesh` (binary little-endian; --normals adds
area-weighted vertex normals of the smoothed mesh as `nx ny nz`).  The default is Open3D's `filter_smooth_taubin`: per
iteration a sweep with --lambda (0.5) and one with --mu (-0.53), inverse-distance weights; --method laplacian shrinks the
mesh, --method simple averages a vertex with its neighbours.  The faces are written as they came.  Prints one JSON line:
the counts of the edge graph (live vertices, edges, boundary vertices, degenerate triangles, the largest row) and how far
the vertices moved (mean and largest displacement)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import mesh_ops, ply_io


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--iterations", type=int, required=True)
    ap.add_argument("--method", choices=("taubin", "laplacian", "simple"), default="taubin")
    ap.add_argument("--weights", choices=("inverse_distance", "uniform"), default="inverse_distance")
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.5, help="the factor of a sweep")
    ap.add_argument("--mu", type=float, default=-0.53, help="the factor of Taubin's second sweep")
    ap.add_argument("--fix-boundary", action="store_true", help="leave the boundary vertices where they are")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    v, f = ply_io.load_mesh(a.in_ply)
    v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    out_v, det = mesh_ops.smooth(v, f, a.iterations, method=a.method, weights=a.weights, lambda_=a.lambda_, mu=a.mu,
                                 fix_boundary=a.fix_boundary, details=True)
    normals = mesh_ops.vertex_normals(out_v, f) if a.normals else None
    ply_io.save_mesh(a.out_ply, out_v, f, normals=normals)
    moved = (out_v.double() - v.double()).norm(dim=1) if v.shape[0] else torch.zeros((1,), dtype=torch.float64)
    line = {"vertices": int(v.shape[0]), "triangles": int(f.shape[0]), **det, "iterations": a.iterations, "method": a.method,
            "weights": a.weights, "lambda": a.lambda_, "mu": a.mu, "fix_boundary": bool(a.fix_boundary), "normals": bool(a.normals),
            "moved_mean": float(moved.mean()), "moved_max": float(moved.max()), "path": a.out_ply}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
