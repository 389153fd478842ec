#!/usr/bin/env python3
"""Does a mesh agree with what the map renders from its own keyframes?  (splat_loam_amd.meshing.mesh_depth_check: no
reference cloud is needed.)  Prints one row per keyframe and one for all of them; --json also writes the figures:

    python tools/mesh_depth_check.py RESULTS_DIR MESH.ply [--json OUT] [--truncation T] [--kf-interval K] ...

RESULTS_DIR: a results directory (graph.yaml, models/*.ply, cfg.yaml or --image-height / --image-width).  MESH.ply:
binary little-endian PLY with a `vertex` element and one `face` element of triangles, in the world frame.  Per row: the
valid pixels of the map's render (the surface sampler's rule), how many of them the mesh covers, and the mean and median
of |range of the mesh - depth of the map| over those, truncated at T metres."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

import mesh_cli
from splat_loam_amd import meshing, ply_io


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("results_dir")
    ap.add_argument("mesh_ply")
    ap.add_argument("--json", default=None, metavar="OUT", help="write the figures here as JSON")
    ap.add_argument("--truncation", type=float, default=0.5, metavar="T", help="residuals are truncated at T metres")
    mesh_cli.add_sample_arguments(ap)           # (of which --kf-samples and --seed do not matter here)
    a = ap.parse_args()
    dev = torch.device(a.device)
    vertices, faces = ply_io.load_mesh(a.mesh_ply)
    options = {k: getattr(a, k) for k in meshing._DEPTH_CHECK_OPTIONS}
    res = meshing.mesh_depth_check(a.results_dir, torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev),
                                   truncation=a.truncation, device=dev, **options)
    fmt = lambda v: "       -" if v is None else f"{v:8.4f}"
    print(f"{'frame':>8} {'valid':>9} {'covered':>9} {'share':>7} {'mean m':>8} {'median m':>8}")
    for r in res["keyframes"] + [dict(res, frame_id="all")]:
        share = r["covered"] / r["valid"] if r["valid"] else 0.0
        print(f"{str(r['frame_id']):>8} {r['valid']:9d} {r['covered']:9d} {share:7.3f} {fmt(r['mean'])} {fmt(r['median'])}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(res, mesh=a.mesh_ply, results_dir=a.results_dir, faces=int(len(faces)), options=options), f, indent=1)


if __name__ == "__main__":
    main()
