#!/usr/bin/env python3
"""Fill the small holes of a triangle mesh on disk, on the device (splat_loam_amd.mesh_ops.fill_holes; DESIGN.md section 2,
"Mesh hole filling"):

    python tools/mesh_fill.py IN.ply OUT.ply [--max-edges 64] [--max-size M] [--capacity 0.25] [--normals]

IN.ply is read with `ply_io.load_mesh`, OUT.ply written with `ply_io.save_mesh` (binary little-endian; --normals adds
area-weighted vertex normals of the filled mesh as `nx ny nz`).  Every closed boundary loop of at most --max-edges edges
(64: a judgement, not a measurement) whose bounding box has a diagonal of at most --max-size (none by default) gets one
triangle (a loop of three) or a fan over its centroid; the vertices and faces of IN.ply come first, unchanged.  It is a fan
and nothing more: no refinement, no fairing, and chains of boundary edges that meet at a non-manifold vertex stay open.
Where --capacity (the room for new triangles as a share of the triangles) does not suffice, the tool retries once with the
room the first pass asked for.  Prints one JSON line: the counts of the stage and the boundary edges before and after."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import mesh_ops, ply_io


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--max-edges", type=int, default=64, help="the longest loop that is filled")
    ap.add_argument("--max-size", type=float, default=None, help="the largest bounding-box diagonal of a loop that is filled")
    ap.add_argument("--capacity", type=float, default=0.25, help="room for new triangles, as a share of the triangles")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    v, f = ply_io.load_mesh(a.in_ply)
    v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    capacity = a.capacity
    try:
        out_v, out_f, det = mesh_ops.fill_holes(v, f, max_edges=a.max_edges, max_size=a.max_size, capacity=capacity, details=True)
    except ValueError as e:
        need = re.search(r"(\d+) triangles and", str(e))
        if need is None or not f.shape[0]:
            raise
        capacity = (int(need.group(1)) - f.shape[0]) / f.shape[0]
        out_v, out_f, det = mesh_ops.fill_holes(v, f, max_edges=a.max_edges, max_size=a.max_size, capacity=capacity, details=True)
    normals = mesh_ops.vertex_normals(out_v, out_f) if a.normals else None
    ply_io.save_mesh(a.out_ply, out_v, out_f, normals=normals)
    after = mesh_ops.cluster_triangles(out_f, out_v.shape[0], details=True)[2] if out_f.shape[0] else {"boundary_edges": 0, "nonmanifold_edges": 0}
    line = {"input_vertices": int(v.shape[0]), "input_triangles": int(f.shape[0]), **det, "max_edges": a.max_edges, "max_size": a.max_size,
            "capacity": capacity, "boundary_edges_after": after["boundary_edges"], "nonmanifold_edges_after": after["nonmanifold_edges"],
            "normals": bool(a.normals), "path": a.out_ply}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
