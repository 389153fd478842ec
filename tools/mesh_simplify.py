#!/usr/bin/env python3
"""Simplify a triangle mesh on disk by vertex clustering, on the device (splat_loam_amd.mesh_ops.simplify_vertex_clustering;
DESIGN.md section 2, "Mesh simplification"):

    python tools/mesh_simplify.py IN.ply OUT.ply --voxel RES [--contraction quadric] [--regularisation L] [--normals]

IN.ply is read with `ply_io.load_mesh`, OUT.ply written with `ply_io.save_mesh` (binary little-endian; --normals adds
area-weighted vertex normals as `nx ny nz`).  The vertices of every voxel of edge RES become one vertex, at their mean or,
with --contraction quadric, at the minimum of the voxel's error quadric (edges and corners stay sharp).  Clustering does not
preserve manifoldness: the JSON line printed at the end holds the counts of the simplification and, from
`mesh_ops.cluster_triangles`, the clusters, boundary edges and non-manifold edges of the mesh before and after."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import mesh_ops, ply_io


def _edges(vertices, faces):
    det = mesh_ops.cluster_triangles(faces, int(vertices.shape[0]), details=True)[2]
    return {k: det[k] for k in ("clusters", "degenerate", "boundary_edges", "nonmanifold_edges")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    ap.add_argument("--voxel", type=float, required=True, help="edge of a clustering voxel, in the units of the mesh")
    ap.add_argument("--contraction", choices=("average", "quadric"), default="average")
    ap.add_argument("--regularisation", type=float, default=1e-3, help="pull of the quadric placement towards the mean")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    dev = torch.device(a.device)
    v, f = ply_io.load_mesh(a.in_ply)
    v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    out_v, out_f, det = mesh_ops.simplify_vertex_clustering(v, f, a.voxel, contraction=a.contraction, regularisation=a.regularisation,
                                                            details=True)
    normals = mesh_ops.vertex_normals(out_v, out_f) if a.normals else None
    ply_io.save_mesh(a.out_ply, out_v, out_f, normals=normals)
    line = {"in": {"vertices": int(v.shape[0]), "triangles": int(f.shape[0]), **(_edges(v, f) if f.shape[0] else {})},
            "out": {**{k: x for k, x in det.items() if k != "vmap"}, **(_edges(out_v, out_f) if out_f.shape[0] else {})},
            "voxel": a.voxel, "contraction": a.contraction, "regularisation": a.regularisation, "normals": bool(a.normals),
            "path": a.out_ply}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
