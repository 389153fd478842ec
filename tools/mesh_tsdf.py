#!/usr/bin/env python3
"""From a results directory (graph.yaml, models/*.ply, optionally cfg.yaml) to a triangle mesh, on the device: the
rendered depth of every keyframe fused into a sparse TSDF volume, the zero surface by marching tetrahedra
(splat_loam_amd.meshing.mesh_tsdf; DESIGN.md section 2, "TSDF volume"):

    python tools/mesh_tsdf.py RESULTS_DIR OUT.ply --voxel 0.1 [--trunc T] [--kf-interval N] [--kf-samples K]
                              [--min-opacity A] [--max-depth-dist D] [--use-median-depth] [--min-weight W] [--weld]
                              [--keep-clusters K] [--min-triangles N] [--normals]
                              [--simplify RES [--contraction quadric] [--regularisation L]]
                              [--smooth N [--smooth-method laplacian] [--smooth-weights uniform] [--fix-boundary]]
                              [--fill-holes 64 [--fill-max-size M]]
                              [--outlier-nb 20 [--outlier-std 2.0]] [--cluster-eps E [--cluster-min-points 10]]
                              [--seed S] [--image-height H --image-width W]

OUT.ply is a binary little-endian triangle mesh (`ply_io.save_mesh`), what `tools/eval_recon.py` takes as the estimate.
--keep-clusters K welds the soup and keeps only the K largest edge-connected clusters of triangles and those of at least
--min-triangles triangles (`mesh_ops.clean_mesh`: the floaters go); --normals adds area-weighted vertex normals as
`nx ny nz`; --simplify RES merges the vertices of every voxel of edge RES after the selection
(`mesh_ops.simplify_vertex_clustering`: at their mean, or with --contraction quadric at the minimum of the voxel's error
quadric); --smooth N runs N smoothing sweeps over the edge graph before the normals (`mesh_ops.smooth`: Taubin with
inverse-distance weights unless told otherwise; --fix-boundary leaves the boundary vertices where they are); --fill-holes N
closes the boundary loops of at most N edges (and a bounding-box diagonal of at most --fill-max-size) after the selection
with a fan over their centroid (`mesh_ops.fill_holes`); --outlier-nb K filters the surface samples that name the volume's
blocks (`evaluation.remove_statistical_outlier(K, --outlier-std)`: what the reference's mesh_poisson meant to do).  Prints one JSON line: blocks, bytes of the volume (4 KB per block), triangles, milliseconds per stage, and
with a clean stage its statistics (of the welded mesh: clusters, degenerate triangles, boundary and non-manifold edges;
n_min; the triangles kept; the counts of the hole filling, of the simplification and of the smoothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mesh_cli
from splat_loam_amd import meshing, ply_io, tsdf


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("results_dir")
    ap.add_argument("out_ply")
    ap.add_argument("--voxel", type=float, required=True, help="edge of a voxel in metres")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance (default 4 voxels)")
    ap.add_argument("--min-weight", type=float, default=1.0)
    ap.add_argument("--weld", action="store_true", help="merge bit-equal vertices before writing")
    mesh_cli.add_sample_arguments(ap)
    mesh_cli.add_cloud_arguments(ap)
    mesh_cli.add_clean_arguments(ap)
    return ap


def main():
    a = build_parser().parse_args()
    *mesh, det = meshing.mesh_tsdf(a.results_dir, a.voxel, a.trunc, min_weight=a.min_weight, device=a.device, details=True,
                                   **mesh_cli.sample_options(a), **mesh_cli.clean_options(a))
    vertices, faces, normals = mesh[0], mesh[1], (mesh[2] if a.normals else None)
    if a.weld and "clean" not in det:
        vertices, faces = tsdf.weld_soup(vertices)
    ply_io.save_mesh(a.out_ply, vertices, faces, normals=normals)
    line = {"blocks": det["blocks"], "volume_bytes": det["volume_bytes"], "triangles": det["triangles"],
            "vertices": int(vertices.shape[0]), "keyframes": len(det["frame_ids"]), "samples": det["samples"],
            "stage_ms": {k: round(v, 3) for k, v in det["stage_ms"].items()}, "out": a.out_ply}
    line.update(mesh_cli.cloud_report(det, a))
    if "clean" in det:
        line["clean"] = mesh_cli.clean_report(det, a, faces)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
