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

from splat_loam_amd import meshing, ply_io, tsdf


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("results_dir")
    ap.add_argument("out_ply")
    ap.add_argument("--voxel", type=float, required=True, help="edge of a voxel in metres")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance (default 4 voxels)")
    ap.add_argument("--kf-interval", type=int, default=-1)
    ap.add_argument("--kf-samples", type=int, default=5000)
    ap.add_argument("--min-opacity", type=float, default=0.5)
    ap.add_argument("--max-depth-dist", type=float, default=0.1)
    ap.add_argument("--use-median-depth", action="store_true")
    ap.add_argument("--min-weight", type=float, default=1.0)
    ap.add_argument("--weld", action="store_true", help="merge bit-equal vertices before writing")
    ap.add_argument("--keep-clusters", type=int, default=None, help="weld, then keep the K largest clusters of triangles")
    ap.add_argument("--min-triangles", type=int, default=50, help="... and every cluster of at least N triangles (with --keep-clusters)")
    ap.add_argument("--normals", action="store_true", help="weld and write area-weighted vertex normals")
    ap.add_argument("--simplify", type=float, default=None, help="weld, then merge the vertices of every voxel of this edge (metres)")
    ap.add_argument("--contraction", choices=("average", "quadric"), default="average", help="where a merged vertex goes (with --simplify)")
    ap.add_argument("--regularisation", type=float, default=1e-3, help="pull of the quadric placement towards the mean (with --simplify)")
    ap.add_argument("--smooth", type=int, default=None, help="weld, then run N smoothing sweeps over the edge graph")
    ap.add_argument("--smooth-method", choices=("taubin", "laplacian", "simple"), default="taubin", help="the sweep (with --smooth)")
    ap.add_argument("--smooth-weights", choices=("inverse_distance", "uniform"), default="inverse_distance", help="neighbour weights (with --smooth)")
    ap.add_argument("--fix-boundary", action="store_true", help="leave the boundary vertices where they are (with --smooth)")
    ap.add_argument("--fill-holes", type=int, default=None, help="weld, then fill the boundary loops of at most N edges")
    ap.add_argument("--fill-max-size", type=float, default=None, help="... whose bounding box has at most this diagonal (with --fill-holes)")
    ap.add_argument("--outlier-nb", type=int, default=None, help="statistical outlier removal of the surface samples: neighbours (1..32)")
    ap.add_argument("--outlier-std", type=float, default=2.0, help="... and the threshold in standard deviations (with --outlier-nb)")
    ap.add_argument("--cluster-eps", type=float, default=None, help="keep the largest DBSCAN cluster of the surface samples: the radius, a few sample spacings")
    ap.add_argument("--cluster-min-points", type=int, default=10, help="... and the neighbours, itself included, that make a sample core (with --cluster-eps)")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--image-height", type=int, default=None)
    ap.add_argument("--image-width", type=int, default=None)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    *mesh, det = meshing.mesh_tsdf(a.results_dir, a.voxel, a.trunc, kf_interval=a.kf_interval, kf_samples=a.kf_samples,
                                   min_opacity=a.min_opacity, max_depth_dist=a.max_depth_dist, use_median_depth=a.use_median_depth,
                                   min_weight=a.min_weight, seed=a.seed, device=a.device, details=True, image_height=a.image_height,
                                   image_width=a.image_width, keep_clusters=a.keep_clusters, min_triangles=a.min_triangles,
                                   normals=a.normals, simplify=a.simplify, contraction=a.contraction, regularisation=a.regularisation,
                                   smooth=a.smooth, smooth_method=a.smooth_method, smooth_weights=a.smooth_weights,
                                   fix_boundary=a.fix_boundary, fill_holes=a.fill_holes, fill_max_size=a.fill_max_size,
                                   outlier_nb=a.outlier_nb, outlier_std=a.outlier_std, cluster_eps=a.cluster_eps,
                                   cluster_min_points=a.cluster_min_points)
    vertices, faces, normals = mesh[0], mesh[1], (mesh[2] if a.normals else None)
    if a.weld and "clean" not in det:
        vertices, faces = tsdf.weld_soup(vertices)
    ply_io.save_mesh(a.out_ply, vertices, faces, normals=normals)
    line = {"blocks": det["blocks"], "volume_bytes": det["volume_bytes"], "triangles": det["triangles"],
            "vertices": int(vertices.shape[0]), "keyframes": len(det["frame_ids"]), "samples": det["samples"],
            "stage_ms": {k: round(v, 3) for k, v in det["stage_ms"].items()}, "out": a.out_ply}
    if "outlier" in det:
        line["outlier"] = dict({k: v for k, v in det["outlier"].items() if k != "index"}, nb_neighbors=a.outlier_nb, std_ratio=a.outlier_std)
    if "cluster" in det:
        line["cluster"] = dict({k: v for k, v in det["cluster"].items() if k != "index"}, eps=a.cluster_eps, min_points=a.cluster_min_points)
    if "clean" in det:
        line["clean"] = {k: det["clean"][k] for k in ("welded_vertices", "clusters", "degenerate", "boundary_edges", "nonmanifold_edges",
                                                      "n_min")}
        line["clean"]["triangles_kept"] = int(faces.shape[0])
        line["clean"]["normals"] = bool(a.normals)
        if "simplify" in det["clean"]:
            line["clean"]["simplify"] = {k: v for k, v in det["clean"]["simplify"].items() if k != "vmap"}
            line["clean"]["simplify"].update(voxel=a.simplify, contraction=a.contraction)
        if "smooth" in det["clean"]:
            line["clean"]["smooth"] = dict(det["clean"]["smooth"], iterations=a.smooth, method=a.smooth_method, weights=a.smooth_weights,
                                           fix_boundary=bool(a.fix_boundary))
        if "fill" in det["clean"]:
            line["clean"]["fill"] = dict(det["clean"]["fill"], max_edges=a.fill_holes, max_size=a.fill_max_size)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
