#!/usr/bin/env python3
"""From a results directory (graph.yaml, models/*.ply, optionally cfg.yaml) to a triangle mesh by screened Poisson
reconstruction on the device (splat_loam_amd.meshing.mesh_poisson; DESIGN.md section 2, "Poisson volume"): the reference's
`mesh_poisson` to its end — sample every keyframe, merge, solve, trim by density, vertex normals:

    python tools/mesh_poisson.py RESULTS_DIR OUT.ply --voxel 0.1 [--margin M] [--screening A] [--iterations N] [--tol T]
                                 [--min-density D | --min-density-quantile Q] [--density-sweeps S]
                                 [--kf-interval N] [--kf-samples K] [--min-opacity A] [--max-depth-dist D]
                                 [--use-median-depth] [--outlier-nb 20 [--outlier-std 2.0]] [--cluster-eps E [--cluster-min-points 10]] [--weld]
                                 [--keep-clusters K] [--min-triangles N] [--normals]
                                 [--simplify RES [--contraction quadric] [--regularisation L]]
                                 [--smooth N [--smooth-method laplacian] [--smooth-weights uniform] [--fix-boundary]]
                                 [--fill-holes 64 [--fill-max-size M]] [--seed S] [--image-height H --image-width W]

What it IS: a uniform band of --voxel voxels --margin (default 3 voxels) around the samples, trilinear splats, a
least-squares fit screened by the sample density (--screening), Jacobi-preconditioned conjugate gradients to a relative
residual of --tol.  What it is NOT: Open3D's adaptive octree solver; --voxel takes the place of its depth, and
--min-density-quantile Q (the Q-quantile of the smoothed density over the voxels that hold a sample) is not its quantile of
vertex densities.  The defaults of --margin, --screening, --iterations, --tol and --density-sweeps are judgements.  The
clean-up flags are those of tools/mesh_tsdf.py.  Prints one JSON line: blocks, samples, triangles, the solve's passes and
residual, milliseconds per stage and with a clean stage its statistics."""
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
    ap.add_argument("--margin", type=float, default=None, help="half width of the band around the samples (default 3 voxels; a judgement)")
    ap.add_argument("--screening", type=float, default=4.0, help="weight of the samples' density in the fit (a judgement)")
    ap.add_argument("--iterations", type=int, default=300, help="at most this many passes of conjugate gradients (0..1000)")
    ap.add_argument("--tol", type=float, default=1e-4, help="relative residual at which the solve ends (a judgement)")
    ap.add_argument("--min-density", type=float, default=None, help="keep only cubes whose corners have this smoothed density")
    ap.add_argument("--min-density-quantile", type=float, default=None, help="... or this quantile of it over the voxels with a sample")
    ap.add_argument("--density-sweeps", type=int, default=2, help="smoothing sweeps of the density (a judgement)")
    ap.add_argument("--kf-interval", type=int, default=-1)
    ap.add_argument("--kf-samples", type=int, default=5000)
    ap.add_argument("--min-opacity", type=float, default=0.5)
    ap.add_argument("--max-depth-dist", type=float, default=0.1)
    ap.add_argument("--use-median-depth", action="store_true")
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
    *mesh, det = meshing.mesh_poisson(a.results_dir, a.voxel, margin=a.margin, screening=a.screening, iterations=a.iterations, tol=a.tol,
                                      min_density=a.min_density, min_density_quantile=a.min_density_quantile,
                                      density_sweeps=a.density_sweeps, kf_interval=a.kf_interval, kf_samples=a.kf_samples,
                                      min_opacity=a.min_opacity, max_depth_dist=a.max_depth_dist, use_median_depth=a.use_median_depth,
                                      seed=a.seed, device=a.device, details=True, image_height=a.image_height,
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
    line = {"blocks": det["blocks"], "samples": det["samples"], "triangles": det["triangles"], "vertices": int(vertices.shape[0]),
            "keyframes": len(det["frame_ids"]), "solve": det["solve"], "min_density": det["min_density"],
            "stage_ms": {k: round(v, 3) for k, v in det["stage_ms"].items()}, "out": a.out_ply}
    if "outlier" in det:
        line["outlier"] = dict({k: v for k, v in det["outlier"].items() if k != "index"}, nb_neighbors=a.outlier_nb, std_ratio=a.outlier_std)
    if "cluster" in det:
        line["cluster"] = dict({k: v for k, v in det["cluster"].items() if k != "index"}, eps=a.cluster_eps, min_points=a.cluster_min_points)
    if "clean" in det:
        line["clean"] = {k: det["clean"][k] for k in ("welded_vertices", "clusters", "degenerate", "boundary_edges", "nonmanifold_edges",
                                                      "n_min")}
        line["clean"]["triangles_kept"] = int(faces.shape[0])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
