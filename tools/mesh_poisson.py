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

import mesh_cli
from splat_loam_amd import meshing, ply_io, tsdf


def build_parser():
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
    ap.add_argument("--weld", action="store_true", help="merge bit-equal vertices before writing")
    mesh_cli.add_sample_arguments(ap)
    mesh_cli.add_cloud_arguments(ap)
    mesh_cli.add_clean_arguments(ap)
    return ap


def main():
    a = build_parser().parse_args()
    *mesh, det = meshing.mesh_poisson(a.results_dir, a.voxel, margin=a.margin, screening=a.screening, iterations=a.iterations, tol=a.tol,
                                      min_density=a.min_density, min_density_quantile=a.min_density_quantile,
                                      density_sweeps=a.density_sweeps, device=a.device, details=True,
                                      **mesh_cli.sample_options(a), **mesh_cli.clean_options(a))
    vertices, faces, normals = mesh[0], mesh[1], (mesh[2] if a.normals else None)
    if a.weld and "clean" not in det:
        vertices, faces = tsdf.weld_soup(vertices)
    ply_io.save_mesh(a.out_ply, vertices, faces, normals=normals)
    line = {"blocks": det["blocks"], "samples": det["samples"], "triangles": det["triangles"], "vertices": int(vertices.shape[0]),
            "keyframes": len(det["frame_ids"]), "solve": det["solve"], "min_density": det["min_density"],
            "stage_ms": {k: round(v, 3) for k, v in det["stage_ms"].items()}, "out": a.out_ply}
    line.update(mesh_cli.cloud_report(det, a))
    if "clean" in det:
        line["clean"] = mesh_cli.clean_report(det, a, faces)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
