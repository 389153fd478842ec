#!/usr/bin/env python3
"""The reference's `evaluate_recon` (utils/eval_utils.py:67-154) for a reference point cloud and an estimated triangle
mesh, on the device (splat_loam_amd.evaluation.evaluate_recon), one JSON line with the reference's keys and units:

    python tools/eval_recon.py REFERENCE.ply MESH.ply [--down-sample-res 0.02] [--threshold 0.2] [--truncation-acc 0.5]
                               [--truncation-com 0.5] [--mesh-sample-point 10000000] [--seed 0] [--crop-to-reference]
                               [--align D [--align-iterations 30] [--align-method plane|point]]
                               [--exact-completeness] [--error-map PREFIX] [--signed]

REFERENCE.ply: binary little-endian PLY with `x y z` as float or double.  MESH.ply: binary little-endian PLY with a
`vertex` element and one `face` element of triangles (`list uchar int vertex_indices`: what Open3D writes for a Poisson
mesh).  The defaults are the reference's.  --crop-to-reference samples only the faces inside the reference cloud's
bounding box (z padded by the voxel size): what the reference intended but does not do, so it is off by default.
--align D first registers the mesh's vertices onto the reference cloud (evaluation.register_icp: ICP on exact nearest
neighbours, pairs farther apart than D metres ignored; no global registration — the mesh must already lie within D of the
cloud) and evaluates the moved mesh; the line then holds "Alignment": the pose in KITTI order (12 numbers, row-major 3x4
reference_T_mesh), fitness, inlier_rmse, updates and the flags.  Without it nothing changes.
--exact-completeness measures every reference point against the mesh itself (evaluation.point_to_mesh), not against its
nearest sample: the completeness then depends neither on --seed nor on --mesh-sample-point.  --error-map PREFIX writes
PREFIX_accuracy.ply, the mesh with its vertices coloured by their distance to the reference cloud (red at
--truncation-acc), and PREFIX_completeness.ply, the evaluated reference points coloured by their exact distance to the mesh
(red at --truncation-com); green is good, yellow is half the truncation.  Without either nothing changes.
--signed adds "Signed": the mean SIGNED distance of the evaluated reference points to the mesh (evaluation.signed_distance;
positive: the point lies in front of the faces — for a mesh of mesh_tsdf / mesh_poisson the observed side, so a positive
mean says the mesh sits behind the true surface), the share of points behind the mesh, and the facts about the mesh the
sign depends on; with --error-map also PREFIX_signed.ply, the reference points white on the surface, red in front of it,
blue behind it.  Without it nothing changes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from splat_loam_amd import evaluation, ply_io


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reference_ply")
    ap.add_argument("mesh_ply")
    ap.add_argument("--down-sample-res", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--truncation-acc", type=float, default=0.5)
    ap.add_argument("--truncation-com", type=float, default=0.5)
    ap.add_argument("--mesh-sample-point", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--crop-to-reference", action="store_true")
    ap.add_argument("--align", type=float, default=None, metavar="D", help="register the mesh to the reference first, gate D metres")
    ap.add_argument("--align-iterations", type=int, default=30)
    ap.add_argument("--align-method", choices=("plane", "point"), default="plane")
    ap.add_argument("--exact-completeness", action="store_true")
    ap.add_argument("--error-map", default=None, metavar="PREFIX")
    ap.add_argument("--signed", action="store_true")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    align = None
    if a.align is not None:
        align = dict(max_distance=a.align, iterations=a.align_iterations, method=a.align_method, seed=a.seed)
        evaluation._check_icp_args(a.align, a.align_iterations, a.align_method, None, {})     # before the files are read
    dev = torch.device(a.device)
    reference = torch.from_numpy(ply_io.load_point_cloud(a.reference_ply)[0]).to(dev)
    vertices, faces = ply_io.load_mesh(a.mesh_ply)
    res = evaluation.evaluate_recon(
        reference, torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev), down_sample_res=a.down_sample_res,
        threshold=a.threshold, truncation_acc=a.truncation_acc, truncation_com=a.truncation_com,
        crop_to_reference=a.crop_to_reference, mesh_sample_point=a.mesh_sample_point, seed=a.seed, align=align,
        completeness="exact" if a.exact_completeness else "sampled", error_map=a.error_map is not None,
        signed=a.signed)
    if a.error_map is not None:
        em = res.pop("ErrorMap")
        ply_io.save_mesh(a.error_map + "_accuracy.ply", em["vertices"], faces, colors=em["vertex_colors"])
        ply_io.save_point_cloud(a.error_map + "_completeness.ply", em["points"], torch.zeros_like(em["points"]), em["point_colors"])
        if a.signed:
            ply_io.save_point_cloud(a.error_map + "_signed.ply", em["points"], torch.zeros_like(em["points"]), em["point_colors_signed"])
    if align is not None:
        al = res["Alignment"]
        al["target_T_source"] = al["target_T_source"][:3].reshape(-1).tolist()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
