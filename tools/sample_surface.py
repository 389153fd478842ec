#!/usr/bin/env python3
"""From a results directory (graph.yaml, models/*.ply, optionally cfg.yaml) to the oriented point cloud Poisson
reconstruction takes — the reference's `run.py mesh` up to the Poisson solve (scene/postprocessing.py:93-190):

    python tools/sample_surface.py RESULTS_DIR OUT.ply [--kf-interval N] [--kf-samples K] [--min-opacity A]
                                   [--max-depth-dist D] [--use-median-depth] [--seed S] [--image-height H --image-width W]
                                   [--outlier-nb 20 [--outlier-std 2.0]] [--cluster-eps E [--cluster-min-points 10]]

--outlier-nb K filters the merged cloud with `evaluation.remove_statistical_outlier(K, --outlier-std)`: the call the
reference makes at this place (postprocessing.py:192) and whose result it discards.  --cluster-eps E then keeps the
largest DBSCAN cluster of the cloud (`evaluation.keep_clusters(E, --cluster-min-points)`: E a few sample spacings).  OUT.ply holds float32 `x y z nx ny nz`; elsewhere: `o3d.io.read_point_cloud(OUT.ply)` and
`o3d.geometry.TriangleMesh.create_from_point_cloud_poisson(pcd, depth=...)`.

    python tools/sample_surface.py --probe [--probe-out FILE.json]

times, in one process, the device path against the torch composition of the reference's shape (render, boolean gather,
.cpu(), np.random.choice) over a synthetic graph of 8 keyframes, 64 x 1024, 50 000 surfels: per keyframe, the median of
20 after 3 warm-ups, torch.cuda.synchronize around each keyframe."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import mesh_cli
from splat_loam_amd import meshing, ply_io, synth, traj_io


def write_synthetic_results(d, n_frames=8, H=64, W=1024, n_surfels=50000, seed=5):
    K = synth.spherical_K(H, W)
    sc = synth.make_scene(n_surfels, H, W, seed=seed, range_lo=2.0, range_hi=40.0, scale_lo=0.05, scale_hi=0.3, opac_lo=0.5)
    ply_io.save_ply(os.path.join(d, "models", "model_0.ply"), sc["means"], np.log(sc["opac"] / (1 - sc["opac"])),
                    np.log(sc["scales"]), sc["rots"])
    poses = synth.keyframe_poses(n_frames)
    world_T_model = np.eye(4)
    world_T_model[:3, 3] = [100.0, -40.0, 3.0]
    models = [{"id": 0, "world_T_model": world_T_model, "filename": "models/model_0.ply", "frame_ids": list(range(n_frames))}]
    frames = [{"id": i, "timestamp": 0.1 * i, "model_T_frame": poses[i], "projmatrix": [K[0, 0], K[1, 1], K[0, 2], K[1, 2]],
               "model_id": 0} for i in range(n_frames)]
    traj_io.write_graph(os.path.join(d, "graph.yaml"), models, frames)
    with open(os.path.join(d, "cfg.yaml"), "w") as f:
        f.write(f"preprocessing:\n  image_height: {H}\n  image_width: {W}\n")


def probe(out_file, kf_samples=5000, min_opacity=0.5, max_depth_dist=0.1):
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from splat_loam_amd.renderer import depth_to_points, render
    from splat_loam_amd.scene import Camera, SurfelModel
    dev = torch.device("cuda:0")
    H, W, n_frames, n_surfels = 64, 1024, 8, 50000
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        write_synthetic_results(d, n_frames, H, W, n_surfels)
        graph = traj_io.read_graph(os.path.join(d, "graph.yaml"))
        raw = ply_io.load_ply(os.path.join(d, graph["models"][0]["filename"]))
        gm = SurfelModel(*(np.array(raw[n]) for n in ("xyz", "scaling", "rotation", "opacity")), device=dev)
        act = (gm.get_xyz.detach(), gm.get_opacity.detach(), gm.get_scaling.detach(), gm.get_rotation.detach())
        world_T_model = meshing._pose44(graph["models"][0]["world_T_model"])
        cams = []
        for fr in graph["frames"]:
            fx, fy, cx, cy = fr["projmatrix"]
            cams.append(Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32), np.zeros((1, H, W), np.float32), None,
                               np.zeros((1, H, W), np.uint8), meshing._pose44(fr["model_T_frame"]), data_device=dev))
        Ms = torch.from_numpy(np.stack([meshing.compose_cam_to_world(
            world_T_model, np.linalg.inv(meshing._pose44(fr["model_T_frame"])).astype(np.float32)) for fr in graph["frames"]])).to(dev)
        slab = (torch.empty((kf_samples, 3), device=dev), torch.empty((kf_samples, 3), device=dev), None,
                torch.zeros((4,), dtype=torch.int32, device=dev))

        def device_path(i):
            cam = cams[i]
            settings = GaussianRasterizationSettings(H, W, 1.0, cam.world_view_transform, cam.projection_matrix, lean_allmap=False)
            _, allmap = GaussianRasterizer(raster_settings=settings)(means3D=act[0], means2D=act[0], opacities=act[1],
                                                                     scales=act[2], rotations=act[3])
            meshing.sample_keyframe(allmap, cam, None, kf_samples=kf_samples, min_opacity=min_opacity,
                                    max_depth_dist=max_depth_dist, seed=1, frame_id=i, out=slab, cam_to_world=Ms[i])

        def torch_composition(i):          # postprocessing.py:162-188 with this tree's public functions
            cam = cams[i]
            pkg = render(cam, gm, 0.0)
            depth, normals = pkg["surf_depth"].clone(), pkg["rend_normal"].clone()
            invalid = ((pkg["rend_alpha"] < min_opacity) | (pkg["rend_dist"] > max_depth_dist))[0]
            depth[..., invalid] = 0.0
            normals[..., invalid] = 0.0
            xyz = depth_to_points(cam, depth, True)[..., ~invalid].T.cpu().numpy()
            nxyz = normals[..., ~invalid].T.cpu().numpy()
            idx = np.random.choice(xyz.shape[0], kf_samples)
            xyz, nxyz = xyz[idx], nxyz[idx]
            return xyz @ world_T_model[:3, :3].T + world_T_model[:3, 3], nxyz @ world_T_model[:3, :3].T

        def timed(fn):
            times = []
            for it in range(23):
                i = it % n_frames
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn(i)
                torch.cuda.synchronize(dev)
                if it >= 3:
                    times.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(times)), float(np.min(times)), float(np.max(times))
        dev_ms = timed(device_path)
        ref_ms = timed(torch_composition)
        whole = []
        for _ in range(5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            pts, _ = meshing.sample_surface(d, kf_samples=kf_samples, min_opacity=min_opacity, max_depth_dist=max_depth_dist, seed=1,
                                            device=dev)
            torch.cuda.synchronize(dev)
            whole.append((time.perf_counter() - t0) * 1e3)
    res = {"what": "per keyframe: rasterizer forward + sls_surface_samples vs render + boolean gather + .cpu() + np.random.choice",
           "data": "synthetic", "image": [H, W], "surfels": n_surfels, "keyframes": n_frames, "kf_samples": kf_samples,
           "protocol": "median of 20 after 3 warm-ups, torch.cuda.synchronize around each keyframe, one process",
           "device_path_ms_per_keyframe": {"median": dev_ms[0], "min": dev_ms[1], "max": dev_ms[2]},
           "torch_composition_ms_per_keyframe": {"median": ref_ms[0], "min": ref_ms[1], "max": ref_ms[2]},
           "sample_surface_whole_graph_ms": {"median": float(np.median(whole[1:])), "first": whole[0], "rows": int(pts.shape[0])},
           "launches_per_keyframe_after_forward": 2, "host_reads_per_keyframe_after_forward": 0,
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("results_dir", nargs="?")
    ap.add_argument("out_ply", nargs="?")
    mesh_cli.add_sample_arguments(ap)
    mesh_cli.add_cloud_arguments(ap)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--probe-out", default=os.path.join(ROOT, "profiles", "r13a_surface_samples.json"))
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    if a.probe:
        probe(a.probe_out)
        return
    if not a.results_dir or not a.out_ply:
        ap.error("RESULTS_DIR and OUT.ply are required (or --probe)")
    pts, nrm, det = meshing.sample_surface(a.results_dir, device=a.device, details=True, **mesh_cli.sample_options(a))
    ply_io.save_point_cloud(a.out_ply, pts, nrm)
    empty = [f for f, kept in zip(det["frame_ids"], det["kept"]) if not kept]
    print(f"{pts.shape[0]} oriented points from {int(det['kept'].sum())} of {len(det['frame_ids'])} keyframes "
          f"(seed {det['seed']}) -> {a.out_ply}" + (f"; no valid pixel in frames {empty}" if empty else "") +
          (f"; {det['outlier']['removed']} outliers removed (threshold {det['outlier']['threshold']:.4f} m)" if "outlier" in det else "") +
          (f"; {det['cluster']['removed']} points outside the largest of {det['cluster']['clusters']} clusters removed" if "cluster" in det else ""))


if __name__ == "__main__":
    main()
