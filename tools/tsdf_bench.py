#!/usr/bin/env python3
"""Times the TSDF volume (splat_loam_amd.tsdf -> sls_tsdf_blocks / sls_tsdf_integrate / sls_tsdf_extract_*) and
meshing.mesh_tsdf, and checks the native integration against a torch restatement of the same rule:

    python tools/tsdf_bench.py [--voxel 0.25] [--reps 10] [--out FILE.json]

Data: the synthetic graph of tools/sample_surface.py --probe (8 keyframes, 64 x 1024, 50 000 surfels).

  integrate   one keyframe into the volume: sls_tsdf_integrate against the same rule written with torch (voxel centres,
              the view transform, atan2 / asin, floor, a gather of four planes, torch.where) — float32 on both sides, so
              the two agree except where torch's atan2 / asin and the header's polynomial put a voxel into different
              pixels; the share of voxels whose weight differs is reported
  extract     TsdfVolume.extract alone (count, one host read, emit)
  mesh_tsdf   the whole graph -> mesh
  there is no earlier implementation to race: the torch restatement is what a user without the native call would write.
Both sides of `integrate` run in one process and alternate; 3 warm-ups, the median of --reps (>= 10),
torch.cuda.synchronize inside the timed region.  evaluate_recon(reference = the sample_surface cloud, the mesh) is
recorded, not judged."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from sample_surface import write_synthetic_results
from splat_loam_amd import _abi, evaluation, meshing, traj_io, tsdf


def torch_integrate(vol, tsdf_t, weight_t, allmap, cam, min_opacity, max_depth_dist, depth_ratio):
    """The rule of include/sls_tsdf_math.h with torch operations; returns the new (tsdf, weight)."""
    dev = allmap.device
    _, H, W = allmap.shape
    l = torch.arange(512, device=dev)
    local = torch.stack([l & 7, (l >> 3) & 7, l >> 6], 1)
    g = (8 * vol.blocks.long()[:, None, :] + local[None]).double()
    origin = torch.tensor(vol.origin, dtype=torch.float64, device=dev)
    c = (origin + (g + 0.5) * vol.voxel_size).float()
    R = torch.tensor(list(cam.Rvw), dtype=torch.float32, device=dev).view(3, 3)
    t = torch.tensor(list(cam.tvw), dtype=torch.float32, device=dev)
    q = c @ R.T + t
    rho = q.norm(dim=2)
    az = torch.atan2(q[..., 1], q[..., 0])
    el = torch.asin((q[..., 2] / rho).clamp(-1.0, 1.0))
    col = torch.floor(cam.fx * az + cam.cx + 1.0).long()
    row = torch.floor(cam.fy * el + cam.cy + 1.0).long()
    if cam.wrap:
        col = col % W
    ok = (rho >= cam.near_cut) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    px = torch.where(ok, row * W + col, torch.zeros_like(col))
    flat = allmap.reshape(7, -1)
    D, alpha, med, dist = flat[0][px], flat[1][px], flat[5][px], flat[6][px]
    ok &= ~(alpha < min_opacity) & ~(dist > max_depth_dist)
    depth = torch.where(alpha > 0, D / alpha, D) * (1.0 - depth_ratio) + med * depth_ratio
    sdf = depth - rho
    trunc = float(np.float32(vol.trunc))
    ok &= (depth > 0) & (sdf >= -trunc)
    tv = (sdf / trunc).clamp_max(1.0)
    return torch.where(ok, (tsdf_t * weight_t + tv) / (weight_t + 1.0), tsdf_t), torch.where(ok, weight_t + 1.0, weight_t)


def timed(fn, reps, dev, warm=3):
    times = []
    for it in range(warm + reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize(dev)
        if it >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
        del res
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--voxel", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18a_tsdf_mesh.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("tsdf_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lib = _abi.lib()
    H, W, n_frames, n_surfels = 64, 1024, 8, 50000
    res = {"what": "tsdf.TsdfVolume.integrate / extract (sls_tsdf_integrate, sls_tsdf_extract_count / _emit) and meshing.mesh_tsdf",
           "data": "synthetic", "image": [H, W], "surfels": n_surfels, "keyframes": n_frames, "voxel_size": a.voxel, "trunc": 4 * a.voxel,
           "protocol": f"one process, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region; integrate: native and "
                       "torch alternating", "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        write_synthetic_results(d, n_frames, H, W, n_surfels)
        vertices, faces, det = meshing.mesh_tsdf(d, a.voxel, seed=1, device=dev, details=True)
        vol = det["volume"]
        B = det["blocks"]
        res.update({"blocks": B, "volume_bytes": det["volume_bytes"], "triangles": det["triangles"], "samples": det["samples"],
                    "first_call_stage_ms": det["stage_ms"]})
        # one keyframe, rendered once: the camera as TsdfVolume.integrate composes it
        graph = traj_io.read_graph(os.path.join(d, "graph.yaml"))
        pose = meshing._pose44(graph["frames"][0]["model_T_frame"])
        _, _, camera, allmap = next(meshing._render_keyframes(meshing.Path(d), graph, [(0, 0)], [pose], H, W, dev))
        from splat_loam_amd.rasterizer import GaussianRasterizationSettings, get_camera
        ce = get_camera(GaussianRasterizationSettings(H, W, 1.0, camera.world_view_transform, camera.projection_matrix), dev)
        cam = _abi.SlsCamera()
        C.memmove(C.byref(cam), C.byref(ce.cam), C.sizeof(cam))
        view = np.eye(4, dtype=np.float32)
        view[:3, :3], view[:3, 3] = np.asarray(ce.cam.Rvw, np.float32).reshape(3, 3), np.asarray(ce.cam.tvw, np.float32)
        m = tsdf.compose_volume_to_view(graph["models"][0]["world_T_model"], view)
        for i in range(3):
            for j in range(3):
                cam.Rvw[3 * i + j] = float(m[4 * i + j])
            cam.tvw[i] = float(m[4 * i + 3])
        t0, w0 = torch.ones_like(vol.tsdf), torch.zeros_like(vol.weight)
        tn, wn = t0.clone(), w0.clone()
        st = torch.cuda.current_stream(dev).cuda_stream

        def native():
            _abi.check(lib.sls_tsdf_integrate(C.byref(cam), B, vol.blocks.data_ptr(), tn.data_ptr(), wn.data_ptr(), allmap.data_ptr(),
                                              vol.voxel_size, vol.trunc, vol.origin.ctypes.data, 0.5, 0.1, 0.0, st), "sls_tsdf_integrate")

        def composed():
            return torch_integrate(vol, t0, w0, allmap, cam, 0.5, 0.1, 0.0)

        t_nat, t_tor = [], []
        for it in range(3 + a.reps):
            for fn, acc in ((native, t_nat), (composed, t_tor)):
                torch.cuda.synchronize(dev)
                s = time.perf_counter()
                out = fn()
                torch.cuda.synchronize(dev)
                if it >= 3:
                    acc.append((time.perf_counter() - s) * 1e3)
                del out
        stat = lambda t: {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
        tn.copy_(t0)
        wn.copy_(w0)
        native()
        tt, wt = composed()
        same = wt == wn
        res["integrate"] = {"voxels": B * 512, "native_ms": stat(t_nat), "torch_ms": stat(t_tor),
                            "bytes_moved_native": B * 512 * 16, "observed_voxels": int((wn > 0).sum()),
                            "weights_that_differ": int((~same).sum()), "share_that_differs": float((~same).float().mean()),
                            "tsdf_max_abs_difference_where_weights_agree": float((tt - tn)[same].abs().max())}
        res["extract_ms"] = timed(lambda: vol.extract(), a.reps, dev)
        pts, _ = meshing.sample_surface(d, seed=1, device=dev)
        res["allocate_blocks_ms"] = timed(lambda: tsdf.allocate_blocks(pts, a.voxel, 4 * a.voxel), a.reps, dev)
        res["mesh_tsdf_ms"] = timed(lambda: meshing.mesh_tsdf(d, a.voxel, seed=1, device=dev), a.reps, dev, warm=1)
        rec = evaluation.evaluate_recon(pts, vertices, faces, mesh_sample_point=1_000_000, seed=1)
        res["evaluate_recon_against_the_sampled_cloud"] = {k: (float(v) if isinstance(v, (int, float)) else v) for k, v in rec.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
