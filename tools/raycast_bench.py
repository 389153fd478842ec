#!/usr/bin/env python3
"""Times range images of a mesh (splat_loam_amd.evaluation.mesh_ray_index -> sls_mesh_rayindex_build, cast_rays ->
sls_mesh_raycast) against a chunked torch Moller-Trumbore brute force on the synthetic cleaned mesh of the other mesh
benches, and checks first that they agree:

    python tools/raycast_bench.py [--images 64x1024 64x2048] [--reps 10] [--torch-chunks 2] [--out FILE.json]

Mesh: `mesh_clean_bench.synthetic_volume` (a sphere of radius 10 m at 0.1 m voxels with floaters) extracted and cleaned:
about 1.13 M triangles.  Rays: the half-pixel rays of a spherical sensor (`renderer.pixel_rays`) INSIDE the sphere, off its
centre — a range image from inside, coherent rays in row-major order, what `render_mesh` casts.  The index build and the
cast are timed separately (`index_build_ms`: mesh_ray_index with its host read; `cast_ms`: cast_rays against that index,
t + face, with its host read).

torch brute force: --torch-rows rays x ALL faces per chunk, float32 Moller-Trumbore, the nearest hit over the faces.  It
costs rays x F intersections, so only --torch-chunks chunks are timed, on the FIRST rays of the image, and the file says
how many: `torch_ms` is the time measured for those rays alone, `torch_ms_all_rays_extrapolated` scales it by rays / rays
timed.  The native call always casts all rays.

Asserted before anything is timed: two native casts give equal bytes; every ray hits (the mesh is closed around the
sensor); on the brute force's rays, in float64, wherever the winning face is clear (its smallest barycentric weight and
|cos| to the ray at least 1e-3, the runner-up's t at least 1e-4 t farther) the native call names that face and
|t - t64| <= 1e-5 t.  One process, both sides alternating, 3 warm-ups, the median of --reps (>= 10),
torch.cuda.synchronize inside the timed region."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from mesh_clean_bench import alternate, synthetic_volume
from splat_loam_amd import evaluation, mesh_ops, synth
from splat_loam_amd.renderer import pixel_rays
from splat_loam_amd.scene import Camera


def brute_force(o, d, a, e1, e2, dtype):
    """(rows,) nearest t over all faces (+inf: none), (rows,) its face, (rows, F) all t, smallest weight and |cos| of the
    winner: o, d (rows,3); a, e1 = b - a, e2 = c - a (F,3)"""
    o, d, a, e1, e2 = (x.to(dtype) for x in (o, d, a, e1, e2))
    p = torch.linalg.cross(d[:, None].expand(-1, a.shape[0], -1), e2[None].expand(d.shape[0], -1, -1))        # (rows, F, 3)
    det = (e1[None] * p).sum(-1)
    s = o[:, None] - a[None]
    u = (s * p).sum(-1) / det
    q = torch.linalg.cross(s, e1[None].expand_as(s))
    v = (d[:, None] * q).sum(-1) / det
    t = (e2[None] * q).sum(-1) / det
    hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (det != 0)
    t = torch.where(hit, t, torch.full_like(t, float("inf")))
    best, face = t.min(dim=1)
    rows = torch.arange(len(o), device=o.device)
    wmin = torch.minimum(torch.minimum(u[rows, face], v[rows, face]), 1 - u[rows, face] - v[rows, face])
    n = torch.linalg.cross(e1[face], e2[face])
    cos = (n * d).sum(-1).abs() / (n.norm(dim=1) * d.norm(dim=1))
    second = t.scatter(1, face[:, None], float("inf")).min(dim=1).values
    return best, face, wmin, cos, second


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--images", nargs="+", default=["64x1024", "64x2048"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-rows", type=int, default=16)
    ap.add_argument("--torch-chunks", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35a_raycast.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("raycast_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        soup, faces = synthetic_volume(a.radius, a.voxel, a.floaters, dev).extract()
        v, f = mesh_ops.clean_mesh(soup, faces, normals=False)
        del soup, faces
        va = v[f[:, 0].long()].contiguous()
        e1, e2 = (v[f[:, 1].long()] - va).contiguous(), (v[f[:, 2].long()] - va).contiguous()
        res = {"what": "evaluation.mesh_ray_index (sls_mesh_rayindex_build) and evaluation.cast_rays against it (sls_mesh_raycast, all "
                       "rays, t + face) vs a chunked torch Moller-Trumbore brute force (torch_ms covers torch_rays_timed rays only)",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "vertices": int(v.shape[0]),
               "triangles": int(f.shape[0]),
               "protocol": f"one process, all sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the "
                           "timed region; agreement asserted first",
               "box_order": "index order (the only one built)",
               "device": torch.cuda.get_device_name(0), "images": []}
        pose = np.eye(4)
        pose[:3, 3] = [0.3 * a.radius, -0.2 * a.radius, 0.1 * a.radius]
        n_timed = a.torch_rows * a.torch_chunks
        for image in a.images:
            H, W = (int(x) for x in image.split("x"))
            cam = Camera(synth.spherical_K(H, W), torch.zeros((1, H, W), device=dev), world_T_lidar=pose, data_device=dev)
            d = pixel_rays(cam).reshape(-1, 3).contiguous()
            o = torch.tensor(pose[:3, 3], dtype=torch.float32, device=dev).expand_as(d).contiguous()
            index = evaluation.mesh_ray_index(v, f)

            def build():
                return evaluation.mesh_ray_index(v, f)

            def cast():
                return evaluation.cast_rays(o, d, v, f, index=index)

            def torch_side():
                return [brute_force(o[i:i + a.torch_rows], d[i:i + a.torch_rows], va, e1, e2, torch.float32)[:2]
                        for i in range(0, n_timed, a.torch_rows)]

            t, face = cast()
            t2, face2 = cast()
            assert torch.equal(t.view(torch.int32), t2.view(torch.int32)) and torch.equal(face, face2), "two native casts differ"
            assert bool((face >= 0).all()), f"{int((face < 0).sum())} rays left the closed mesh"
            n_clear, worst = 0, 0.0
            for i in range(0, n_timed, a.torch_rows):
                t64, f64, wmin, cos, second = brute_force(o[i:i + a.torch_rows], d[i:i + a.torch_rows], va, e1, e2, torch.float64)
                clear = (wmin >= 1e-3) & (cos >= 1e-3) & (second >= t64 * (1 + 1e-4)) & torch.isfinite(t64)
                n_clear += int(clear.sum())
                mine_f, mine_t = face[i:i + a.torch_rows][clear], t[i:i + a.torch_rows][clear].double()
                assert torch.equal(mine_f.long(), f64[clear]), "a clear first hit is named differently"
                if n_clear:
                    worst = max(worst, float(((mine_t - t64[clear]).abs() / t64[clear]).max()) if clear.any() else 0.0)
            assert n_clear >= n_timed // 2 and worst <= 1e-5, (n_clear, worst)
            t_build, t_cast, t_tor = alternate([build, cast, torch_side], a.reps, dev)
            rays = H * W
            row = {"image": image, "rays": rays, "index_build_ms": t_build, "cast_ms": t_cast, "torch_ms": t_tor,
                   "torch_rays_timed": n_timed, "torch_chunk_rows": a.torch_rows,
                   "torch_ms_all_rays_extrapolated": t_tor["median"] * rays / n_timed,
                   "cast_faster_than_torch_extrapolated": bool(t_cast["median"] < t_tor["median"] * rays / n_timed),
                   "build_plus_cast_faster_than_torch_extrapolated": bool(t_build["median"] + t_cast["median"] < t_tor["median"] * rays / n_timed),
                   "mrays_per_s": rays / t_cast["median"] / 1e3, "clear_rays_checked": n_clear, "t_error_relative_float64_max": worst,
                   "mean_range_m": float(t.mean())}
            res["images"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
