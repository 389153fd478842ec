#!/usr/bin/env python3
"""Times the voxel down-sampling, the mesh sampling and the whole of evaluate_recon (splat_loam_amd.evaluation ->
sls_voxel_downsample, sls_mesh_sample) against torch compositions written here, and checks that both compute the same:

    python tools/recon_bench.py [--voxel-sizes 2000000 10000000] [--samples 10000000] [--reps 10] [--out FILE.json]

Data: the synthetic room of tools/nn_bench.py (40 x 24 x 6 m, 16 keyframes, 1 cm of noise) as the cloud; the room's own
six faces as a mesh of about one million triangles (cells of 7.33 cm), its vertices moved by up to 1 cm.

torch compositions (what a user without the native calls would write):
  voxels    the same float64 index arithmetic, torch.unique(key, return_inverse=True, return_counts=True), index_add_ of
            the float64 points, a division (float64 atomics: the last bits of its sums change from run to run)
  sampling  float64 areas, cumsum, torch.rand, searchsorted, the same point formula
  whole     the two compositions above in front of evaluation.cloud_metrics (the nearest-neighbour search has no torch
            counterpart at this size: tools/nn_bench.py)
Both sides run in one process and alternate; 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize inside the
timed region; host reads included on both sides (the native calls read their status words, torch.unique reads its
count).  Where the two down-samplings are compared, np.unique on the host is the referee (`*_counts_equal_numpy`: at
10 M points the torch composition's counts are the ones that differ from it).  The stages of the native down-sampling are timed in a pass of their own with the library's event timer
(sls_timing_enable): the 63-bit sort is 18 of its 25 launches."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from nn_bench import ROOM_MAX, ROOM_MIN, room_cloud
from splat_loam_amd import _abi, evaluation


def room_mesh(cell=0.0733, seed=5):
    """The six faces of the room as grids of `cell`-sized quads, two triangles each; vertices jittered by up to 1 cm."""
    rng = np.random.default_rng(seed)
    vertices, faces, base = [], [], 0
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        nu = max(1, int(round((ROOM_MAX[u] - ROOM_MIN[u]) / cell)))
        nv = max(1, int(round((ROOM_MAX[v] - ROOM_MIN[v]) / cell)))
        gu, gv = np.meshgrid(np.linspace(ROOM_MIN[u], ROOM_MAX[u], nu + 1), np.linspace(ROOM_MIN[v], ROOM_MAX[v], nv + 1), indexing="ij")
        i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
        a = (i * (nv + 1) + j).ravel()
        quad = np.stack([a, a + nv + 1, a + nv + 2, a, a + nv + 2, a + 1], 1).reshape(-1, 3)
        for side in (ROOM_MIN[axis], ROOM_MAX[axis]):
            p = np.empty((gu.size, 3))
            p[:, u], p[:, v], p[:, axis] = gu.ravel(), gv.ravel(), side
            vertices.append(p)
            faces.append(quad + base)
            base += gu.size
    vertices = np.concatenate(vertices)
    vertices += rng.uniform(-0.01, 0.01, vertices.shape)
    return vertices.astype(np.float32), np.concatenate(faces).astype(np.int32)


def torch_voxels(points, vs):
    o = points.amin(0).double() - 0.5 * vs
    idx = torch.floor((points.double() - o) / vs).long()
    key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
    _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
    sums = torch.zeros((counts.shape[0], 3), dtype=torch.float64, device=points.device).index_add_(0, inverse, points.double())
    return (sums / counts[:, None].double()).float(), counts


def torch_sample(vertices, faces, n, gen):
    f = faces.long()
    v0, v1, v2 = vertices[f[:, 0]].double(), vertices[f[:, 1]].double(), vertices[f[:, 2]].double()
    area = 0.5 * torch.linalg.cross(v1 - v0, v2 - v0).norm(dim=1)
    cdf = torch.cumsum(area, 0)
    u = torch.rand((n,), dtype=torch.float64, device=vertices.device, generator=gen) * cdf[-1]
    face = torch.searchsorted(cdf, u, right=True).clamp_max(f.shape[0] - 1)
    r = torch.rand((2, n), dtype=torch.float32, device=vertices.device, generator=gen)
    s = torch.sqrt(r[0])
    g = f[face]
    return ((1 - s)[:, None] * vertices[g[:, 0]] + (s * (1 - r[1]))[:, None] * vertices[g[:, 1]]) + (s * r[1])[:, None] * vertices[g[:, 2]], face


def alternate(native, composed, reps, dev):
    t_nat, t_tor = [], []
    for it in range(3 + reps):
        for fn, acc in ((native, t_nat), (composed, t_tor)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize(dev)
            if it >= 3:
                acc.append((time.perf_counter() - t0) * 1e3)
            del res
    stat = lambda t: {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
    return {"native_ms": stat(t_nat), "torch_ms": stat(t_tor), "native_faster_than_torch": bool(np.median(t_nat) < np.median(t_tor))}


def native_stages(fn, dev, runs=3):
    """Per-slot milliseconds of one call (the library's event timer, in a pass of its own)."""
    lib = _abi.lib()
    lib.sls_timing_enable(1)
    for _ in range(runs):
        fn()
    torch.cuda.synchronize(dev)
    ns = lib.sls_timing_slots()
    tot, cnt = (C.c_double * ns)(), (C.c_int64 * ns)()
    lib.sls_timing_collect(tot, cnt)
    lib.sls_timing_enable(0)
    return {lib.sls_timing_name(s).decode(): {"ms_per_call": tot[s] / runs, "launches_per_call": int(cnt[s]) // runs} for s in range(ns) if cnt[s]}


def bench_voxels(M, vs, reps, dev):
    points = torch.from_numpy(room_cloud(M, seed=1, noise=0.01)).to(dev)
    res = {"M": M, "voxel_size": vs}
    res.update(alternate(lambda: evaluation.voxel_down_sample(points, vs, return_counts=True), lambda: torch_voxels(points, vs), reps, dev))
    rows, counts = evaluation.voxel_down_sample(points, vs, return_counts=True)
    rows2, _ = evaluation.voxel_down_sample(points, vs, return_counts=True)
    trows, tcounts = torch_voxels(points, vs)
    res["n_voxels"] = int(rows.shape[0])
    res["same_voxels_and_counts"] = bool(rows.shape == trows.shape and torch.equal(counts.long(), tcounts))
    if res["same_voxels_and_counts"]:
        res["centroid_max_abs_difference"] = float((rows - trows).abs().max())
    # the referee: the same keys and np.unique on the host, once
    p = points.cpu().numpy()
    idx = np.floor((p.astype(np.float64) - (p.min(0).astype(np.float64) - 0.5 * vs)) / vs).astype(np.uint64)
    _, ref_counts = np.unique(idx[:, 0] | (idx[:, 1] << np.uint64(21)) | (idx[:, 2] << np.uint64(42)), return_counts=True)
    for name, c in (("native", counts), ("torch", tcounts)):
        c = c.cpu().numpy()
        res[f"{name}_counts_equal_numpy"] = bool(len(c) == len(ref_counts) and (c == ref_counts).all())
    res["native_bits_repeat"] = bool(torch.equal(rows.view(torch.int32), rows2.view(torch.int32)))
    stages = native_stages(lambda: evaluation.voxel_down_sample(points, vs, return_counts=True), dev)
    sort_ms = sum(v["ms_per_call"] for k, v in stages.items() if k.startswith("sort_"))
    res["native_sort_stages"] = stages
    res["native_sort_ms"] = sort_ms
    res["native_sort_share_of_call"] = sort_ms / res["native_ms"]["median"]
    return res


def bench_sampling(vertices, faces, n, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"V": int(vertices.shape[0]), "F": int(faces.shape[0]), "n_samples": n}
    res.update(alternate(lambda: evaluation.sample_mesh(vertices, faces, n, seed=1, return_faces=True),
                         lambda: torch_sample(vertices, faces, n, gen), reps, dev))
    pts, face = evaluation.sample_mesh(vertices, faces, n, seed=1, return_faces=True)
    tpts, tface = torch_sample(vertices, faces, n, gen)
    # the same distribution: the share of the samples in each of 64 equal runs of faces, and the clouds' means
    bins = lambda f: torch.bincount((f.long() * 64) // faces.shape[0], minlength=64).double() / n
    res["face_share_max_difference_64_bins"] = float((bins(face) - bins(tface)).abs().max())
    res["cloud_mean_difference_m"] = float((pts.double().mean(0) - tpts.double().mean(0)).abs().max())
    return res


def bench_whole(reference, vertices, faces, n, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(2)

    def composed():
        est, _ = torch_sample(vertices, faces, n, gen)
        return evaluation.cloud_metrics(torch_voxels(reference, 0.02)[0], torch_voxels(est, 0.02)[0])

    res = {"reference_points": int(reference.shape[0]), "F": int(faces.shape[0]), "mesh_sample_point": n, "down_sample_res": 0.02}
    res.update(alternate(lambda: evaluation.evaluate_recon(reference, vertices, faces, mesh_sample_point=n), composed, reps, dev))
    res["native_result"] = evaluation.evaluate_recon(reference, vertices, faces, mesh_sample_point=n)
    m = composed()
    res["torch_result_cm"] = {"MAE_accuracy (cm)": m["accuracy_m"] * 100, "MAE_completeness (cm)": m["completeness_m"] * 100}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--voxel-sizes", type=int, nargs="+", default=[2_000_000, 10_000_000])
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--reference-points", type=int, default=2_000_000)
    ap.add_argument("--mesh-cell", type=float, default=0.0733)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16a_recon_eval.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("recon_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v, f = room_mesh(a.mesh_cell)
    vertices, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    res = {"what": "evaluation.voxel_down_sample / sample_mesh / evaluate_recon (sls_voxel_downsample, sls_mesh_sample) vs torch compositions",
           "data": "synthetic room, 16 keyframes, 1 cm noise; the room's faces as a triangle mesh, vertices jittered by 1 cm",
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region, "
                       "host reads included on both sides",
           "device": torch.cuda.get_device_name(0)}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    res["voxel_down_sample"] = []
    for M in a.voxel_sizes:
        res["voxel_down_sample"].append(bench_voxels(M, 0.02, a.reps, dev))
        write()
    res["sample_mesh"] = bench_sampling(vertices, faces, a.samples, a.reps, dev)
    write()
    reference = torch.from_numpy(room_cloud(a.reference_points, seed=1, noise=0.01)).to(dev)
    res["evaluate_recon"] = bench_whole(reference, vertices, faces, a.samples, a.reps, dev)
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
