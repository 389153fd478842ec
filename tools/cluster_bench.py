#!/usr/bin/env python3
"""Times the cloud clustering (splat_loam_amd.evaluation.cluster_dbscan -> sls_cloud_dbscan, keep_clusters -> + sls_cloud_select)
on the synthetic room clouds of tools/nn_bench.py, and records what the cluster stage does to the meshing chain:

    python tools/cluster_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--no-profile] [--out FILE.json]

  eps          about three point spacings of each cloud: 3 * sqrt(room surface / M); min_points = 10.
  dbscan       the whole cluster_dbscan and the whole keep_clusters, each with its one host read.
  radius       remove_radius_outlier(nb_points = min_points - 1, radius = eps) on the same cloud: it answers the same core
               question through a 16-long neighbour list (its code is the same before and after this bench was added).  The
               count search does less work per target, so cluster_dbscan's count kernel is expected not to be slower than that
               filter's query kernel; both whole calls and, by kernel, both kernels are recorded, slower rows included.
  torch        chunked float32 distances <= eps * eps, summed per query, for the first 32 768 queries (the core flags alone:
               no components, no borders), scaled to all M queries — every chunk does the same work.
  by kernel    a child of its own under `rocprofv3 --kernel-trace --stats` at every size: two cluster_dbscan and two
               remove_radius_outlier calls, the averages per kernel.
  chain        on the synthetic graph of tools/sample_surface.py --probe with the statistical filter on: samples kept,
               blocks allocated, mesh clusters before keep_clusters, and evaluate_recon (against the UNFILTERED cloud), without
               and with cluster_eps at three radii, and the whole sample_surface at each (alternating, medians, as above).
               Recorded, not judged.
Equal outputs are asserted before anything is timed: the cores of cluster_dbscan are exactly the rows the radius filter keeps,
keep_clusters is cluster_dbscan followed by the rule, a second run gives the same bytes, and torch's core flags agree for at
least 99.9 % of the queries compared (its float32 expression is another one).  One process, alternating, 3 warm-ups, the
median of --reps (>= 10), torch.cuda.synchronize inside the timed region."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from nn_bench import ROOM_MAX, ROOM_MIN, room_cloud
from outlier_bench import alternate, torch_dist2
from splat_loam_amd import evaluation

MIN_POINTS = 10
TORCH_QUERIES = 32768


def eps_for(M):
    d = np.asarray(ROOM_MAX, np.float64) - np.asarray(ROOM_MIN, np.float64)
    area = 2.0 * (d[0] * d[1] + d[1] * d[2] + d[0] * d[2])
    return float(np.float32(3.0 * np.sqrt(area / M)))


def torch_core(cols, query, r2, rows):
    out = torch.empty((len(query),), dtype=torch.bool, device=query.device)
    for a in range(0, len(query), rows):
        out[a:a + rows] = (torch_dist2(cols, query[a:a + rows]) <= r2).sum(1) >= MIN_POINTS
    return out


def bench_size(M, reps, dev):
    cloud = torch.from_numpy(room_cloud(M, seed=1)).to(dev)
    eps = eps_for(M)
    cols = tuple(cloud[:, c].contiguous() for c in range(3))
    rows = 4096
    free = torch.cuda.mem_get_info(dev)[0]
    while rows > 64 and 4 * rows * M * 4 > 0.5 * free:
        rows //= 2
    n_timed = min(M, TORCH_QUERIES)
    # equal outputs first
    labels, counts, det = evaluation.cluster_dbscan(cloud, eps, MIN_POINTS, return_counts=True, details=True)
    labels2, counts2 = evaluation.cluster_dbscan(cloud, eps, MIN_POINTS, return_counts=True)
    assert torch.equal(labels, labels2) and torch.equal(counts, counts2), "two runs differ"
    kept_radius = evaluation.remove_radius_outlier(cloud, MIN_POINTS - 1, eps, return_index=True)[1]
    assert int(kept_radius.shape[0]) == det["core"], (kept_radius.shape, det)
    assert bool((labels[kept_radius.long()] >= 0).all())
    kept, index, kdet = evaluation.keep_clusters(cloud, eps, MIN_POINTS, return_index=True, details=True)
    n_min = int(counts.max()) if counts.numel() else 0
    want = torch.nonzero((labels >= 0) & (counts[labels.clamp_min(0).long()] >= n_min)).flatten() if counts.numel() else index[:0].long()
    assert torch.equal(index.long(), want) and kdet["n_min"] == n_min and torch.equal(kept, cloud[want])
    core_native = torch.zeros((M,), dtype=torch.bool, device=dev)
    core_native[kept_radius.long()] = True
    core_torch = torch_core(cols, cloud[:n_timed], eps * eps, rows)
    agree = float((core_torch == core_native[:n_timed]).float().mean())
    assert agree >= 0.999, (M, agree)
    del labels2, counts2, kept, index, want, core_torch
    db, kc, rad, tor = alternate((lambda: evaluation.cluster_dbscan(cloud, eps, MIN_POINTS),
                                  lambda: evaluation.keep_clusters(cloud, eps, MIN_POINTS),
                                  lambda: evaluation.remove_radius_outlier(cloud, MIN_POINTS - 1, eps),
                                  lambda: torch_core(cols, cloud[:n_timed], eps * eps, rows)), reps, dev)
    row = {"M": M, "eps": eps, "min_points": MIN_POINTS, "clusters": det, "kept_by_keep_clusters": kdet["kept"],
           "largest_counts": counts.sort(descending=True).values[:5].tolist(),
           "cluster_dbscan_ms": db, "keep_clusters_ms": kc, "remove_radius_outlier_ms": rad,
           "cluster_dbscan_slower_than_radius_filter": bool(db["median"] > rad["median"]),
           "torch_core_flags_ms": tor, "torch_queries_timed": n_timed, "torch_core_flags_ms_all_queries_extrapolated": tor["median"] * M / n_timed,
           "torch_core_flags_that_agree": agree}
    print(f"M={M} eps={eps:.4f}: dbscan {db['median']:.2f} ms, keep_clusters {kc['median']:.2f} ms, radius filter {rad['median']:.2f} ms, "
          f"torch core flags {tor['median']:.2f} ms for {n_timed} queries; {det}", file=sys.stderr, flush=True)
    return row


def by_kernel(M):
    """A child under rocprofv3 --kernel-trace --stats: the kernels of two cluster_dbscan and two remove_radius_outlier calls."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "-d", d, "-o", "cluster", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", str(M)]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not files:
            return {"skipped": f"rocprofv3 run gave code {run.returncode} and {len(files)} stats files", "stderr": run.stderr[-400:]}
        rows = []
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if any(s in name for s in ("cluster_", "knn_", "nn_query_k", "outlier_", "sort_", "radix")):
                    rows.append({"kernel": name.split("(")[0][-70:], "calls": int(r.get("Calls", 0)),
                                 "total_us": float(r.get("TotalDurationNs", 0)) / 1e3, "average_us": float(r.get("AverageNs", 0)) / 1e3})
        return {"calls_traced": "2 x cluster_dbscan, 2 x remove_radius_outlier (the index build's kernels serve both)", "kernels": rows}


def profile_child(M):
    dev = torch.device("cuda:0")
    cloud = torch.from_numpy(room_cloud(M, seed=1)).to(dev)
    for _ in range(2):
        evaluation.cluster_dbscan(cloud, eps_for(M), MIN_POINTS)
        evaluation.remove_radius_outlier(cloud, MIN_POINTS - 1, eps_for(M))
    torch.cuda.synchronize(dev)


def chain(dev, reps, voxel=0.25):
    from sample_surface import write_synthetic_results
    from splat_loam_amd import mesh_ops, meshing
    out = {"data": "the synthetic graph of tools/sample_surface.py --probe: 8 keyframes, 64 x 1024, 50 000 surfels", "voxel_size": voxel,
           "outlier_nb": 20, "reference_of_evaluate_recon": "the unfiltered sample_surface cloud", "rows": []}
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        write_synthetic_results(d)
        reference, _ = meshing.sample_surface(d, seed=1, device=dev)
        radii = (None, 0.5, 1.0, 2.0)
        # the whole sample_surface behind outlier_nb=20 at every radius, timed as everything else here (the cloud's spacing is
        # a few cm near the sensor: these radii are MANY spacings there, the quadratic case)
        laps = alternate([(lambda e=e: meshing.sample_surface(d, seed=1, device=dev, outlier_nb=20, cluster_eps=e)) for e in radii], reps, dev)
        for eps, lap in zip(radii, laps):
            v, f, det = meshing.mesh_tsdf(d, voxel, seed=1, device=dev, details=True, outlier_nb=20, cluster_eps=eps)
            clean = mesh_ops.clean_mesh(v, f, details=True)[-1]
            v1, f1 = meshing.mesh_tsdf(d, voxel, seed=1, device=dev, outlier_nb=20, cluster_eps=eps, keep_clusters=1)[:2]
            rec = evaluation.evaluate_recon(reference, v1, f1, mesh_sample_point=1_000_000, seed=1)
            row = {"cluster_eps": eps, "samples": det["samples"], "blocks": det["blocks"], "triangles": det["triangles"],
                   "mesh_clusters_before_keep_clusters": clean["clusters"], "sample_surface_ms": lap, "stage_ms_one_lap": det["stage_ms"],
                   "evaluate_recon_after_keep_clusters_1": {k: (float(x) if isinstance(x, (int, float)) else x) for k, x in rec.items()}}
            if "cluster" in det:
                row["cluster"] = {k: x for k, x in det["cluster"].items() if k != "index"}
            out["rows"].append(row)
            print(json.dumps({k: x for k, x in row.items() if k != "evaluate_recon_after_keep_clusters_1"}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-profile", action="store_true", help="leave out the rocprofv3 children")
    ap.add_argument("--no-chain", action="store_true", help="leave out the meshing chain")
    ap.add_argument("--profile-child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33a_cluster.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_bench needs a GPU: a time taken elsewhere says nothing")
    if a.profile_child is not None:
        return profile_child(a.profile_child)
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    dev = torch.device("cuda:0")
    res = {"what": "evaluation.cluster_dbscan (sls_cloud_dbscan) and keep_clusters (+ sls_cloud_select), each with its host read, beside "
                   "remove_radius_outlier(min_points - 1, eps) and chunked torch distances <= eps (core flags alone, "
                   "torch_queries_timed queries)",
           "data": "synthetic room, 16 keyframes", "eps": "3 * sqrt(room surface / M)",
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region",
           "device": torch.cuda.get_device_name(0), "sizes": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def save():                                            # (the file is complete after every step)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for M in a.sizes:
        row = bench_size(M, a.reps, dev)
        row["by_kernel"] = {"skipped": "--no-profile"} if a.no_profile else by_kernel(M)
        res["sizes"].append(row)
        save()
    if not a.no_chain:
        res["chain"] = chain(dev, a.reps)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
