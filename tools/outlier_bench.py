#!/usr/bin/env python3
"""Times the k-nearest-neighbour query and the statistical outlier filter (splat_loam_amd.evaluation.nearest_k ->
sls_nn_query_k, remove_statistical_outlier -> sls_outlier_statistical) against a torch composition on the synthetic room
clouds of tools/nn_bench.py, checks that both give the same result, and records what the filter does to mesh_tsdf:

    python tools/outlier_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--torch-chunks 8] [--out FILE.json]

  nearest_k   the cloud queried by itself at k = 8, 20 and 32, all M queries, distances + indices.  torch composition:
              chunks of queries x all targets, float32 differences squared and summed by broadcasting as in
              tools/nn_bench.py (not torch.cdist: its matrix-multiply form, |a|^2 + |b|^2 - 2 a.b, cancels at the small
              distances a neighbour search is about, and the neighbour sets would differ) + topk(k, smallest, sorted).  Its cost is M x M distances, minutes at 2 M, so at most --torch-chunks chunks are timed (0: all) and
              the file says how many: `torch_ms` is the time MEASURED for those queries alone,
              `torch_ms_all_queries_extrapolated` scales it by M / queries timed (every chunk does the same work).
  filter      remove_statistical_outlier(20, 2.0), the whole call with its host read, against: the same chunked
              distances + topk, sqrt, mean over k, then mean / std / mask / boolean gather with torch (float64 statistics).
              Where the k-NN part was timed on a slice, the composition's time is that part extrapolated + the rest
              measured, and is marked so.
  k = 1       evaluation.nearest (sls_nn_query, the packed best) beside nearest_k(k=1) (the list kernel at K = 4) for a
              second scan of the room as queries: what the list costs over the packed best.
  mesh_tsdf   on the synthetic graph of tools/sample_surface.py --probe: triangles, clusters and evaluate_recon (against
              the UNFILTERED sample_surface cloud) with and without outlier_nb=20.  Recorded, not judged.
Native and torch run in one process and alternate; 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize
inside the timed region.  Agreement is asserted before anything is timed: torch's distances to 1e-4 relative (its
float32 expression is another one than include/sls_nn_math.h's), the same neighbour sets for at least 99.9 % of the
queries compared, and the same kept rows for at least 99.9 % of the cloud."""
import argparse
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

from nn_bench import room_cloud
from splat_loam_amd import evaluation


def torch_dist2(target_cols, q):
    tx, ty, tz = target_cols
    acc = tx[None, :] - q[:, 0:1]
    acc.mul_(acc)
    d = ty[None, :] - q[:, 1:2]
    acc.addcmul_(d, d)
    torch.sub(tz[None, :], q[:, 2:3], out=d)
    acc.addcmul_(d, d)
    return acc


def torch_knn(target_cols, query, k, rows, n_chunks):
    """(dist2, index) of the first min(len(query), rows * n_chunks) queries: all distances + topk per chunk."""
    n = min(len(query), rows * n_chunks)
    d2 = torch.empty((n, k), dtype=torch.float32, device=query.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=query.device)
    for a in range(0, n, rows):
        v, i = torch.topk(torch_dist2(target_cols, query[a:a + rows]), k, dim=1, largest=False, sorted=True)
        d2[a:a + rows], idx[a:a + rows] = v, i
    return d2, idx


def torch_filter_tail(points, dist2, std_ratio):
    """mean / std / mask / boolean gather of the restated rule from (M, k) squared distances."""
    mean = dist2.sqrt().double().sum(1) / dist2.shape[1]
    counted = mean > 0
    n = mean.shape[0]
    cloud_mean = mean[counted].sum() / n
    std = ((mean[counted] - cloud_mean) ** 2).sum().div(n - 1).sqrt()
    keep = counted & (mean < cloud_mean + std_ratio * std)
    return points[keep], keep


def stat(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def alternate(fns, reps, dev, warm=3):
    times = [[] for _ in fns]
    for it in range(warm + reps):
        for fn, acc in zip(fns, times):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize(dev)
            if it >= warm:
                acc.append((time.perf_counter() - t0) * 1e3)
            del res
    return [stat(t) for t in times]


def bench_size(M, reps, torch_chunks, dev):
    cloud = torch.from_numpy(room_cloud(M, seed=1)).to(dev)
    second = torch.from_numpy(room_cloud(M, seed=2, noise=0.01)).to(dev)
    cols = tuple(cloud[:, c].contiguous() for c in range(3))
    rows = 4096
    free = torch.cuda.mem_get_info(dev)[0]
    while rows > 64 and 4 * rows * M * 4 > 0.5 * free:       # the distance matrix, topk's temporaries, slack
        rows //= 2
    all_chunks = -(-M // rows)
    n_chunks = all_chunks if torch_chunks <= 0 else min(all_chunks, torch_chunks)
    n_timed = min(M, rows * n_chunks)
    res = {"M": M, "torch_chunk_rows": rows, "torch_chunks_timed": n_chunks, "torch_chunks_all": all_chunks,
           "torch_queries_timed": n_timed, "nearest_k": {}}
    for k in (8, 20, 32):
        d2n, idxn = evaluation.nearest_k(cloud, cloud, k)
        d2t, idxt = torch_knn(cols, cloud, k, rows, n_chunks)
        rel = float(((d2n[:n_timed] - d2t).abs() / d2t.clamp_min(1e-12)).max())
        same = float((idxn[:n_timed].long().sort(1).values == idxt.sort(1).values).all(1).float().mean())
        assert rel <= 1e-4 and same >= 0.999, (M, k, rel, same)
        del d2n, idxn, d2t, idxt
        nat, tor = alternate((lambda: evaluation.nearest_k(cloud, cloud, k), lambda: torch_knn(cols, cloud, k, rows, n_chunks)), reps, dev)
        res["nearest_k"][str(k)] = {"native_ms": nat, "torch_ms": tor, "torch_ms_all_queries_extrapolated": tor["median"] * M / n_timed,
                                    "native_faster_than_torch_as_measured": bool(nat["median"] < tor["median"]),
                                    "dist2_max_relative_difference": rel, "queries_with_the_same_neighbour_set": same}
        print(f"M={M} k={k}: native {nat['median']:.2f} ms, torch {tor['median']:.2f} ms for {n_timed} queries", file=sys.stderr, flush=True)
    # the whole filter: the composition's k-NN part over all queries only where that was asked for (or is all there is)
    k, ratio = 20, 2.0
    out_n, index_n, det = evaluation.remove_statistical_outlier(cloud, k, ratio, return_index=True, details=True)
    d2_all = evaluation.nearest_k(cloud, cloud, k, return_index=False)[0] if n_timed < M else torch_knn(cols, cloud, k, rows, n_chunks)[0]
    out_t, keep_t = torch_filter_tail(cloud, d2_all, ratio)
    keep_n = torch.zeros((M,), dtype=torch.bool, device=dev)
    keep_n[index_n.long()] = True
    agree = float((keep_n == keep_t).float().mean())
    assert agree >= 0.999, (M, agree)
    nat, knn_part, tail = alternate((lambda: evaluation.remove_statistical_outlier(cloud, k, ratio),
                                     lambda: torch_knn(cols, cloud, k, rows, n_chunks),
                                     lambda: torch_filter_tail(cloud, d2_all, ratio)), reps, dev)
    composed = knn_part["median"] * M / n_timed + tail["median"]
    res["remove_statistical_outlier_20_2.0"] = {
        "native_ms": nat, "torch_knn_part_ms": knn_part, "torch_tail_ms": tail, "torch_composition_ms": composed,
        "torch_composition_is_extrapolated": bool(n_timed < M), "native_faster_than_torch_composition": bool(nat["median"] < composed),
        "kept": det["kept"], "removed": det["removed"], "threshold_m": det["threshold"], "kept_rows_that_agree": agree,
        "torch_tail_input": "the native distances" if n_timed < M else "torch's own distances"}
    del d2_all, out_t, keep_t, out_n
    print(f"M={M} filter: native {nat['median']:.2f} ms, torch composition {composed:.2f} ms", file=sys.stderr, flush=True)
    # k = 1: the packed best against the list kernel
    a2, ai = evaluation.nearest(cloud, second)
    b2, bi = evaluation.nearest_k(cloud, second, 1)
    assert torch.equal(a2.view(torch.int32), b2[:, 0].view(torch.int32)) and torch.equal(ai, bi[:, 0])
    one, lst = alternate((lambda: evaluation.nearest(cloud, second), lambda: evaluation.nearest_k(cloud, second, 1)), reps, dev)
    res["k1_second_scan"] = {"nearest_ms": one, "nearest_k_1_ms": lst, "equal_bit_for_bit": True}
    return res


def does_it_help(dev, voxel=0.25):
    from sample_surface import write_synthetic_results
    from splat_loam_amd import mesh_ops, meshing
    out = {"data": "the synthetic graph of tools/sample_surface.py --probe: 8 keyframes, 64 x 1024, 50 000 surfels", "voxel_size": voxel,
           "reference_of_evaluate_recon": "the unfiltered sample_surface cloud"}
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        write_synthetic_results(d)
        reference, _ = meshing.sample_surface(d, seed=1, device=dev)
        for name, nb in (("without", None), ("outlier_nb_20", 20)):
            v, f, det = meshing.mesh_tsdf(d, voxel, seed=1, device=dev, details=True, outlier_nb=nb)
            clean = mesh_ops.clean_mesh(v, f, details=True)[-1]
            rec = evaluation.evaluate_recon(reference, v, f, mesh_sample_point=1_000_000, seed=1)
            out[name] = {"samples": det["samples"], "blocks": det["blocks"], "triangles": det["triangles"], "clusters": clean["clusters"],
                         "evaluate_recon": {k: (float(x) if isinstance(x, (int, float)) else x) for k, x in rec.items()}}
            if "outlier" in det:
                out[name]["outlier"] = {k: x for k, x in det["outlier"].items() if k != "index"}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-chunks", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23a_outlier.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("outlier_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"what": "evaluation.nearest_k (sls_nn_query_k, the cloud by itself, all M queries, distances + indices) and "
                   "remove_statistical_outlier(20, 2.0) (sls_outlier_statistical + its host read) vs chunked torch distances + topk and "
                   "torch statistics (torch_ms covers torch_queries_timed queries only)",
           "data": "synthetic room, 16 keyframes; k = 1: queries = a second scan with 1 cm noise",
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region",
           "device": torch.cuda.get_device_name(0), "mesh_tsdf": does_it_help(dev), "sizes": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for M in a.sizes:                                  # (the file is complete after every size)
        res["sizes"].append(bench_size(M, a.reps, a.torch_chunks, dev))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
