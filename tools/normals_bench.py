#!/usr/bin/env python3
"""Times the PCA normal estimate (splat_loam_amd.evaluation.estimate_normals -> sls_cloud_normals) against a torch
composition on the synthetic room clouds of tools/outlier_bench.py, and checks that both give the same result:

    python tools/normals_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--torch-chunks 8] [--out FILE.json]

  rows         max_nn = 30 and 50, each with radius = 0.5 and with None (the max_nn nearest at any distance), the viewpoint
               at the origin.
  torch        chunks of queries x all targets, float32 differences squared and summed by broadcasting as in
               tools/outlier_bench.py + topk(max_nn, smallest, sorted), the radius as a mask on topk's distances, a float64
               mean and covariance over the masked neighbours, torch.linalg.eigh, the first eigenvector flipped towards
               the viewpoint, unit(viewpoint - p) below three neighbours.  Its cost is M x M distances, so at most
               --torch-chunks chunks are timed (0: all) and the file says how many: `torch_ms` is the time MEASURED for
               those queries alone, `torch_ms_all_queries_extrapolated` scales it by M / queries timed.
  split        the search and the rest — the new kernel — of one native call, in device time (events around the call, an extra
               pass that is not the timed one): the search is the same call at radius 1e-6, where every neighbourhood is
               the point alone, the kernel reads one entry of a row and writes the fallback; the rest is the difference.
  beyond 32    the search at max_nn = 32 (one pass of the 32-long register list) and at max_nn = 33 and 64 (two passes: the 32
               nearest, then the rest beyond the 32nd key, which only this call reaches): what the second pass costs.
Native and torch run in one process and alternate; 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize inside
the timed region.  Agreement is asserted before anything is timed, on the queries torch covers: the same neighbour sets
(and counts) for at least 99.9 % of them — torch's float32 distance is another expression than include/sls_nn_math.h's, so
a tie or a point at the radius may fall the other way — and, where the sets agree and (l1 - l0) >= 1e-3 * l2,
|n x n_eigh| <= 1e-6: the float32 rounding of the output with a margin of ten (tests/test_normals_math.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from nn_bench import room_cloud
from outlier_bench import alternate, torch_knn
from splat_loam_amd import evaluation


def torch_normals(cloud, cols, k, radius, rows, n_chunks):
    """(normals float64 (n,3), count (n,), sorted neighbour rows (n,k) with -1 outside the radius, eigenvalues (n,3))."""
    d2, idx = torch_knn(cols, cloud, k, rows, n_chunks)
    n = d2.shape[0]
    inside = torch.ones_like(d2, dtype=torch.bool) if radius is None else d2 <= float(np.float32(radius) * np.float32(radius))
    count = inside.sum(1)
    w = inside.double().unsqueeze(-1)
    P = cloud.double()[idx]                                             # (n, k, 3)
    mean = (P * w).sum(1) / count.clamp_min(1).double().unsqueeze(-1)
    D = (P - mean.unsqueeze(1)) * w
    cov = torch.einsum("nki,nkj->nij", D, D) / count.clamp_min(1).double().view(-1, 1, 1)
    lam, vec = torch.linalg.eigh(cov)
    nrm = vec[:, :, 0]
    view = -cloud[:n].double()                                          # viewpoint at the origin
    nrm = torch.where(((nrm * view).sum(1) < 0).unsqueeze(-1), -nrm, nrm)
    unit = view / view.norm(dim=1, keepdim=True).clamp_min(1e-300)
    nrm = torch.where((count < 3).unsqueeze(-1), unit, nrm)
    return nrm, count, torch.where(inside, idx, torch.full_like(idx, -1)).sort(1).values, lam


def agreement(cloud, cols, k, radius, rows, n_chunks):
    nrm_t, count_t, set_t, lam = torch_normals(cloud, cols, k, radius, rows, n_chunks)
    n = nrm_t.shape[0]
    nrm_n, count_n, _, _, idx_n = evaluation._estimate_normals(cloud, radius, k, (0.0, 0.0, 0.0), True, True)
    keep = torch.arange(k, device=cloud.device)[None, :] < count_n[:n].long()[:, None]
    set_n = torch.where(keep, idx_n[:n].long(), torch.full_like(idx_n[:n].long(), -1)).sort(1).values
    same = (set_n == set_t).all(1) & (count_n[:n].long() == count_t)
    clear = same & (count_t >= 3) & ((lam[:, 1] - lam[:, 0]) >= 1e-3 * lam[:, 2])
    cross = torch.linalg.cross(nrm_n[:n].double(), nrm_t).norm(dim=1)
    worst = float(cross[clear].max()) if bool(clear.any()) else 0.0
    few = same & (count_t < 3)
    worst_few = float((nrm_n[:n].double() - nrm_t)[few].abs().max()) if bool(few.any()) else 0.0
    share, compared = float(same.float().mean()), float(clear.float().mean())
    assert share >= 0.999 and worst <= 1e-6 and worst_few <= 1e-6, (k, radius, share, worst, worst_few)
    return {"queries_with_the_same_neighbour_set": share, "queries_compared_with_eigh": compared,
            "max_cross_product_with_eigh": worst, "fallback_queries": float(few.float().mean()),
            "mean_neighbours": float(count_n.double().mean())}


def device_ms(fn, reps, dev):
    times = []
    for it in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize(dev)
        if it >= 3:
            times.append(a.elapsed_time(b))
        del res
    return float(np.median(times))


def split(cloud, k, radius, reps, dev):
    """(whole call, search) in device ms per call, from events around the call.  The search: the same call at a radius that
    leaves every point alone — the lists are found as before, the kernel then reads one entry of a row and writes the fallback."""
    whole = device_ms(lambda: evaluation.estimate_normals(cloud, radius, k), reps, dev)
    search = device_ms(lambda: evaluation.estimate_normals(cloud, 1e-6, k), reps, dev)
    return whole, search


def bench_size(M, reps, torch_chunks, dev):
    cloud = torch.from_numpy(room_cloud(M, seed=1)).to(dev)
    cols = tuple(cloud[:, c].contiguous() for c in range(3))
    rows = 2048
    free = torch.cuda.mem_get_info(dev)[0]
    while rows > 64 and 4 * rows * M * 4 > 0.5 * free:       # the distance matrix, topk's temporaries, slack
        rows //= 2
    all_chunks = -(-M // rows)
    n_chunks = all_chunks if torch_chunks <= 0 else min(all_chunks, torch_chunks)
    n_timed = min(M, rows * n_chunks)
    res = {"M": M, "torch_chunk_rows": rows, "torch_chunks_timed": n_chunks, "torch_chunks_all": all_chunks,
           "torch_queries_timed": n_timed, "rows": []}
    for k in (30, 50):
        for radius in (0.5, None):
            row = {"max_nn": k, "radius": radius}
            row.update(agreement(cloud, cols, k, radius, rows, n_chunks))
            nat, tor = alternate((lambda: evaluation.estimate_normals(cloud, radius, k),
                                  lambda: torch_normals(cloud, cols, k, radius, rows, n_chunks)), reps, dev)
            whole, search = split(cloud, k, radius, reps, dev)
            extrapolated = tor["median"] * M / n_timed
            row.update({"native_ms": nat, "torch_ms": tor, "torch_ms_all_queries_extrapolated": extrapolated,
                        "native_faster_than_torch_as_measured": bool(nat["median"] < tor["median"]),
                        "native_faster_than_torch_extrapolated": bool(nat["median"] < extrapolated),
                        "native_device_ms": whole, "search_device_ms": search, "normals_kernel_device_ms": whole - search})
            res["rows"].append(row)
            print(f"M={M} max_nn={k} radius={radius}: native {nat['median']:.2f} ms (search {search:.2f}, rest {whole - search:.2f}), "
                  f"torch {tor['median']:.2f} ms for {n_timed} queries", file=sys.stderr, flush=True)
    w32, s32 = split(cloud, 32, None, reps, dev)
    w33, s33 = split(cloud, 33, None, reps, dev)
    w64, s64 = split(cloud, 64, None, reps, dev)
    res["beyond_32"] = {"max_nn_32_one_pass": {"native_device_ms": w32, "search_device_ms": s32},
                        "max_nn_33_two_passes": {"native_device_ms": w33, "search_device_ms": s33},
                        "max_nn_64_two_passes": {"native_device_ms": w64, "search_device_ms": s64},
                        "search_ratio_33_to_32": s33 / s32, "search_ratio_64_to_32": s64 / s32}
    print(f"M={M}: search at max_nn 32 {s32:.2f} ms, at 33 {s33:.2f} ms, at 64 {s64:.2f} ms", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-chunks", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24a_normals.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("normals_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"what": "evaluation.estimate_normals (sls_cloud_normals: the self-query + the PCA kernel, all M points) vs chunked torch "
                   "distances + topk + float64 covariance + torch.linalg.eigh (torch_ms covers torch_queries_timed queries only)",
           "data": "synthetic room, 16 keyframes, viewpoint at the origin",
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region; "
                       "the split: device events around the call, the search = the same call at radius 1e-6, an extra pass",
           "device": torch.cuda.get_device_name(0), "sizes": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for M in a.sizes:                                  # (the file is complete after every size)
        res["sizes"].append(bench_size(M, a.reps, a.torch_chunks, dev))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
