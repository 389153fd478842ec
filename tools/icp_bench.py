#!/usr/bin/env python3
"""Times the cloud registration (splat_loam_amd.evaluation.register_icp -> sls_cloud_icp) against a torch composition on
the synthetic room clouds of tools/nn_bench.py, and checks first that both associate alike:

    python tools/icp_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--torch-chunks 8] [--out FILE.json]
    python tools/icp_bench.py --trace-run M          # one call per method for a kernel trace taken from outside
    python tools/icp_bench.py --parse-trace KERNEL_TRACE.csv [--out FILE.json]

  clouds       target: the room, M points; source: M other points of the room with 1 cm of noise, moved by 0.5 degrees and
               3 cm; the target's normals estimated once, outside the timed region; the gate 0.3 m; point-to-plane.
  native       the whole call at iterations = 0 (the index build and ONE pass) and at iterations = 10 with eps_rot =
               eps_trans = 0, so that all ten updates and the evaluation pass run: `per_pass_ms` = (t10 - t0) / 10.
  torch        ONE pass: the pose applied in float64, chunks of queries x all targets (float32 differences squared and
               summed by broadcasting) + argmin, the gate, the float64 rows J = [n, p' x n] and r, J^T J and J^T r by
               matrix products, torch.linalg.solve.  Its cost is M x M distances, so at most --torch-chunks chunks of
               queries are timed (0: all) and the file says how many: `torch_ms` is the time MEASURED for those queries
               alone, `torch_ms_all_queries_extrapolated` scales it by M / queries timed.
  split        from a rocprofv3 kernel trace taken in a run of its own (--trace-run under the profiler, then --parse-trace):
               device time of the index build (everything before the first transform kernel), of the search per pass
               (transform, sort, gather, query) and of the linearisation and solve per pass.
Native and torch run in one process and alternate; 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize inside
the timed region.  Agreement is asserted before anything is timed, on the queries torch covers: the same inlier set and the
same pairs for at least 99.9 % of them — torch's float32 distance is another expression than include/sls_nn_math.h's, so a
tie or a point at the gate may fall the other way — and the solved step within 1e-6 of the native first update when torch
covers every query."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

GATE = 0.3


def clouds(M, dev):
    from nn_bench import room_cloud
    from splat_loam_amd import evaluation
    target = torch.from_numpy(room_cloud(M, seed=1)).to(dev)
    moved = room_cloud(M, seed=2, noise=0.01).astype(np.float64)
    a = np.radians(0.5)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.02, -0.02, 0.01])
    source = torch.from_numpy(((moved - t) @ R).astype(np.float32)).to(dev)        # p = R^T (p' - t)
    normals = evaluation.estimate_normals(target, 0.5, 30, (12.0, 0.0, 1.0))
    return source, target, normals


def torch_pass(source, target, cols, normals, pose, rows, n_chunks):
    """One pass of the composition on the first rows * n_chunks queries: (index, inlier, H (6,6), b (6,), xi (6,))."""
    from nn_bench import torch_chunk
    n = min(len(source), rows * n_chunks)
    moved = (source[:n].double() @ pose[:3, :3].T + pose[:3, 3]).float()
    idx = torch.empty((n,), dtype=torch.int64, device=source.device)
    d2 = torch.empty((n,), dtype=torch.float32, device=source.device)
    for a in range(0, n, rows):
        v, i = torch_chunk(cols, moved[a:a + rows])
        d2[a:a + rows], idx[a:a + rows] = v, i
    inlier = d2 <= float(np.float32(GATE) * np.float32(GATE))
    p, q, nn = moved.double(), target[idx].double(), normals[idx].double()
    r = ((p - q) * nn).sum(1) * inlier
    J = torch.cat([nn, torch.linalg.cross(p, nn)], 1) * inlier.unsqueeze(1)
    H, b = J.T @ J, J.T @ r
    xi = torch.linalg.solve(H + 1e-9 * torch.eye(6, dtype=torch.float64, device=H.device), -b)
    return idx, inlier, H, b, xi


def bench_size(M, reps, torch_chunks, dev):
    from outlier_bench import alternate
    from splat_loam_amd import evaluation
    source, target, normals = clouds(M, dev)
    cols = tuple(target[:, c].contiguous() for c in range(3))
    rows = 4096
    free = torch.cuda.mem_get_info(dev)[0]
    while rows > 64 and 4 * rows * M * 4 > 0.5 * free:
        rows //= 2
    all_chunks = -(-M // rows)
    n_chunks = all_chunks if torch_chunks <= 0 else min(all_chunks, torch_chunks)
    n_timed = min(M, rows * n_chunks)
    eye = torch.eye(4, dtype=torch.float64, device=dev)
    kw = dict(max_distance=GATE, method="plane", eps_rot=0.0, eps_trans=0.0)
    # agreement first
    one = evaluation.register_icp(source, target, normals, iterations=0, return_details=True, **kw)
    idx_t, inl_t, H, b, xi = torch_pass(source, target, cols, normals, eye, rows, n_chunks)
    inl_n = one["dist2"][:n_timed] <= float(np.float32(GATE) * np.float32(GATE))
    same = (inl_n == inl_t) & ((one["index"][:n_timed].long() == idx_t) | ~inl_t)
    share = float(same.float().mean())
    assert share >= 0.999, (M, share)
    res = {"M": M, "torch_chunk_rows": rows, "torch_chunks_timed": n_chunks, "torch_chunks_all": all_chunks,
           "torch_queries_timed": n_timed, "queries_with_the_same_pair_and_gate_decision": share,
           "fitness_at_the_initial_pose": one["fitness"]}
    if n_timed == M:
        first = evaluation.register_icp(source, target, normals, iterations=1, **kw)["target_T_source"]
        step = float((first[:3, 3] - xi[:3].cpu()).abs().max())
        assert step <= 1e-6, step
        res["first_update_translation_vs_torch"] = step
    full = evaluation.register_icp(source, target, normals, iterations=30, max_distance=GATE)
    res["default_run"] = {k: full[k] for k in ("fitness", "inlier_rmse", "updates", "converged", "flags")}
    t0, t10, tor = alternate((lambda: evaluation.register_icp(source, target, normals, iterations=0, **kw),
                              lambda: evaluation.register_icp(source, target, normals, iterations=10, **kw),
                              lambda: torch_pass(source, target, cols, normals, eye, rows, n_chunks)), reps, dev)
    per_pass = (t10["median"] - t0["median"]) / 10.0
    extrapolated = tor["median"] * M / n_timed
    res.update({"native_one_pass_ms": t0, "native_ten_updates_ms": t10, "native_per_pass_ms": per_pass, "torch_one_pass_ms": tor,
                "torch_ms_all_queries_extrapolated": extrapolated,
                "native_one_pass_faster_than_torch_as_measured": bool(t0["median"] < tor["median"]),
                "native_one_pass_faster_than_torch_extrapolated": bool(t0["median"] < extrapolated),
                "native_per_pass_faster_than_torch_extrapolated": bool(per_pass < extrapolated)})
    print(f"M={M}: native one pass {t0['median']:.2f} ms, ten updates {t10['median']:.2f} ms ({per_pass:.2f} per pass), torch "
          f"{tor['median']:.2f} ms for {n_timed} queries ({extrapolated:.1f} extrapolated)", file=sys.stderr, flush=True)
    return res


def trace_run(M, dev):
    """What a kernel trace taken from outside should see: the clouds, one warm-up, then ONE call of five updates."""
    from splat_loam_amd import evaluation
    source, target, normals = clouds(M, dev)
    for _ in range(2):
        evaluation.register_icp(source, target, normals, iterations=5, max_distance=GATE, eps_rot=0.0, eps_trans=0.0)
        torch.cuda.synchronize(dev)


def parse_trace(path):
    """Device time per group of kernels of the LAST sls_cloud_icp call in a rocprofv3 kernel-trace CSV."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"]
    starts = [i for i, r in enumerate(rows) if "icp_init_kernel" in name(r)]
    call = rows[starts[-1]:]
    first_pass = next(i for i, r in enumerate(call) if "icp_transform_kernel" in name(r))
    us = lambda rs: sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs) / 1e3
    passes = sum("icp_solve_kernel" in name(r) for r in call)
    body = call[first_pass:]
    lin = [r for r in body if "icp_linearize_kernel" in name(r)]
    sol = [r for r in body if "icp_solve_kernel" in name(r)]
    qry = [r for r in body if "nn_query_kernel" in name(r)]
    tra = [r for r in body if "icp_transform_kernel" in name(r)]
    rest = [r for r in body if r not in lin and r not in sol and r not in qry and r not in tra]
    return {"passes": passes, "index_build_us": us(call[:first_pass]), "per_pass_us": {
        "transform_and_code": us(tra) / passes, "sort_and_gather": us(rest) / passes, "query": us(qry) / passes,
        "linearize": us(lin) / passes, "solve": us(sol) / passes}, "kernels_in_the_call": len(call)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-chunks", type=int, default=8)
    ap.add_argument("--trace-run", type=int, default=None, metavar="M")
    ap.add_argument("--parse-trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30a_icp.json"))
    a = ap.parse_args()
    if a.parse_trace:
        print(json.dumps(parse_trace(a.parse_trace)))
        return
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("icp_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    if a.trace_run is not None:
        trace_run(a.trace_run, dev)
        return
    res = {"what": "evaluation.register_icp (sls_cloud_icp, point-to-plane, all M source points against M target points) vs one "
                   "pass of chunked torch distances + argmin + float64 normal equations + torch.linalg.solve (torch_one_pass_ms "
                   "covers torch_queries_timed queries only)",
           "data": "synthetic room, 16 keyframes; the source moved by 0.5 degrees and 3 cm, 1 cm of noise; gate 0.3 m",
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region",
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
