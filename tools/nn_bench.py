#!/usr/bin/env python3
"""Times the two-cloud nearest-neighbour search (splat_loam_amd.evaluation.nearest -> sls_nn_query) against a chunked
torch brute force on synthetic room clouds, and checks that both return the same squared distances:

    python tools/nn_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--torch-chunks 32] [--out FILE.json]

Clouds: a 40 x 24 x 6 m room scanned from `synth.keyframe_poses` with the spherical sensor of `synth` (its vertical
field of view widened so that floor and ceiling are hit), one block of rows per keyframe in the world frame — the layout
of `meshing.sample_surface`'s output.  The query cloud is a second scan of the same room with 1 cm of noise.

torch composition: 4 096 queries x all targets per chunk (float32 differences, squares summed in the order of
include/sls_nn_math.h), min / argmin per chunk.  The brute force costs Mt x Mq distance evaluations, minutes at 2 M, so
at most --torch-chunks chunks are timed (0: all) and the file says how many: `torch_ms` is the time MEASURED for those
queries alone, `torch_ms_all_queries_extrapolated` scales it by Mq / queries timed (every chunk does the same work).
The native call always serves ALL Mq queries.  Both run in one process and alternate; 3 warm-ups, the median of --reps
(>= 10), torch.cuda.synchronize inside the timed region.  With scipy present, one `cKDTree` build + 16-worker query is
recorded as information."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from splat_loam_amd import evaluation, synth

ROOM_MIN = np.array([-8.0, -12.0, -2.0])
ROOM_MAX = np.array([32.0, 12.0, 4.0])


def room_cloud(n, seed, noise=0.0, n_frames=16):
    """n points on the walls, floor and ceiling of the room, in blocks of one keyframe each."""
    rng = np.random.default_rng(seed)
    poses = synth.keyframe_poses(n_frames)
    per = -(-n // n_frames)
    out = []
    for T in poses:
        az = rng.uniform(-math.pi, math.pi, per)
        el = rng.uniform(math.radians(-40.0), math.radians(40.0), per)
        ray = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], 1) @ T[:3, :3].T
        o = T[:3, 3]
        with np.errstate(divide="ignore"):
            t = np.where(ray > 0, (ROOM_MAX - o) / ray, (ROOM_MIN - o) / ray)       # exit distance per axis
        out.append(o + ray * t.min(1, keepdims=True))
    pts = np.concatenate(out)[:n]
    if noise:
        pts = pts + rng.normal(0, noise, pts.shape)
    return pts.astype(np.float32)


def torch_chunk(target_cols, q):
    tx, ty, tz = target_cols
    acc = tx[None, :] - q[:, 0:1]
    acc.mul_(acc)
    d = ty[None, :] - q[:, 1:2]
    acc.addcmul_(d, d)
    torch.sub(tz[None, :], q[:, 2:3], out=d)
    acc.addcmul_(d, d)
    return acc.min(dim=1)


def torch_brute_force(target_cols, query, rows, n_chunks):
    d2 = torch.empty((min(len(query), rows * n_chunks),), dtype=torch.float32, device=query.device)
    idx = torch.empty_like(d2, dtype=torch.int64)
    for c in range(n_chunks):
        a = c * rows
        if a >= len(query):
            break
        v, i = torch_chunk(target_cols, query[a:a + rows])
        d2[a:a + rows], idx[a:a + rows] = v, i
    return d2, idx


def bench_size(M, reps, torch_chunks, dev):
    target = torch.from_numpy(room_cloud(M, seed=1)).to(dev)
    query = torch.from_numpy(room_cloud(M, seed=2, noise=0.01)).to(dev)
    cols = tuple(target[:, k].contiguous() for k in range(3))
    rows = 4096
    free = torch.cuda.mem_get_info(dev)[0]
    while rows > 64 and 3 * rows * M * 4 > 0.5 * free:      # two (rows x M) float32 temporaries + slack
        rows //= 2
    all_chunks = -(-M // rows)
    n_chunks = all_chunks if torch_chunks <= 0 else min(all_chunks, torch_chunks)
    n_timed = min(M, rows * n_chunks)

    def native():
        return evaluation.nearest(target, query)

    def composed():
        return torch_brute_force(cols, query, rows, n_chunks)

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
    d2n, idxn = native()
    d2t, idxt = composed()
    rel = ((d2n[:n_timed] - d2t).abs() / d2t.clamp_min(1e-30)).max().item()
    same_index = float((idxn[:n_timed].long() == idxt).float().mean().item())
    res = {"Mt": M, "Mq": M, "native_ms": {"median": float(np.median(t_nat)), "min": float(np.min(t_nat)), "max": float(np.max(t_nat))},
           "torch_ms": {"median": float(np.median(t_tor)), "min": float(np.min(t_tor)), "max": float(np.max(t_tor))},
           "torch_chunk_rows": rows, "torch_chunks_timed": n_chunks, "torch_chunks_all": all_chunks, "torch_queries_timed": n_timed,
           "torch_ms_all_queries_extrapolated": float(np.median(t_tor)) * M / n_timed,
           "native_faster_than_torch_as_measured": bool(np.median(t_nat) < np.median(t_tor)),
           "dist2_max_relative_difference": rel, "dist2_agree_to_2^-21": bool(rel <= 2.0 ** -21),
           "index_agreement": same_index}
    try:
        from scipy.spatial import cKDTree
        tn, qn = target.cpu().numpy().astype(np.float64), query.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(tn)
        t1 = time.perf_counter()
        tree.query(qn, k=1, workers=16)
        res["ckdtree_16_workers_ms"] = {"build": (t1 - t0) * 1e3, "query": (time.perf_counter() - t1) * 1e3, "runs": 1}
    except ImportError:
        res["ckdtree_16_workers_ms"] = "not measured: scipy is not installed"
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-chunks", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15a_nn_search.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("nn_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"what": "evaluation.nearest (sls_nn_query, all Mq queries, distances + indices) vs a chunked torch brute force "
                   "(torch_ms covers torch_queries_timed queries only)",
           "data": "synthetic room, 16 keyframes, query = a second scan with 1 cm noise",
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region",
           "device": torch.cuda.get_device_name(0), "sizes": [bench_size(M, a.reps, a.torch_chunks, dev) for M in a.sizes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
