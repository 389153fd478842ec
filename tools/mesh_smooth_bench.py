#!/usr/bin/env python3
"""Times mesh smoothing over the edge graph (splat_loam_amd.mesh_ops.vertex_adjacency / smooth -> sls_mesh_adjacency,
sls_mesh_smooth) against what a user without it would write, and checks that both give the same mesh:

    python tools/mesh_smooth_bench.py [--radius 10] [--voxel 0.1] [--floaters 24] [--reps 10] [--out FILE.json]

Data: the synthetic TSDF volume of tools/mesh_clean_bench.py (a sphere of --radius metres, about 1.15 M triangles at the
defaults), extracted and cleaned with mesh_ops.clean_mesh.

  composition  the rules of include/sls_smooth_math.h in torch with EQUAL neighbour sets: torch.unique over the directed
               pairs a * V + b (the adjacency build), and per sweep index_add_ of the float64 weights and the weighted
               float64 positions (three atomic scatters), the float32 distance as the header takes it
  adjacency    mesh_ops.vertex_adjacency against the torch.unique build (offsets by searchsorted): neighbours equal
  sweep        (a whole call of n iterations - a whole call of 0 iterations) / sweeps, both sides: the 0-iteration call
               is the adjacency build and the copy
  call         whole calls of 10 Taubin iterations (20 sweeps), the adjacency build included on both sides
  check        positions agree within the tolerance this run records: the two sides differ in the order of the float64
               sums alone, a relative 2^-53 per addition, which the rounding to float32 shows as one ulp now and then
  stages       the native call's launches by group through sls_timing_enable(1), in a run of their own
Both sides of a comparison run in one process and alternate; 3 warm-ups, the median of --reps (>= 10),
torch.cuda.synchronize inside the timed region."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from mesh_clean_bench import alternate, synthetic_volume
from splat_loam_amd import _abi, mesh_ops


def composed_adjacency(f, V):
    """(rows (2E,) int64, neighbours (2E,) int64, offsets (V+1,) int64) with torch.unique on the directed pairs"""
    fl = f.long()
    ok = ((fl >= 0) & (fl < V)).all(1) & (fl[:, 0] != fl[:, 1]) & (fl[:, 1] != fl[:, 2]) & (fl[:, 2] != fl[:, 0])
    fo = fl[ok]
    a = torch.cat([fo[:, 0], fo[:, 1], fo[:, 1], fo[:, 2], fo[:, 2], fo[:, 0]])
    b = torch.cat([fo[:, 1], fo[:, 0], fo[:, 2], fo[:, 1], fo[:, 0], fo[:, 2]])
    key = torch.unique(a * V + b)
    rows, nbr = key // V, key % V
    offsets = torch.searchsorted(rows, torch.arange(V + 1, device=f.device))
    return rows, nbr, offsets


def composed_smooth(v, f, iterations, method, weights, lam, mu, graph=None):
    rows, nbr, _ = graph if graph is not None else composed_adjacency(f, int(v.shape[0]))
    V = int(v.shape[0])
    live = torch.zeros((V,), dtype=torch.bool, device=v.device)
    live[rows] = True
    factors = [lam] * iterations if method == "laplacian" else [lam, mu] * iterations
    p = v
    for fac in factors:
        pn = p[nbr]
        if weights == "uniform":
            w = torch.ones((int(nbr.shape[0]),), dtype=torch.float64, device=v.device)
        else:
            d = pn - p[rows]
            w = 1.0 / (torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).double() + 1e-12)
        W = torch.zeros((V,), dtype=torch.float64, device=v.device).index_add_(0, rows, w)
        S = torch.zeros((V, 3), dtype=torch.float64, device=v.device).index_add_(0, rows, w[:, None] * pn.double())
        x = p.double()
        q = (x + fac * (S / W[:, None] - x)).float()
        p = torch.where(live[:, None], q, p)
    return p


def stage_times(fn, runs, dev):
    """{group: ms per call} of the native call's launches, from the library's event timers"""
    lib = _abi.lib()
    fn()
    torch.cuda.synchronize(dev)
    lib.sls_timing_enable(1)
    for _ in range(runs):
        fn()
    torch.cuda.synchronize(dev)
    ns = lib.sls_timing_slots()
    tot, cnt = (C.c_double * ns)(), (C.c_int64 * ns)()
    lib.sls_timing_collect(tot, cnt)
    lib.sls_timing_enable(0)
    raw = {lib.sls_timing_name(s).decode(): tot[s] / runs for s in range(ns) if cnt[s]}
    out = {"sort": sum(v for k, v in raw.items() if k.startswith("sort_"))}
    out.update({k[len("smooth_"):]: v for k, v in raw.items() if k.startswith("smooth_")})
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21a_mesh_smooth.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("mesh_smooth_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    n = a.iterations
    with torch.no_grad():
        vol = synthetic_volume(a.radius, a.voxel, a.floaters, dev)
        soup, faces = vol.extract()
        v, f = mesh_ops.clean_mesh(soup, faces, normals=False)
        V = int(v.shape[0])
        res = {"what": "mesh_ops.vertex_adjacency / mesh_ops.smooth (sls_mesh_adjacency, sls_mesh_smooth) against a torch composition with "
                       "equal neighbour sets: torch.unique on the directed pairs, per sweep index_add_ of float64 weights and weighted positions",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "soup_triangles": int(faces.shape[0]),
               "vertices": V, "triangles": int(f.shape[0]), "iterations": n,
               "protocol": f"one process, both sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed "
                           "region; the stage groups from event timers in a run of their own",
               "device": torch.cuda.get_device_name(0)}
        offsets, nbr, boundary, det = mesh_ops.vertex_adjacency(f, V, details=True)
        crows, cnbr, coffsets = composed_adjacency(f, V)
        assert torch.equal(nbr.long(), cnbr) and torch.equal(offsets.long(), coffsets), "the neighbour sets differ"
        res["graph"] = det
        native_adj = lambda: mesh_ops.vertex_adjacency(f, V)                                                    # noqa: E731
        torch_adj = lambda: composed_adjacency(f, V)                                                             # noqa: E731
        res["adjacency_native_ms"], res["adjacency_composition_ms"] = alternate([native_adj, torch_adj], a.reps, dev)
        res["adjacency_speedup"] = round(res["adjacency_composition_ms"]["median"] / res["adjacency_native_ms"]["median"], 3)
        res["runs"], failures = [], []
        for method, weights in (("taubin", "inverse_distance"), ("taubin", "uniform"), ("laplacian", "inverse_distance")):
            sweeps = 2 * n if method == "taubin" else n
            gv = mesh_ops.smooth(v, f, n, method=method, weights=weights)
            again = mesh_ops.smooth(v, f, n, method=method, weights=weights)
            assert torch.equal(gv.view(torch.int32), again.view(torch.int32)), "two native runs differ"
            cv = composed_smooth(v, f, n, method, weights, 0.5, -0.53)
            worst = float((gv.double() - cv.double()).abs().max())
            scale = float(v.abs().max())
            tol = 4 * sweeps * scale * 2.0 ** -24      # an ulp of the largest coordinate now and then, carried through the sweeps
            if not worst <= tol:
                failures.append(f"{method}/{weights}: positions differ by {worst} > {tol}")
            native = lambda k=n: mesh_ops.smooth(v, f, k, method=method, weights=weights)                        # noqa: E731
            torch_side = lambda k=n: composed_smooth(v, f, k, method, weights, 0.5, -0.53)                       # noqa: E731
            run = {"method": method, "weights": weights, "sweeps": sweeps, "positions_max_abs_difference": worst, "tolerance": tol,
                   "differing_vertices": int((gv.view(torch.int32) != cv.view(torch.int32)).any(1).sum()), "native_runs_equal": True}
            run["native_ms"], run["composition_ms"], nat0, comp0 = alternate([native, torch_side, lambda: native(0), lambda: torch_side(0)],
                                                                              a.reps, dev)
            run["native_build_and_copy_ms"], run["composition_build_ms"] = nat0, comp0
            run["native_sweep_ms"] = round((run["native_ms"]["median"] - nat0["median"]) / sweeps, 5)
            run["composition_sweep_ms"] = round((run["composition_ms"]["median"] - comp0["median"]) / sweeps, 5)
            run["call_speedup"] = round(run["composition_ms"]["median"] / run["native_ms"]["median"], 3)
            run["sweep_speedup"] = round(run["composition_sweep_ms"] / run["native_sweep_ms"], 3)
            run["stage_ms"] = stage_times(native, a.reps, dev)
            res["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
