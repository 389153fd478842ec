#!/usr/bin/env python3
"""Times hole filling (splat_loam_amd.mesh_ops.boundary_loops / fill_holes -> sls_mesh_boundary_loops, sls_mesh_fill_holes)
against what a user without it would write, and checks that both give the same mesh:

    python tools/mesh_fill_bench.py [--radius 10] [--voxel 0.1] [--floaters 24] [--rings 2000] [--caps 12] [--reps 10] [--out FILE.json]

Data: the synthetic TSDF volume of tools/mesh_clean_bench.py (a sphere of --radius metres, about 1.15 M triangles at the
defaults), extracted and cleaned with mesh_ops.clean_mesh, then holes punched into it with a seeded generator: the one-rings
of --rings random vertices, and --caps larger caps (every triangle within 2 to 12 voxels of a random vertex).

  host         the rules of include/sls_fill_math.h with NumPy on the host: the faces copied down, np.unique on the edge
               keys, np.bincount for the degrees, a walk along the next pointers, the float64 sums in the header's order,
               the result copied up again
  loops        mesh_ops.boundary_loops against the host's half-edges, loop numbers and lengths: equal
  fill         mesh_ops.fill_holes against the host's vertices and faces: equal bit for bit (asserted before any timing)
  sort share   the sorter's launches through sls_timing_enable(1), in a run of their own, as a share of the call
  clean_mesh   clean_mesh(fill_holes=64) - clean_mesh() on the mesh with holes: what the stage adds to the chain
  does it help the sphere with holes of the tests (tests/fill_ref.py: sphere_caps), evaluate_recon against points sampled
               from the whole sphere, before and after fill_holes(max_edges=128)
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

import numpy as np
import torch

from mesh_clean_bench import alternate, synthetic_volume
from splat_loam_amd import _abi, evaluation, mesh_ops

LONG = 64


def punch(v, f, rings, caps, voxel, seed=5):
    """the faces without the one-rings of `rings` seeded vertices and without `caps` seeded caps"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    V = int(v.shape[0])
    hubs = torch.randperm(V, generator=g)[:rings].to(v.device)
    gone = torch.zeros((V,), dtype=torch.bool, device=v.device)
    gone[hubs] = True
    drop = gone[f.long()].any(1)
    centres = v[torch.randperm(V, generator=g)[:caps].to(v.device)]
    radii = (2.0 + 10.0 * torch.rand((caps,), generator=g)).to(v.device) * voxel
    for c, r in zip(centres, radii):
        drop |= ((v - c).norm(dim=1) < r)[f.long()].all(1)
    return f[~drop].contiguous()


def segment_sum(items):
    n = len(items)
    if n <= LONG:
        return np.cumsum(items, axis=0)[-1]                         # one after the other
    part = np.zeros((LONG, items.shape[1]))
    for i0 in range(0, n, LONG):
        rows = items[i0:i0 + LONG]
        part[:len(rows)] = part[:len(rows)] + rows
    lanes = np.arange(LONG)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ off]
    return part[0]


def host_loops(f, V):
    """(halfedges (B,2), loop (B,), cycles) of device faces, on the host"""
    fh = f.cpu().numpy().astype(np.int64)
    ok = fh[((fh >= 0) & (fh < V)).all(1) & (fh[:, 0] != fh[:, 1]) & (fh[:, 1] != fh[:, 2]) & (fh[:, 2] != fh[:, 0])]
    d = np.concatenate([ok[:, [0, 1]], ok[:, [1, 2]], ok[:, [2, 0]]])
    key = np.minimum(d[:, 0], d[:, 1]) * V + np.maximum(d[:, 0], d[:, 1])
    _, inverse, owners = np.unique(key, return_inverse=True, return_counts=True)
    d = d[owners[inverse] == 1]
    d = d[np.argsort(d[:, 0] * V + d[:, 1], kind="stable")]
    B = len(d)
    out_n, in_n = np.bincount(d[:, 0], minlength=V), np.bincount(d[:, 1], minlength=V)
    simple = (out_n == 1) & (in_n == 1)
    leaving = np.full((V,), -1, np.int64)
    leaving[d[:, 0]] = np.arange(B)
    nxt = np.where(simple[d[:, 1]], leaving[d[:, 1]], -1)          # the half-edge that follows, where the head is simple
    good = simple[d[:, 0]] & simple[d[:, 1]]
    loop, cycles, seen = np.full((B,), -1, np.int64), [], np.zeros((B,), bool)
    nxt_l, good_l = nxt.tolist(), good.tolist()
    for h0 in range(B):                                             # ascending: a loop is met at its lowest half-edge first
        if seen[h0] or not good_l[h0]:
            continue
        chain, h, closed = [h0], nxt_l[h0], False
        while h >= 0 and good_l[h]:
            if h == h0:
                closed = True
                break
            chain.append(h)
            h = nxt_l[h]
        if closed:
            seen[chain] = True
            loop[chain] = len(cycles)
            cycles.append(chain)
    return d, loop, cycles


def host_fill(v, f, max_edges):
    """(vertices', faces') as device tensors: the host's fill, the copies down and up included"""
    V = int(v.shape[0])
    d, loop, cycles = host_loops(f, V)
    vh = v.cpu().numpy()
    new_v, new_f = [], []
    for cycle in cycles:
        L = len(cycle)
        if L > max_edges:
            continue
        tails = d[cycle]
        order = np.argsort(tails[:, 0])
        p = vh[tails[order, 0]]
        if not np.isfinite(p).all():
            continue
        if L == 3:
            new_f.append([tails[0, 0], d[cycle[1], 1], tails[0, 1]])
            continue
        c = V + len(new_v)
        new_v.append((segment_sum(p.astype(np.float64)) / np.float64(L)).astype(np.float32))
        fan = np.empty((L, 3), np.int64)
        fan[:, 0], fan[:, 1], fan[:, 2] = tails[order, 1], tails[order, 0], c
        new_f.append(fan)
    out_v = np.concatenate([vh, np.asarray(new_v, dtype=np.float32).reshape(-1, 3)])
    out_f = np.concatenate([f.cpu().numpy()] + [np.asarray(x, dtype=np.int32).reshape(-1, 3) for x in new_f])
    return torch.from_numpy(out_v).to(v.device), torch.from_numpy(out_f.astype(np.int32)).to(v.device)


def sort_ms(fn, runs, dev):
    """ms per call in the sorter's launches, from the library's event timers"""
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
    return round(sum(tot[s] / runs for s in range(ns) if cnt[s] and lib.sls_timing_name(s).decode().startswith("sort_")), 4)


def sphere_quality(dev):
    """evaluate_recon of the tests' sphere with holes against points of the whole sphere, before and after the fill"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fill_ref
    v, f = (torch.from_numpy(np.array(x)).to(dev) for x in fill_ref.sphere_caps())
    whole = torch.from_numpy(np.array(fill_ref.welded_sphere()[1])).to(dev)
    reference = evaluation.sample_mesh(v, whole, 400_000, seed=2)
    keys = ("MAE_completeness (cm)", "Recall [Completeness] (%)", "MAE_accuracy (cm)", "F-score (%)")
    out = {}
    for name, (mv, mf) in (("before", (v, f)), ("after", mesh_ops.fill_holes(v, f, max_edges=128))):
        m = evaluation.evaluate_recon(reference, mv, mf, down_sample_res=0.02, threshold=0.05, mesh_sample_point=400_000, seed=1)
        out[name] = {k: round(float(m[k]), 4) for k in keys}
    out["threshold_m"] = 0.05
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--rings", type=int, default=2000)
    ap.add_argument("--caps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22a_mesh_fill.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("mesh_fill_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        vol = synthetic_volume(a.radius, a.voxel, a.floaters, dev)
        soup, faces = vol.extract()
        v, whole = mesh_ops.clean_mesh(soup, faces, normals=False)
        f = punch(v, whole, a.rings, a.caps, a.voxel)
        V = int(v.shape[0])
        res = {"what": "mesh_ops.boundary_loops / mesh_ops.fill_holes (sls_mesh_boundary_loops, sls_mesh_fill_holes) against the same rule "
                       "with NumPy on the host: np.unique on the edge keys, a walk along the next pointers, the copies down and up included",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "rings": a.rings, "caps": a.caps,
               "vertices": V, "triangles_whole": int(whole.shape[0]), "triangles": int(f.shape[0]),
               "protocol": f"one process, both sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed "
                           "region; the sorter's share from event timers in a run of their own",
               "device": torch.cuda.get_device_name(0)}
        # equal before any timing
        he, loop, edges, det = mesh_ops.boundary_loops(f, V, details=True)
        hd, hloop, hcycles = host_loops(f, V)
        assert np.array_equal(he.cpu().numpy(), hd) and np.array_equal(loop.cpu().numpy(), hloop), "the loops differ"
        assert edges.cpu().tolist() == [len(c) for c in hcycles], "the loop lengths differ"
        gv, gf, fdet = mesh_ops.fill_holes(v, f, details=True)
        again = mesh_ops.fill_holes(v, f)
        assert torch.equal(gv.view(torch.int32), again[0].view(torch.int32)) and torch.equal(gf, again[1]), "two native runs differ"
        cv, cf = host_fill(v, f, 64)
        assert torch.equal(gv.view(torch.int32), cv.view(torch.int32)) and torch.equal(gf, cf), "the filled meshes differ"
        lengths = np.asarray(edges.cpu().tolist())
        res["loops"] = dict(det, longest=int(lengths.max()) if len(lengths) else 0, median=float(np.median(lengths)) if len(lengths) else 0.0,
                            at_most_64=int((lengths <= 64).sum()), above_64=int((lengths > 64).sum()))
        res["fill"] = fdet
        res["outputs_equal"] = True
        after = mesh_ops.cluster_triangles(gf, gv.shape[0], details=True)[2]
        res["boundary_edges_before"], res["boundary_edges_after"] = det["halfedges"], after["boundary_edges"]
        native_loops = lambda: mesh_ops.boundary_loops(f, V)                                                     # noqa: E731
        native_fill = lambda: mesh_ops.fill_holes(v, f)                                                          # noqa: E731
        res["loops_native_ms"], res["loops_host_ms"] = alternate([native_loops, lambda: host_loops(f, V)], a.reps, dev)
        res["fill_native_ms"], res["fill_host_ms"] = alternate([native_fill, lambda: host_fill(v, f, 64)], a.reps, dev)
        res["loops_speedup"] = round(res["loops_host_ms"]["median"] / res["loops_native_ms"]["median"], 3)
        res["fill_speedup"] = round(res["fill_host_ms"]["median"] / res["fill_native_ms"]["median"], 3)
        res["loops_sort_ms"], res["fill_sort_ms"] = sort_ms(native_loops, a.reps, dev), sort_ms(native_fill, a.reps, dev)
        res["loops_sort_share"] = round(res["loops_sort_ms"] / res["loops_native_ms"]["median"], 3)
        res["fill_sort_share"] = round(res["fill_sort_ms"] / res["fill_native_ms"]["median"], 3)
        plain = lambda: mesh_ops.clean_mesh(v, f)                                                                # noqa: E731
        filled = lambda: mesh_ops.clean_mesh(v, f, fill_holes=64)                                                # noqa: E731
        res["clean_mesh_ms"], res["clean_mesh_fill_ms"] = alternate([plain, filled], a.reps, dev)
        res["clean_mesh_added_ms"] = round(res["clean_mesh_fill_ms"]["median"] - res["clean_mesh_ms"]["median"], 4)
        res["sphere_with_holes"] = sphere_quality(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
