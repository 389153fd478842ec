#!/usr/bin/env python3
"""Times mesh simplification by vertex clustering (splat_loam_amd.mesh_ops.simplify_vertex_clustering -> sls_mesh_simplify)
against what a user without it would write, and checks that both give the same mesh:

    python tools/mesh_simplify_bench.py [--radius 10] [--voxel 0.1] [--floaters 24] [--reps 10] [--out FILE.json]

Data: the synthetic TSDF volume of tools/mesh_clean_bench.py (a sphere of --radius metres, about 1.15 M triangles at the
defaults), extracted and cleaned with mesh_ops.clean_mesh.  The cleaned mesh is simplified at 2 and 4 times the fusion
voxel with both contractions.

  composition  the rules of include/sls_simplify_math.h in torch: the live vertices by a scatter of ones, the voxel keys,
               torch.unique over the keys, index_add_ for the float64 means, torch.unique(dim=0) over the rotated cluster
               triples (the first occurrence by scatter_reduce amin), and for the quadric index_add_ of the nine float64
               words per corner and the 3 x 3 solve on the host with NumPy
  checks       faces and average vertices must be EQUAL (float64 sums of float32 coordinates of this magnitude are exact in
               any order); the quadric vertices agree within 1e-5 voxel_size (torch's float64 atomics add in another order)
  stages       the native call's launches by group through sls_timing_enable(1), in a run of their own: the sorts (three, and
               the corner sort of the quadric), cluster (live flags, bounding box, keys, segments), faces (mapping,
               de-duplication, the two compactions), corners (the corner keys), place (segment sums, and for the quadric
               the quadric sums and the solve)
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
from splat_loam_amd import _abi, mesh_ops

NO_KEY = (1 << 63) - 1


def composed_simplify(v, f, h, contraction, lam):
    """(vertices', faces' int32) by the rules of include/sls_simplify_math.h with torch.unique and index_add_."""
    dev, V = v.device, int(v.shape[0])
    fl = f.long()
    ok = ((fl >= 0) & (fl < V)).all(1) & (fl[:, 0] != fl[:, 1]) & (fl[:, 1] != fl[:, 2]) & (fl[:, 2] != fl[:, 0])
    fo = fl[ok]
    live = torch.zeros((V,), dtype=torch.bool, device=dev)
    live[fo.reshape(-1)] = True
    vd = v.double()
    origin = v[live].min(0).values.double() - 0.5 * h
    idx = torch.floor((vd - origin) / h).long()
    key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
    key = torch.where(live, key, torch.full_like(key, NO_KEY))
    uniq, cid = torch.unique(key, return_inverse=True)             # sorted: the vertices without a cluster come last
    nc = int(uniq.shape[0])
    sums = torch.zeros((nc, 3), dtype=torch.float64, device=dev).index_add_(0, cid, vd)
    mean = sums / torch.bincount(cid, minlength=nc).double()[:, None]
    c = cid[fo]
    distinct = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 2] != c[:, 0])
    cand = c[distinct]
    k = cand.argmin(1)
    rows = torch.gather(cand, 1, (k[:, None] + torch.arange(3, device=dev)[None]) % 3)
    urows, inv = torch.unique(rows, dim=0, return_inverse=True)
    first = torch.full((int(urows.shape[0]),), int(rows.shape[0]), dtype=torch.long, device=dev)
    first.scatter_reduce_(0, inv, torch.arange(int(rows.shape[0]), device=dev), reduce="amin")
    kept = rows[torch.sort(first).values]
    surv = torch.zeros((nc,), dtype=torch.bool, device=dev)
    surv[kept.reshape(-1)] = True
    cnew = torch.cumsum(surv, 0) - 1
    out_f = cnew[kept].int()
    if contraction == "average":
        return mean[surv].float(), out_f
    p0, p1, p2 = (vd[fo[:, j]] for j in range(3))
    cr = torch.cross(p1 - p0, p2 - p0, dim=1)
    L = cr.norm(dim=1)
    good = (L > 0) & torch.isfinite(L)
    n = cr / torch.where(good, L, torch.ones_like(L))[:, None]
    w = torch.where(good, 0.5 * L, torch.zeros_like(L))
    s = (n * p0).sum(1)
    q = torch.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                     s * n[:, 0], s * n[:, 1], s * n[:, 2]], 1) * w[:, None]
    acc = torch.zeros((nc, 9), dtype=torch.float64, device=dev)
    for j in range(3):
        acc.index_add_(0, c[:, j], q)
    # the 3 x 3 solve on the host
    a, m = acc[surv].cpu().numpy(), mean[surv].cpu().numpy()
    A = a[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    tr = a[:, 0] + a[:, 3] + a[:, 5]
    M = A + (lam * tr)[:, None, None] * np.eye(3)[None]
    r = a[:, 6:9] - np.einsum("nij,nj->ni", A, m)
    det = np.linalg.det(M)
    solvable = (tr > 0) & (det > 0)
    d = np.zeros_like(m)
    d[solvable] = np.linalg.solve(M[solvable], r[solvable][:, :, None])[:, :, 0]
    fell = ~solvable | ~np.isfinite(d).all(1) | (np.abs(d) > h).any(1)
    d[fell] = 0.0
    return torch.from_numpy((m + d).astype(np.float32)).to(dev), out_f


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
    out = {"sorts": sum(v for k, v in raw.items() if k.startswith("sort_"))}
    out.update({k[len("simp_"):]: v for k, v in raw.items() if k.startswith("simp_")})
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regularisation", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20a_mesh_simplify.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("mesh_simplify_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        vol = synthetic_volume(a.radius, a.voxel, a.floaters, dev)
        soup, faces = vol.extract()
        v, f = mesh_ops.clean_mesh(soup, faces, normals=False)
        res = {"what": "mesh_ops.simplify_vertex_clustering (sls_mesh_simplify) against a torch composition: torch.unique on the voxel keys, "
                       "index_add_ means, torch.unique(dim=0) on the rotated faces, the quadric solved on the host",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "soup_triangles": int(faces.shape[0]),
               "vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "regularisation": a.regularisation,
               "protocol": f"one process, both sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed "
                           "region; the stage groups from event timers in a run of their own",
               "device": torch.cuda.get_device_name(0), "runs": []}
        for factor in (2, 4):
            h = factor * a.voxel
            for how in ("average", "quadric"):
                native = lambda: mesh_ops.simplify_vertex_clustering(v, f, h, contraction=how, regularisation=a.regularisation)     # noqa: E731
                torch_side = lambda: composed_simplify(v, f, h, how, a.regularisation)                                           # noqa: E731
                gv, gf, det = mesh_ops.simplify_vertex_clustering(v, f, h, contraction=how, regularisation=a.regularisation, details=True)
                cv, cf = torch_side()
                assert torch.equal(gf, cf), f"faces differ at {factor} voxels, {how}"
                assert gv.shape == cv.shape
                worst = float((gv.double() - cv.double()).abs().max())
                if how == "average":
                    assert torch.equal(gv.view(torch.int32), cv.view(torch.int32)), f"average vertices differ at {factor} voxels: {worst}"
                else:
                    assert worst <= 1e-5 * h, f"quadric vertices differ by {worst} at {factor} voxels"
                edges = mesh_ops.cluster_triangles(gf, int(gv.shape[0]), details=True)[2]
                run = {"voxels": factor, "simplify_voxel": h, "contraction": how,
                       **{k: det[k] for k in ("vertices", "triangles", "collapsed", "duplicates", "fallbacks")},
                       "triangle_reduction": round(int(f.shape[0]) / max(det["triangles"], 1), 3),
                       "boundary_edges": edges["boundary_edges"], "nonmanifold_edges": edges["nonmanifold_edges"],
                       "faces_equal": True, "vertices_max_abs_difference": worst}
                run["native_ms"], run["composition_ms"] = alternate([native, torch_side], a.reps, dev)
                run["speedup"] = round(run["composition_ms"]["median"] / run["native_ms"]["median"], 3)
                run["stage_ms"] = stage_times(native, a.reps, dev)
                res["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
