#!/usr/bin/env python3
"""Times the mesh cleaning stage (splat_loam_amd.mesh_ops -> sls_mesh_weld / _clusters / _filter / _vertex_normals)
against what a user without it would write, and checks that both give the same mesh:

    python tools/mesh_clean_bench.py [--radius 10] [--voxel 0.1] [--floaters 24] [--reps 10] [--out FILE.json]

Data: a synthetic TSDF volume — a sphere of --radius metres and --floaters small detached spheres (radius 3 voxels) around
it, tsdf set analytically at every voxel centre of the blocks the surfaces touch — extracted by TsdfVolume.extract: a
soup of about a million triangles at the defaults.

  weld        mesh_ops.weld against tsdf.weld_soup (torch.unique over the int32 view of 3T rows); the results are equal
  clean_mesh  weld + keep_clusters=1, min_triangles=50 + vertex normals, one host read, against the composition of the
              same rules: torch.unique, the edge list sorted with NumPy on the host, a union-find on the host (hooking
              the larger root under the smaller, pointer jumping, vectorised with NumPy), the selection with NumPy, the
              normals with torch (index_add_ on the device).  Vertices and faces must be equal; the normals differ by
              the order of torch's float atomics, the largest difference is reported
  the stages of clean_mesh are also timed one by one (each with its own host read).
Both sides of a comparison run in one process and alternate; 3 warm-ups, the median of --reps (>= 10),
torch.cuda.synchronize inside the timed region."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from splat_loam_amd import mesh_ops, tsdf


def synthetic_volume(radius, voxel, n_floaters, dev, seed=3):
    """A TsdfVolume whose zero surface is a sphere and n_floaters small spheres just outside it."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    trunc = 4 * voxel
    d = torch.randn((n_floaters, 3), generator=g, dtype=torch.float64)
    centres = torch.cat([torch.zeros((1, 3), dtype=torch.float64), d / d.norm(dim=1, keepdim=True) * (radius + 12 * voxel)]) + 0.0371
    radii = torch.cat([torch.tensor([float(radius)], dtype=torch.float64), torch.full((n_floaters,), 3.0 * voxel, dtype=torch.float64)])
    pts = []
    for c, r in zip(centres, radii):                            # points on every surface, a few per block it crosses
        n = int(max(2000, 40 * 4 * np.pi * float(r) ** 2 / (8 * voxel) ** 2))
        u = torch.randn((n, 3), generator=g, dtype=torch.float64)
        pts.append(c + u / u.norm(dim=1, keepdim=True) * r)
    blocks = tsdf.allocate_blocks(torch.cat(pts).float().to(dev), voxel, trunc)
    vol = tsdf.TsdfVolume(blocks, voxel, trunc)
    l = torch.arange(512, device=dev)
    local = torch.stack([l & 7, (l >> 3) & 7, l >> 6], 1)
    c = ((8 * blocks.long()[:, None, :] + local[None]).double() + 0.5) * voxel
    dist = torch.full(c.shape[:2], float("inf"), dtype=torch.float64, device=dev)
    for ci, ri in zip(centres.to(dev), radii.to(dev)):
        dist = torch.minimum(dist, (c - ci).norm(dim=2) - ri)
    vol.tsdf.copy_((dist / trunc).clamp(-1.0, 1.0).float())
    vol.weight.fill_(1.0)
    return vol


def host_union_find(a, b, T):
    """parent (T,) after uniting every pair (a[i], b[i]): the root of a component is its lowest member."""
    parent = np.arange(T, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        m = lo != hi
        if not m.any():
            return parent
        np.minimum.at(parent, hi[m], lo[m])                     # hook the larger root under the smaller
        while True:                                             # pointer jumping until every node points at its root
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp


def composed_clean(soup, keep_clusters=1, min_triangles=50):
    """The rules of include/sls_mesh_math.h with torch.unique, NumPy on the host and torch.index_add_."""
    v, f = tsdf.weld_soup(soup)
    V, fh = int(v.shape[0]), f.cpu().numpy().astype(np.int64)
    T = len(fh)
    ok = (fh[:, 0] != fh[:, 1]) & (fh[:, 1] != fh[:, 2]) & (fh[:, 2] != fh[:, 0])
    e = np.concatenate([fh[:, [0, 1]], fh[:, [1, 2]], fh[:, [2, 0]]])
    key = np.minimum(e[:, 0], e[:, 1]) * V + np.maximum(e[:, 0], e[:, 1])
    tri = np.tile(np.arange(T), 3)
    keep = np.tile(ok, 3)
    key, tri = key[keep], tri[keep]
    order = np.argsort(key, kind="stable")
    key, tri = key[order], tri[order]
    same = key[1:] == key[:-1]
    parent = host_union_find(tri[1:][same], tri[:-1][same], T)
    roots, labels = np.unique(parent[ok], return_inverse=True)
    counts = np.bincount(labels, minlength=len(roots))
    k = min(keep_clusters, len(counts)) if keep_clusters > 0 else 0
    n_min = max(max(min_triangles, 0), int(np.sort(counts)[::-1][k - 1]) if k > 0 else 0)
    kept = np.zeros((T,), bool)
    kept[ok] = counts[labels] >= n_min
    fk = fh[kept]
    used = np.zeros((V,), bool)
    used[fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    dev = soup.device
    v2 = v[torch.from_numpy(used).to(dev)]
    f2 = torch.from_numpy(remap[fk].astype(np.int32)).to(dev)
    p = v2[f2.long()]
    fn = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
    s = torch.zeros_like(v2)
    for c in range(3):
        s.index_add_(0, f2[:, c].long(), fn)
    length = s.norm(dim=1, keepdim=True)
    n = torch.where((length > 0) & torch.isfinite(length), s / length, torch.zeros_like(s))
    return v2, f2, n, {"clusters": int(len(counts)), "n_min": int(n_min)}


def alternate(fns, reps, dev, warm=3):
    times = [[] for _ in fns]
    for it in range(warm + reps):
        for fn, acc in zip(fns, times):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(dev)
            if it >= warm:
                acc.append((time.perf_counter() - t0) * 1e3)
            del out
    return [{"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))} for t in times]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19a_mesh_clean.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("mesh_clean_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        vol = synthetic_volume(a.radius, a.voxel, a.floaters, dev)
        soup, faces = vol.extract()
        T = int(faces.shape[0])
        res = {"what": "mesh_ops.weld / clean_mesh (sls_mesh_weld, sls_mesh_clusters, sls_mesh_filter, sls_mesh_vertex_normals) against "
                       "torch.unique and a torch + NumPy composition with a union-find on the host",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "blocks": int(vol.blocks.shape[0]),
               "triangles": T, "soup_rows": 3 * T,
               "protocol": f"one process, both sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region",
               "device": torch.cuda.get_device_name(0)}
        # weld
        gv, gf = mesh_ops.weld(soup)
        wv, wf = tsdf.weld_soup(soup)
        res["weld"] = {"vertices": int(gv.shape[0]), "equal": bool(torch.equal(gv.view(torch.int32), wv.view(torch.int32)) and torch.equal(gf, wf))}
        res["weld"]["native_ms"], res["weld"]["torch_unique_ms"] = alternate([lambda: mesh_ops.weld(soup), lambda: tsdf.weld_soup(soup)], a.reps, dev)
        # the whole chain
        v, f, n, det = mesh_ops.clean_mesh(soup, faces, details=True)
        cv, cf, cn, cdet = composed_clean(soup)
        res["clean_mesh"] = {"clusters": det["clusters"], "n_min": det["n_min"], "degenerate": det["degenerate"],
                             "boundary_edges": det["boundary_edges"], "nonmanifold_edges": det["nonmanifold_edges"],
                             "vertices_kept": int(v.shape[0]), "triangles_kept": int(f.shape[0]),
                             "composition_clusters": cdet["clusters"], "composition_n_min": cdet["n_min"],
                             "mesh_equal": bool(torch.equal(v.view(torch.int32), cv.view(torch.int32)) and torch.equal(f, cf)),
                             "normals_max_abs_difference": float((n - cn).abs().max()) if n.shape == cn.shape else None}
        res["clean_mesh"]["native_ms"], res["clean_mesh"]["composition_ms"] = alternate(
            [lambda: mesh_ops.clean_mesh(soup, faces), lambda: composed_clean(soup)], a.reps, dev)
        # the stages, each with its own host read
        V = int(gv.shape[0])
        stages = alternate([lambda: mesh_ops.cluster_triangles(gf, V), lambda: mesh_ops.keep_clusters(gv, gf), lambda: mesh_ops.vertex_normals(v, f)],
                           a.reps, dev)
        res["stages_ms"] = dict(zip(("cluster_triangles", "keep_clusters (clusters + filter)", "vertex_normals"), stages))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
