#!/usr/bin/env python3
"""Times the signed point-to-mesh distance (splat_loam_amd.evaluation.mesh_pseudonormals -> sls_mesh_pseudonormals,
signed_distance -> sls_mesh_signed_distance) on the synthetic cleaned mesh of the other mesh benches, and checks first
that the sides agree:

    python tools/signed_distance_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--out FILE.json]

Mesh: `mesh_clean_bench.synthetic_volume` (a sphere of radius 10 m at 0.1 m voxels with floaters) extracted and cleaned:
about 1.13 M triangles.  Queries: points drawn from the mesh (`sample_mesh`, seeded) and moved by 2 cm of Gaussian noise.

Three measurements, one process, all sides alternating, 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize
inside the timed region:
  1. `mesh_pseudonormals` alone;
  2. the table build against a torch composition of the same tables in float64: cross products, `atan2`-weighted normals
     summed over the corners with `index_add_`, the edge groups from `torch.unique` over the edge keys.  Asserted first: the
     three tables agree within 1e-6;
  3. `signed_distance` with the tables built before against `point_to_mesh`, per size: the difference is what the sign
     costs.  Asserted first: two runs give equal bytes, |sdist| is the root of point_to_mesh's dist2 bit for bit, the faces
     are equal."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from mesh_clean_bench import alternate, synthetic_volume
from splat_loam_amd import evaluation, mesh_ops


def torch_tables(v, f):
    """(face_n (F,3), edge_n (F,3,3), vertex_n (V,3)) float32 from float64 sums; no index-degenerate faces"""
    p = v.double()[f.long()]                                                            # (F, 3, 3)
    n = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = n.norm(dim=1, keepdim=True)
    fn = torch.where(ln > 0, n / ln.clamp_min(1e-300), torch.zeros_like(n))
    vn = torch.zeros((v.shape[0], 3), dtype=torch.float64, device=v.device)
    fl = f.long()
    for k in range(3):
        u, w = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        theta = torch.atan2(torch.linalg.cross(u, w).norm(dim=1), (u * w).sum(1))
        vn.index_add_(0, fl[:, k], torch.where(ln > 0, theta[:, None], torch.zeros_like(ln)) * fn)
    nxt = fl.roll(-1, 1)
    key = (torch.minimum(fl, nxt) * (int(v.shape[0]) + 1) + torch.maximum(fl, nxt)).reshape(-1)
    _, group = torch.unique(key, return_inverse=True)
    sums = torch.zeros((int(group.max()) + 1, 3), dtype=torch.float64, device=v.device)
    sums.index_add_(0, group, fn.repeat_interleave(3, dim=0))
    return fn.float(), sums[group].view(-1, 3, 3).float(), vn.float()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r36a_signed_distance.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("signed_distance_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        soup, faces = synthetic_volume(a.radius, a.voxel, a.floaters, dev).extract()
        v, f = mesh_ops.clean_mesh(soup, faces, normals=False)
        del soup, faces
        pn, details = evaluation.mesh_pseudonormals(v, f, return_details=True)
        pn2 = evaluation.mesh_pseudonormals(v, f)
        for x, y in ((pn.face_normals, pn2.face_normals), (pn.edge_normals, pn2.edge_normals), (pn.vertex_normals, pn2.vertex_normals)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "two table builds differ"
        assert details["degenerate_faces"] == 0, "the torch composition is written for meshes without index-degenerate faces"
        tfn, ten, tvn = torch_tables(v, f)
        diff = [float((x - y).abs().max()) for x, y in ((pn.face_normals, tfn), (pn.edge_normals, ten), (pn.vertex_normals, tvn))]
        assert max(diff) <= 1e-6, f"tables differ from the torch composition: {diff}"
        t_nat, t_tor = alternate([lambda: evaluation.mesh_pseudonormals(v, f), lambda: torch_tables(v, f)], a.reps, dev)
        res = {"what": "evaluation.mesh_pseudonormals (sls_mesh_pseudonormals) alone and vs a float64 torch composition (atan2-weighted "
                       "index_add_ over corners, torch.unique over the edge keys); evaluation.signed_distance with prebuilt tables "
                       "(sls_mesh_signed_distance) vs evaluation.point_to_mesh (sls_mesh_distance)",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "vertices": int(v.shape[0]),
               "triangles": int(f.shape[0]), "mesh": details,
               "protocol": f"one process, all sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the "
                           "timed region; agreement asserted first",
               "device": torch.cuda.get_device_name(0),
               "tables": {"native_ms": t_nat, "torch_ms": t_tor, "native_faster_than_torch": bool(t_nat["median"] < t_tor["median"]),
                          "max_abs_difference_face_edge_vertex": diff},
               "sizes": []}
        print(json.dumps(res["tables"]), flush=True)
        for M in a.sizes:
            g = torch.Generator(device=dev).manual_seed(M)
            q = evaluation.sample_mesh(v, f, M, seed=M) + 0.02 * torch.randn((M, 3), device=dev, generator=g)

            def signed():
                return evaluation.signed_distance(q, v, f, return_face=True, pseudonormals=pn)

            def unsigned():
                return evaluation.point_to_mesh(q, v, f)

            sd, face = signed()
            sd2, face2 = signed()
            assert torch.equal(sd.view(torch.int32), sd2.view(torch.int32)) and torch.equal(face, face2), "two signed runs differ"
            d2, pface = unsigned()
            assert torch.equal(face, pface), "the faces differ from point_to_mesh's"
            assert np.abs(sd.cpu().numpy()).tobytes() == np.sqrt(d2.cpu().numpy()).tobytes(), "|sdist| is not the root of dist2"
            t_s, t_u = alternate([signed, unsigned], a.reps, dev)
            row = {"Mq": M, "signed_ms": t_s, "unsigned_ms": t_u, "sign_costs_ms": t_s["median"] - t_u["median"],
                   "sign_share_of_search": (t_s["median"] - t_u["median"]) / t_u["median"],
                   "signed_mean_m": float(sd.double().mean()), "share_behind": float((sd < 0).double().mean())}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
