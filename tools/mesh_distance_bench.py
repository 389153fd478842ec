#!/usr/bin/env python3
"""Times the exact point-to-mesh distance (splat_loam_amd.evaluation.point_to_mesh -> sls_mesh_distance) against a chunked
torch brute force and against the sampled route `evaluate_recon` takes by default, on the synthetic cleaned mesh of the
other mesh benches, and checks first that they agree:

    python tools/mesh_distance_bench.py [--sizes 50000 500000 2000000] [--reps 10] [--torch-chunks 2] [--out FILE.json]

Mesh: `mesh_clean_bench.synthetic_volume` (a sphere of radius 10 m at 0.1 m voxels with floaters) extracted and cleaned:
about 1.13 M triangles.  Queries: points drawn from the mesh (`sample_mesh`, seeded) and moved by 2 cm of Gaussian noise —
a reference cloud lying near the surface, what `evaluate_recon(completeness="exact")` asks.

torch brute force: --torch-rows queries x ALL faces per chunk, float32, the same candidates as the header (three clamped
edge segments and the plane's foot point where it falls inside), min over the faces.  It costs Mq x F triangle
distances, so only --torch-chunks chunks are timed, on the FIRST queries, and the file says how many: `torch_ms` is the
time measured for those queries alone, `torch_ms_all_queries_extrapolated` scales it by Mq / queries timed.
Sampled route: `sample_mesh(10 M, seeded)`, `voxel_down_sample(0.02)`, `nearest` — distance to the nearest SAMPLE, an
upper bound of the exact distance, for all Mq queries.  The native call always serves all Mq queries.

Asserted before anything is timed: two native runs give equal bytes; on the brute force's queries, in float64, the
distance to the face the native call names is within 1e-5 of the scale of the float64 minimum over all faces; every
exact distance is <= the distance to the nearest of the 10 M samples themselves * (1 + 1e-5) + 1e-6 m (the samples lie on
the faces; their voxel averages, which the sampled route measures against, leave a curved surface by about res^2 / 8 R).
One process, all sides alternating, 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize inside the timed
region."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from mesh_clean_bench import alternate, synthetic_volume
from splat_loam_amd import evaluation, mesh_ops


def brute_force(q, a, b, c, dtype):
    """(rows,) min over all faces of the squared distance, (rows,) argmin: q (rows,3), a / b / c (F,3)"""
    q, a, b, c = (x.to(dtype) for x in (q, a, b, c))
    A, B, Cc = a[None] - q[:, None], b[None] - q[:, None], c[None] - q[:, None]        # (rows, F, 3)

    def segment(P, e):
        ee = (e * e).sum(-1)
        t = (-(P * e).sum(-1) / ee.clamp_min(1e-38)).clamp_(0.0, 1.0)
        p = P + t[..., None] * e
        return (p * p).sum(-1)
    ab, bc, ca = B - A, Cc - B, A - Cc
    d2 = torch.minimum(torch.minimum(segment(A, ab), segment(B, bc)), segment(Cc, ca))
    n = torch.linalg.cross(ab, -ca)
    nn = (n * n).sum(-1)
    va = (n * torch.linalg.cross(B, bc)).sum(-1)
    vb = (n * torch.linalg.cross(Cc, ca)).sum(-1)
    vc = (n * torch.linalg.cross(A, ab)).sum(-1)
    h = (A * n).sum(-1)
    plane = h * h / nn.clamp_min(1e-38)
    inside = (va > 0) & (vb > 0) & (vc > 0)
    d2 = torch.where(inside, torch.minimum(d2, plane), d2)
    return d2.min(dim=1)


def face_dist64(q, v, f, face):
    """float64 distance of every query to ITS face, and the scale: the largest distance to the face's vertices"""
    tri = v[f[face.long()].long()].double()                                             # (M, 3, 3)
    d2 = torch.stack([brute_force(q[i:i + 1], tri[i:i + 1, 0], tri[i:i + 1, 1], tri[i:i + 1, 2], torch.float64)[0] for i in range(len(q))]).view(-1)
    scale = (tri - q.double()[:, None]).norm(dim=2).max(dim=1).values
    return d2.sqrt(), scale


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--floaters", type=int, default=24)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 500000, 2000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-rows", type=int, default=64)
    ap.add_argument("--torch-chunks", type=int, default=2)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32a_mesh_distance.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("mesh_distance_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        soup, faces = synthetic_volume(a.radius, a.voxel, a.floaters, dev).extract()
        v, f = mesh_ops.clean_mesh(soup, faces, normals=False)
        del soup, faces
        va, vb, vc = (v[f[:, k].long()].contiguous() for k in range(3))
        res = {"what": "evaluation.point_to_mesh (sls_mesh_distance, all Mq queries, distances + faces) vs a chunked torch brute force "
                       "(torch_ms covers torch_queries_timed queries only) and vs the sampled route (sample_mesh + voxel_down_sample + "
                       "nearest, all Mq queries)",
               "data": "synthetic", "radius": a.radius, "voxel_size": a.voxel, "floaters": a.floaters, "vertices": int(v.shape[0]),
               "triangles": int(f.shape[0]), "samples": a.samples,
               "protocol": f"one process, all sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the "
                           "timed region; agreement asserted first",
               "device": torch.cuda.get_device_name(0), "sizes": []}
        n_timed = a.torch_rows * a.torch_chunks
        for M in a.sizes:
            g = torch.Generator(device=dev).manual_seed(M)
            q = evaluation.sample_mesh(v, f, M, seed=M) + 0.02 * torch.randn((M, 3), device=dev, generator=g)

            def native():
                return evaluation.point_to_mesh(q, v, f)

            def torch_side():
                return [brute_force(q[i:i + a.torch_rows], va, vb, vc, torch.float32) for i in range(0, n_timed, a.torch_rows)]

            def sampled():
                est = evaluation.voxel_down_sample(evaluation.sample_mesh(v, f, a.samples, seed=0), 0.02)
                return evaluation.nearest(est, q, return_index=False)[0]

            d2, face = native()
            d2b, faceb = native()
            assert torch.equal(d2.view(torch.int32), d2b.view(torch.int32)) and torch.equal(face, faceb), "two native runs differ"
            head = min(n_timed, M)
            truth = torch.cat([brute_force(q[i:i + a.torch_rows], va, vb, vc, torch.float64)[0] for i in range(0, head, a.torch_rows)]).sqrt()
            mine, scale = face_dist64(q[:head], v, f, face[:head])
            excess = float(((mine - truth) / scale).max())
            assert excess <= 1e-5, f"the returned face is {excess} of the scale farther than the float64 minimum"
            d_sampled = sampled().double().sqrt()
            # the samples themselves lie ON the faces; their voxel averages leave a curved surface by about res^2 / 8 R
            d_raw = evaluation.nearest(evaluation.sample_mesh(v, f, a.samples, seed=0), q, return_index=False)[0].double().sqrt()
            over = float((d2.double().sqrt() - (d_raw * (1 + 1e-5) + 1e-6)).max())
            assert over <= 0.0, f"an exact distance exceeds its distance to the nearest sample by {over} m"
            t_nat, t_tor, t_sam = alternate([native, torch_side, sampled], a.reps, dev)
            row = {"Mq": M, "native_ms": t_nat, "torch_ms": t_tor, "sampled_route_ms": t_sam, "torch_queries_timed": head,
                   "torch_chunk_rows": a.torch_rows, "torch_ms_all_queries_extrapolated": t_tor["median"] * M / head,
                   "native_faster_than_torch_extrapolated": bool(t_nat["median"] < t_tor["median"] * M / head),
                   "native_faster_than_sampled_route": bool(t_nat["median"] < t_sam["median"]),
                   "returned_face_excess_of_scale_float64": excess,
                   "mean_exact_m": float(d2.double().sqrt().mean()), "mean_sampled_m": float(d_sampled.mean()),
                   "exact_minus_sampled_route_max_m": float((d2.double().sqrt() - d_sampled).max())}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
