#!/usr/bin/env python3
"""Times the Poisson volume (splat_loam_amd.poisson -> sls_poisson_splat / sls_poisson_solve / sls_poisson_density) and
checks it against a torch composition of the same operator:

    python tools/poisson_bench.py [--reps 10] [--out FILE.json] [--quick]

Data: a synthetic room — the six faces of an 8 x 6 x 3 m box sampled uniformly with 5 mm of noise along inward normals —
at 50 k / 500 k / 2 M oriented samples and 0.1 m / 0.05 m voxels (--quick: the first size only).

  splat        PoissonVolume.splat against index_add_ of the eight trilinear weights (float32 atomics: another order)
  per pass     (solve with 60 passes - solve with 10 passes) / 50 at tol = 0, so that no run ends early; the yardstick is a
               sparse-CSR torch.sparse.mm PCG with the same preconditioner and stopping rule (one host read per pass: what a
               user without the native call would write — so its time per pass INCLUDES a device synchronisation the
               native call does not have; quote the two together with that)
  to tol       passes until <r,r> <= tol^2 <b,b> at tol = 1e-4, both sides
  reconstruct  allocate + splat + solve + extract, and the extraction alone
Asserted first, per row: the same sign of chi at every voxel farther than one voxel from the surface (not an end of an edge
that crosses zero), |chi - chi_torch|_inf / |chi|_inf <= 1e-5 and the splat's field within 1e-5 of the torch one's (both
figures recorded).
Native and torch alternate in one process; 3 warm-ups, the median of --reps (>= 10), torch.cuda.synchronize inside the timed
region.  Every row is reported, slower ones included.  By kernel: a `rocprofv3 --kernel-trace --stats` run of its own over
one row (a child process).  Bytes per voxel and pass are counted from the kernels' loads and stores in WORDS and set
against the 6.29 TB/s a float4 copy reaches on this device: the x-face halos are read at a stride of 8 floats (32 in the
system kernel), so the sectors actually fetched are more and the TB/s column understates the traffic.  Also recorded, not judged: evaluate_recon of mesh_poisson and of mesh_tsdf on
the synthetic graph of tools/tsdf_bench.py, and the capped unit sphere (19 000 samples less a 0.43 m cap) closed by the solve."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from splat_loam_amd import evaluation, mesh_ops, meshing, poisson, tsdf

COPY_TBPS = 6.29
# float32 words per voxel and pass: apply reads z, p_old, diag and 384 / 512 of a halo of z and of p_old, writes p and q; update
# reads x, p, r, q, diag, writes x, r, z
BYTES_PER_VOXEL_PASS = 4 * (3 + 1.5 + 2 + 5 + 3)
# The yardstick must agree with the code under test before a time of it means anything.  Both bars are float32 round-off, not
# what this code happens to give: the torch splat sums float32 products in float32 in any order where the native one sums in
# float64 — eps = 6e-8 times the square root of the few thousand terms a node of the densest row takes, rounded up to 1e-5;
# the two solves stop at the same residual after the same hundred-odd passes of float32 updates — eps times the number of
# passes, 1e-5 likewise.  Recorded on the rows of this tool: splat up to 1.1e-6, chi 5.0e-7 to 8.1e-7.
SPLAT_BAR = 1e-5
CHI_BAR = 1e-5


def room_cloud(M, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    size = torch.tensor([8.0, 6.0, 3.0], device=dev)
    area = torch.tensor([6.0 * 3.0, 8.0 * 3.0, 8.0 * 6.0], device=dev).repeat_interleave(2)
    face = torch.multinomial(area / area.sum(), M, replacement=True, generator=g)
    axis, side = face // 2, face % 2
    p = torch.rand((M, 3), device=dev, generator=g) * size
    n = torch.zeros((M, 3), device=dev)
    sign = 1.0 - 2.0 * side.float()                          # the low face looks up, the high face down: inwards
    n[torch.arange(M, device=dev), axis] = sign
    p[torch.arange(M, device=dev), axis] = side.float() * size[axis] + 0.005 * torch.randn((M,), device=dev, generator=g)
    return (p - size / 2 + torch.tensor([0.013, -0.027, 0.041], device=dev)).contiguous(), n


def sphere_cloud(dev, n=19000, cap=0.43):
    i = torch.arange(n, device=dev, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = torch.sqrt(1.0 - z * z)
    nrm = torch.stack([rho * torch.cos(phi), rho * torch.sin(phi), z], 1)
    keep = ~((nrm[:, 2] > 0) & (torch.hypot(nrm[:, 0], nrm[:, 1]) < cap))
    nrm = nrm[keep].float()
    return (nrm + torch.tensor([0.137, -0.219, 0.071], device=dev)).contiguous(), nrm.contiguous()


def timed(fn, reps, dev, warm=3):
    times = []
    for it in range(warm + reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize(dev)
        if it >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
        del res
    return float(np.median(times))


def alternate(fns, reps, dev, warm=3):
    acc = [[] for _ in fns]
    for it in range(warm + reps):
        for fn, a in zip(fns, acc):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize(dev)
            if it >= warm:
                a.append((time.perf_counter() - t0) * 1e3)
            del res
    return [float(np.median(a)) for a in acc]


# ---- the torch composition ---------------------------------------------------------------------------------------------
def block_keys(b):
    b = b.long() + (1 << 20)
    return b[..., 0] | (b[..., 1] << 21) | (b[..., 2] << 42)


def lookup(blocks, b):
    keys = block_keys(blocks)
    want = block_keys(b)
    pos = torch.searchsorted(keys, want).clamp_max(keys.numel() - 1)
    return torch.where(keys[pos] == want, pos, torch.full_like(pos, -1))


def torch_neighbour_slots(blocks):
    B, dev = blocks.shape[0], blocks.device
    l = torch.arange(512, device=dev)
    out = []
    for d in range(6):
        sh = 3 * (d >> 1)
        step = torch.zeros(3, dtype=torch.int32, device=dev)
        step[d >> 1] = 1 if d & 1 else -1
        nb = lookup(blocks, blocks + step)
        c = (l >> sh) & 7
        outside = (c == 7) if d & 1 else (c == 0)
        l2 = torch.where(outside, l - (7 << sh) if d & 1 else l + (7 << sh), l + (1 << sh) if d & 1 else l - (1 << sh))
        k2 = torch.where(outside[None], nb[:, None], torch.arange(B, device=dev)[:, None])
        out.append(torch.where(k2 >= 0, k2 * 512 + l2[None], torch.full_like(k2, -1)).reshape(-1))
    return out


def torch_splat(points, normals, blocks, h, origin):
    dev = points.device
    u = (points.double() - torch.tensor(origin, dtype=torch.float64, device=dev)) / h - 0.5
    i = torch.floor(u)
    f = (u - i).float()
    cell = i.long()
    field = torch.zeros((blocks.shape[0] * 512, 4), dtype=torch.float32, device=dev)
    have = lookup(blocks, cell >> 3) >= 0
    for c in range(8):
        d = torch.tensor([c & 1, (c >> 1) & 1, c >> 2], device=dev)
        node = cell + d
        k = lookup(blocks, node >> 3)
        ok = have & (k >= 0)
        slot = (k * 512 + ((node[:, 0] & 7) | (node[:, 1] & 7) << 3 | (node[:, 2] & 7) << 6))[ok]
        w3 = torch.where(d[None] == 1, f, 1.0 - f)
        w = (w3[:, 0] * w3[:, 1] * w3[:, 2])[ok]
        field.index_add_(0, slot, torch.cat([w[:, None] * normals[ok], w[:, None]], 1))
    return field.view(-1, 512, 4)


def torch_system(field, nbr, alpha):
    """(A as sparse CSR without its diagonal, diag, b): float32, the operator of include/sls_poisson_math.h"""
    F = field.reshape(-1, 4)
    n, dev = F.shape[0], F.device
    b = torch.zeros(n, device=dev)
    deg = torch.zeros(n, device=dev)
    rows, cols = [], []
    for d in range(6):
        has = nbr[d] >= 0
        g = 0.5 * (F[nbr[d].clamp_min(0), d >> 1] + F[:, d >> 1])
        b = torch.where(has, b - g if d & 1 else b + g, b)
        deg += has
        rows.append(torch.nonzero(has)[:, 0])
        cols.append(nbr[d][has])
    rows, cols = torch.cat(rows), torch.cat(cols)
    off = torch.sparse_coo_tensor(torch.stack([rows, cols]), -torch.ones(rows.numel(), device=dev), (n, n)).coalesce().to_sparse_csr()
    return off, deg + alpha * F[:, 3], b


def torch_pcg(off, diag, b, iterations, tol):
    x = torch.zeros_like(b)
    r = b.clone()
    z = r / diag
    p = z.clone()
    rz = torch.dot(r.double(), z.double())
    bb = torch.dot(b.double(), b.double())
    thr = tol * tol * bb
    it = 0
    for it in range(1, iterations + 1):
        q = diag * p + torch.sparse.mm(off, p[:, None])[:, 0]
        a = rz / torch.dot(p.double(), q.double())
        x = x + a.float() * p
        r = r - a.float() * q
        z = r / diag
        rr = torch.dot(r.double(), r.double())
        rz2 = torch.dot(r.double(), z.double())
        if bool(rr <= thr):                                  # the one host read per pass
            break
        p = z + (rz2 / rz).float() * p
        rz = rz2
    return x, it


def compare_chi(vol, chi_t, nbr):
    chi = vol.chi.reshape(-1)
    near = torch.zeros_like(chi, dtype=torch.bool)          # an end of an edge that crosses zero: within one voxel of the surface
    for d in range(6):
        has = nbr[d] >= 0
        near |= has & ((chi < 0) != (chi[nbr[d].clamp_min(0)] < 0))
    far = ~near
    wrong = int(((chi < 0) != (chi_t < 0))[far].sum())
    err = float((chi - chi_t).abs().max() / chi.abs().max())
    return {"voxels_beyond_one_voxel": int(far.sum()), "wrong_sign_beyond_one_voxel": wrong, "chi_rel_error_inf": err}


def bench_row(M, h, reps, dev):
    points, normals = room_cloud(M, dev)
    blocks = tsdf.allocate_blocks(points, h, 3 * h)
    B = int(blocks.shape[0])
    vol = poisson.PoissonVolume(blocks, h)
    origin = (0.0, 0.0, 0.0)
    nbr = torch_neighbour_slots(blocks)
    t_splat, t_splat_torch = alternate([lambda: vol.splat(points, normals), lambda: torch_splat(points, normals, blocks, h, origin)], reps, dev)
    field_t = torch_splat(points, normals, blocks, h, origin)
    vol.splat(points, normals)
    splat_err = float((vol.field - field_t).abs().max() / vol.field.abs().max())
    assert splat_err <= SPLAT_BAR, splat_err
    off, diag, b = torch_system(vol.field, nbr, 4.0)
    info = vol.solve(4.0, 300, 1e-4)
    x_t, it_t = torch_pcg(off, diag, b, 300, 1e-4)
    W = vol.field[..., 3].reshape(-1)
    chi_t = x_t - (W.double() @ x_t.double() / W.double().sum()).float()
    check = compare_chi(vol, chi_t, nbr)
    assert check["wrong_sign_beyond_one_voxel"] == 0, check
    assert check["chi_rel_error_inf"] <= CHI_BAR, check
    t10, t60 = alternate([lambda: vol.solve(4.0, 10, 0.0), lambda: vol.solve(4.0, 60, 0.0)], reps, dev)
    t_tol, t_tol_torch = alternate([lambda: vol.solve(4.0, 300, 1e-4), lambda: torch_pcg(off, diag, b, 300, 1e-4)], reps, dev)
    t10_t, t60_t = alternate([lambda: torch_pcg(off, diag, b, 10, 0.0), lambda: torch_pcg(off, diag, b, 60, 0.0)], max(reps // 2, 5), dev)
    vol.solve(4.0, 300, 1e-4)
    t_extract = timed(lambda: vol.extract(), reps, dev)
    t_density = timed(lambda: vol.density(2), reps, dev)
    t_all = timed(lambda: poisson.reconstruct(points, normals, h), reps, dev)
    per_pass = (t60 - t10) / 50
    return {"samples": M, "voxel_size": h, "blocks": B, "voxels": 512 * B, "triangles": int(vol.extract()[1].shape[0]),
            "splat_ms": t_splat, "splat_torch_index_add_ms": t_splat_torch, "splat_rel_error_inf": splat_err,
            "pass_us": 1e3 * per_pass, "pass_torch_sparse_us": 1e3 * (t60_t - t10_t) / 50,
            "passes_to_tol": info["iterations"], "passes_to_tol_torch": it_t, "residual": info["residual"],
            "solve_to_tol_ms": t_tol, "solve_to_tol_torch_ms": t_tol_torch, "density_2_sweeps_ms": t_density, "extract_ms": t_extract,
            "reconstruct_ms": t_all, "bytes_per_voxel_pass": BYTES_PER_VOXEL_PASS,
            "achieved_TBps": BYTES_PER_VOXEL_PASS * 512 * B / (per_pass * 1e-3) / 1e12, "float4_copy_TBps": COPY_TBPS, **check}


def by_kernel(dev):
    """A child under rocprofv3 --kernel-trace --stats: the kernels of one reconstruct at 500 k samples, 0.1 m."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "-d", d, "-o", "poisson", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--profile-child"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not files:
            return {"skipped": f"rocprofv3 run gave code {run.returncode} and {len(files)} stats files", "stderr": run.stderr[-400:]}
        rows = []
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if "poisson" in name or "sort_" in name or "tsdf_" in name:
                    rows.append({"kernel": name.split("(")[0][-60:], "calls": int(row.get("Calls", 0)),
                                 "total_us": float(row.get("TotalDurationNs", 0)) / 1e3, "average_us": float(row.get("AverageNs", 0)) / 1e3,
                                 "percent": float(row.get("Percentage", 0))})
        return {"row": "500 k samples, 0.1 m voxels, one reconstruct after one warm-up (both traced)", "kernels": rows}


def profile_child():
    dev = torch.device("cuda:0")
    points, normals = room_cloud(500_000, dev)
    for _ in range(2):
        poisson.reconstruct(points, normals, 0.1)
    torch.cuda.synchronize(dev)


def recon_comparison(dev):
    from sample_surface import write_synthetic_results
    out = {}
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        write_synthetic_results(d, 8, 64, 1024, 50000)
        ref_pts, _ = meshing.sample_surface(d, seed=1, device=dev)
        for name, fn in (("mesh_tsdf", lambda: meshing.mesh_tsdf(d, 0.25, seed=1, device=dev, keep_clusters=1)),
                         ("mesh_poisson", lambda: meshing.mesh_poisson(d, 0.25, seed=1, device=dev, keep_clusters=1)),
                         ("mesh_poisson_q05", lambda: meshing.mesh_poisson(d, 0.25, seed=1, device=dev, keep_clusters=1, min_density_quantile=0.05))):
            v, f = fn()[:2]
            m = evaluation.evaluate_recon(ref_pts, v, f, down_sample_res=0.02, mesh_sample_point=200000, seed=1)
            edges = mesh_ops.cluster_triangles(f, v.shape[0], details=True)[2]
            out[name] = {"triangles": int(f.shape[0]), "F-score (%)": float(m["F-score (%)"]), "Recall [Completeness] (%)": float(m["Recall [Completeness] (%)"]),
                         "MAE_completeness (cm)": float(m["MAE_completeness (cm)"]), "MAE_accuracy (cm)": float(m["MAE_accuracy (cm)"]),
                         "boundary_edges": edges["boundary_edges"]}
    return out


def sphere_numbers(dev):
    points, normals = sphere_cloud(dev)
    v, f, det = poisson.reconstruct(points, normals, 0.1, origin=(0.05, -0.02, 0.11), weld=True, details=True)
    edges = mesh_ops.cluster_triangles(f, v.shape[0], details=True)[2]
    r = (v - torch.tensor([0.137, -0.219, 0.071], device=dev)).norm(dim=1)
    return {"samples": int(points.shape[0]), "blocks": det["blocks"], "passes": det["solve"]["iterations"], "triangles": int(f.shape[0]),
            "boundary_edges": edges["boundary_edges"], "clusters": edges["clusters"], "euler": int(v.shape[0]) - (3 * int(f.shape[0])) // 2 + int(f.shape[0]),
            "mean_radius_error_mm": 1e3 * float((r - 1).abs().mean()), "max_radius_error_mm": 1e3 * float((r - 1).abs().max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31a_poisson.json"))
    ap.add_argument("--quick", action="store_true", help="the 50 k rows only")
    ap.add_argument("--no-profile", action="store_true", help="leave out the rocprofv3 child")
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("poisson_bench needs a GPU: a time taken elsewhere says nothing")
    if a.profile_child:
        return profile_child()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    dev = torch.device("cuda:0")
    res = {"what": "poisson.PoissonVolume (sls_poisson_splat / _solve / _density) and poisson.reconstruct against a torch composition "
                   "(index_add_ splat, sparse-CSR PCG)", "data": "synthetic room, 8 x 6 x 3 m, 5 mm noise", "screening": 4.0, "margin_voxels": 3,
           "protocol": f"one process, alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed region",
           "device": torch.cuda.get_device_name(0), "rows": []}
    with torch.no_grad():
        for M in ((50_000,) if a.quick else (50_000, 500_000, 2_000_000)):
            for h in (0.1, 0.05):
                row = bench_row(M, h, a.reps, dev)
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
        res["capped_sphere"] = sphere_numbers(dev)
        res["evaluate_recon"] = recon_comparison(dev)
    res["by_kernel"] = {"skipped": "--no-profile"} if a.no_profile else by_kernel(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))


if __name__ == "__main__":
    main()
