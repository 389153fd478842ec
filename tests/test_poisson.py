"""The Poisson volume on the GPU (sls_poisson_splat, sls_poisson_solve, sls_poisson_density, splat_loam_amd/poisson.py,
meshing.mesh_poisson) against include/sls_poisson_math.h run on the host (poisson_ref.host()), bit for bit: the field and its
status words, chi and the solve's status words, the density, the triangle soup in order.  The closedness and radius checks of
tests/test_poisson_math.py run on the device output as well; a keyframe of a synthetic room goes through the real rasterizer
forward, the sampler, the solve and the mesh cleaning end to end."""
import functools

import numpy as np
import pytest
import torch

import poisson_ref as ref
import tsdf_ref
from helpers import write_room as _write_room
from splat_loam_amd import _abi, evaluation, mesh_ops, meshing, ply_io, poisson
from poisson_ref import ORIGIN, VS, bits, same_bits

pytestmark = pytest.mark.gpu


def _dev(a, device, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(device)         # (a copy: the shared inputs are read-only)


def _run(device, pts, nrm, blocks, h, origin, alpha=4.0, iterations=300, tol=1e-4, sweeps=2):
    """dict(field, splat, chi, status, density) as NumPy arrays, from the device"""
    vol = poisson.PoissonVolume(_dev(blocks, device, np.int32).view(-1, 3), h, origin)
    det = vol.splat(_dev(pts, device, np.float32).view(-1, 3), _dev(nrm, device, np.float32).view(-1, 3), details=True)
    info = vol.solve(alpha, iterations, tol)
    words = vol.status.cpu().numpy().view(np.uint64)
    assert info["iterations"] == int(words[0]) and info["flags"] == int(words[1]) and info["converged"] == bool(words[1] & 1)
    return {"field": vol.field.cpu().numpy(), "splat": [det["n_nonfinite"], det["n_out_of_range"], det["n_dropped"]],
            "chi": vol.chi.cpu().numpy(), "status": words, "density": vol.density(sweeps).cpu().numpy(), "volume": vol, "info": info}


def _host(pts, nrm, blocks, h, origin, alpha=4.0, iterations=300, tol=1e-4, sweeps=2):
    host = ref.host()
    field, st = host.splat(pts, nrm, blocks, h, origin)
    out = host.solve(blocks, field, alpha, iterations, tol)
    return {"field": field, "splat": st[:3].tolist(), "chi": out["chi"], "status": out["status"], "density": host.density(blocks, field, sweeps)}


def _compare(got, want, what):
    same_bits(got["field"], want["field"], f"{what}: field")
    assert got["splat"] == want["splat"], (what, got["splat"], want["splat"])
    assert got["status"].tolist() == want["status"].tolist(), (what, ref.status_dict(got["status"]), ref.status_dict(want["status"]))
    same_bits(got["chi"], want["chi"], f"{what}: chi")
    same_bits(got["density"], want["density"], f"{what}: density")


def _cloud_in(blocks, h, origin, M, seed, spread=(0.2, 7.8)):
    """M points inside randomly chosen blocks, normals roughly along +z: a field with a non-zero divergence"""
    rng = np.random.default_rng(seed)
    blocks = np.asarray(blocks)
    k = rng.integers(0, len(blocks), M)
    pts = (np.asarray(origin) + (8 * blocks[k] + rng.uniform(spread[0], spread[1], (M, 3))) * h).astype(np.float32)
    nrm = rng.normal(size=(M, 3)) * 0.3 + [0, 0, 1]
    return pts, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)


# ---- 1. one block: every halo absent; one point; no point -----------------------------------------------------------------
@pytest.mark.parametrize("M", [700, 1])
def test_one_block(device, M):
    blocks = ref.sort_blocks([[2, -3, 1]])
    pts, nrm = _cloud_in(blocks, 0.125, ORIGIN, M, seed=M, spread=(-0.2, 8.2))
    got, want = _run(device, pts, nrm, blocks, 0.125, ORIGIN, tol=1e-5), _host(pts, nrm, blocks, 0.125, ORIGIN, tol=1e-5)
    _compare(got, want, f"one block, {M} points")
    assert got["status"][2] == 1 and (M == 1 or (got["info"]["converged"] and got["splat"][2] > 0))


def test_no_point_touches_nothing_but_the_status(device):
    lib = _abi.lib()
    field = torch.full((1, 512, 4), 7.0, device=device)
    status = torch.full((4,), -1, dtype=torch.int32, device=device)
    blocks = torch.zeros((1, 3), dtype=torch.int32, device=device)
    origin = np.zeros(3)
    _abi.check(lib.sls_poisson_splat(0, None, None, 1, blocks.data_ptr(), 0.1, origin.ctypes.data, field.data_ptr(), status.data_ptr(), None, 0,
                                     torch.cuda.current_stream(device).cuda_stream), "sls_poisson_splat")
    assert status.tolist() == [0, 0, 0, 1] and bool((field == 7.0).all())
    # ... and through the class: a zero field, CONVERGED | EMPTY, chi = 0, no surface; a volume without blocks likewise
    for B in (1, 0):
        vol = poisson.PoissonVolume(blocks[:B], 0.1)
        assert vol.splat(torch.zeros((0, 3), device=device), torch.zeros((0, 3), device=device), details=True)["n_dropped"] == 0
        info = vol.solve()
        assert info["iterations"] == 0 and info["flags"] == ref.FLAG_CONVERGED | ref.FLAG_EMPTY and info["iso"] == 0.0
        assert vol.status.cpu().numpy().view(np.uint64)[:3].tolist() == [0, ref.FLAG_CONVERGED | ref.FLAG_EMPTY, B]
        assert not bool(vol.chi.any()) and vol.extract()[1].shape[0] == 0 and vol.density().shape == (B, 512)


# ---- 2. 2 x 2 x 2 blocks around the origin, one missing ----------------------------------------------------------------------
def test_eight_blocks_less_one(device):
    blocks = ref.sort_blocks([[x, y, z] for z in (-1, 0) for y in (-1, 0) for x in (-1, 0) if (x, y, z) != (0, -1, 0)])
    assert len(blocks) == 7
    nb = ref.host().neighbours(blocks)
    assert all(((nb[:, d] >= 0).any() and (nb[:, d] < 0).any()) for d in range(6))      # present and absent faces in all six directions
    pts, nrm = _cloud_in(blocks, VS, ORIGIN, 3000, seed=2, spread=(-0.4, 8.4))
    got, want = _run(device, pts, nrm, blocks, VS, ORIGIN, alpha=1.0), _host(pts, nrm, blocks, VS, ORIGIN, alpha=1.0)
    _compare(got, want, "seven blocks")
    assert got["info"]["converged"] and got["info"]["iterations"] > 10


# ---- 3. a row with a gap; block faces; bad points; a crowded voxel --------------------------------------------------------
def test_row_with_a_gap(device):
    blocks = ref.sort_blocks([[0, 0, 0], [1, 0, 0], [3, 0, 0]])
    h, o = VS, np.asarray(ORIGIN)
    rng = np.random.default_rng(3)
    pts, nrm = _cloud_in(blocks, h, ORIGIN, 1500, seed=3)
    face = o + (np.array([[7.6, 3.3, 4.4], [8.4, 3.3, 4.4], [8.6, 2.2, 1.1], [15.7, 5, 5], [16.2, 5, 5], [23.9, 1, 1], [24.3, 1, 1]])) * h
    crowd = o + (np.array([11.0, 4.0, 2.0]) + rng.uniform(0.5, 1.5, (5000, 3))) * h
    bad = np.array([[np.nan, 0, 0], [0.3, np.inf, 0.1], [9.0, 9.0, 9.0], [-5.0, 0.2, 0.2], [3.0e9, 0, 0]])
    pts = np.concatenate([pts, face, crowd, bad]).astype(np.float32)
    extra = len(pts) - len(nrm)
    nrm = np.concatenate([nrm, np.tile(np.float32([0.6, 0, 0.8]), (extra, 1))]).astype(np.float32)
    nrm[100] = [np.nan, 0, 1]                                   # a normal that is not finite counts as a point that is not
    got, want = _run(device, pts, nrm, blocks, h, ORIGIN), _host(pts, nrm, blocks, h, ORIGIN)
    _compare(got, want, "row with a gap")
    assert got["splat"][0] == 3 and got["splat"][1] == 1 and got["splat"][2] >= 4
    restated, rs = ref.splat(pts, nrm, blocks, h, ORIGIN)
    same_bits(got["field"], restated, "the NumPy restatement's field")
    assert rs[:3].tolist() == got["splat"]
    assert got["field"][..., 3].max() > 500.0                   # the crowded voxel's eight nodes


# ---- 4. past one round of the final reduction -------------------------------------------------------------------------------
def test_slab_of_1089_blocks(device):
    blocks = ref.sort_blocks([[x, y, 0] for x in range(33) for y in range(33)])
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(0.0, 26.4, (20000, 2)), 0.41 + 0.01 * rng.normal(size=(20000, 1))], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (20000, 1))
    got = _run(device, pts, nrm, blocks, 0.1, (0.0, 0.0, 0.0), iterations=12)
    want = _host(pts, nrm, blocks, 0.1, (0.0, 0.0, 0.0), iterations=12)
    _compare(got, want, "slab")
    assert got["status"][:3].tolist() == [12, 0, 1089]


# ---- 5. the freeze --------------------------------------------------------------------------------------------------------
def test_the_remaining_passes_change_nothing(device):
    blocks = ref.sort_blocks([[x, y, z] for z in (-1, 0) for y in (-1, 0) for x in (-1, 0) if (x, y, z) != (0, -1, 0)])
    pts, nrm = _cloud_in(blocks, VS, ORIGIN, 3000, seed=2, spread=(-0.4, 8.4))
    full = _run(device, pts, nrm, blocks, VS, ORIGIN)
    k = int(full["status"][0])
    assert 5 < k < 300 and full["status"][1] == ref.FLAG_CONVERGED
    exact = _run(device, pts, nrm, blocks, VS, ORIGIN, iterations=k)
    _compare(exact, full, "iterations = k against iterations = 300")
    short = _run(device, pts, nrm, blocks, VS, ORIGIN, iterations=k - 1)
    assert short["status"][:2].tolist() == [k - 1, 0] and not np.array_equal(bits(short["chi"]), bits(full["chi"]))
    _compare(short, _host(pts, nrm, blocks, VS, ORIGIN, iterations=k - 1), "iterations = k - 1")


# ---- 6. the capped sphere ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_sphere():
    pts, nrm = ref.capped_sphere()
    blocks = ref.blocks_around(pts)
    out = _host(pts, nrm, blocks, VS, ORIGIN)
    out["blocks"] = blocks
    return out


def test_capped_sphere(device):
    pts, nrm = ref.capped_sphere()
    want = _host_sphere()
    vertices, faces, det = poisson.reconstruct(_dev(pts, device), _dev(nrm, device), VS, origin=ORIGIN, details=True)
    vol = det["volume"]
    assert np.array_equal(vol.blocks.cpu().numpy(), want["blocks"]) and det["splat"]["n_dropped"] == 0
    same_bits(vol.chi.cpu().numpy(), want["chi"], "chi")
    soup, _ = tsdf_ref.host().extract(want["blocks"], want["chi"], np.ones_like(want["chi"]), VS, ORIGIN, 1.0)
    same_bits(vertices.cpu().numpy().reshape(-1, 3, 3), soup, "the soup")
    v2, f2 = vol.extract()
    assert torch.equal(v2, vertices) and torch.equal(f2, faces)
    wv, wf = vol.extract(weld=True)
    _, _, edges = mesh_ops.cluster_triangles(wf, wv.shape[0], details=True)
    rep = ref.sphere_report(soup)
    print(f"{det['blocks']} blocks, {det['solve']}, {edges}, {rep}")
    assert edges["boundary_edges"] == 0 and edges["nonmanifold_edges"] == 0 and edges["clusters"] == 1
    assert rep["closed"] and rep["euler"] == 2 and rep["outward"] and rep["cap_vertices"] > 50 and rep["cap_error"] <= VS
    assert det["solve"]["converged"] and det["solve"]["residual"] <= 1e-4


# ---- 7. the noisy plane with a hole, trimmed by density ----------------------------------------------------------------------
def test_holed_plane_trimmed(device):
    sweeps, thr = 3, 1e-2           # three sweeps reach four voxels: the middle of the hole, three voxels from every sample
    pts, nrm = ref.holed_plane()
    blocks = ref.blocks_around(pts)
    want = _host(pts, nrm, blocks, VS, ORIGIN, sweeps=sweeps)
    vertices, faces, det = poisson.reconstruct(_dev(pts, device), _dev(nrm, device), VS, origin=ORIGIN, min_density=thr,
                                               density_sweeps=sweeps, details=True)
    same_bits(det["volume"].chi.cpu().numpy(), want["chi"], "chi")
    same_bits(det["density"].cpu().numpy(), want["density"], "density")
    soup, _ = tsdf_ref.host().extract(blocks, want["chi"], want["density"], VS, ORIGIN, thr)
    same_bits(vertices.cpu().numpy().reshape(-1, 3, 3), soup, "the trimmed soup")
    untrimmed = det["volume"].extract()[1].shape[0]
    v = soup.reshape(-1, 3).astype(np.float64)
    reach = (sweeps + 1) * VS
    print(f"{len(blocks)} blocks, {det['solve']}: {len(soup)} of {untrimmed} triangles kept; farthest |x|, |y| {np.abs(v[:, :2]).max():.3f}")
    assert len(soup) < untrimmed
    assert np.abs(v[:, :2]).max() <= 3.0 + reach                # nothing beyond the rim by more than the smoothing reach
    col = np.rint((v[:, :2] - np.asarray(ORIGIN[:2])) / VS - 0.5).astype(int)
    have = set(map(tuple, col.tolist()))
    g = np.arange(-40, 40)
    cx, cy = ORIGIN[0] + (g + 0.5) * VS, ORIGIN[1] + (g + 0.5) * VS
    need = [(int(a), int(b)) for a, x in zip(g, cx) for b, y in zip(g, cy) if abs(x) <= 3.0 and abs(y) <= 3.0]
    assert len(need) == 3600 and all(c in have for c in need)   # every column whose centre lies on the patch, rim and hole included
    assert np.abs(v[np.abs(v[:, :2]).max(1) <= 3.0, 2] - 0.033).max() <= VS      # ... and there the surface is within a voxel of the plane


# ---- 8. two runs ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(device):
    pts, nrm = ref.capped_sphere()
    blocks = _host_sphere()["blocks"]
    a, b = _run(device, pts, nrm, blocks, VS, ORIGIN), _run(device, pts, nrm, blocks, VS, ORIGIN)
    _compare(a, b, "second run")
    _compare(a, _host_sphere(), "against the host")


# ---- 9. a results directory to a mesh ------------------------------------------------------------------------------------------
K2, VS2, SEED = 4000, 0.1, 0x5EED


def test_mesh_poisson_end_to_end(device, tmp_path):
    _write_room(tmp_path)
    vertices, faces, det = meshing.mesh_poisson(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True)
    print(f"{det['blocks']} blocks, {det['samples']} samples, {det['triangles']} triangles, {det['solve']}, stages {det['stage_ms']}")
    assert faces.shape[0] == det["triangles"] > 1000 and vertices.shape == (3 * faces.shape[0], 3) and det["solve"]["iterations"] > 0
    # the pieces composed by hand, bit for bit
    pts, nrm = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    v2, f2 = poisson.reconstruct(pts, nrm, VS2)
    assert torch.equal(v2, vertices) and torch.equal(f2, faces)
    # cleaned: the largest cluster with normals; trimmed by a density quantile: fewer triangles
    cv, cf, cn, cdet = meshing.mesh_poisson(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, keep_clusters=1, normals=True,
                                            min_density_quantile=0.05, details=True)
    assert cn.shape == cv.shape and cf.shape[0] > 1000 and cdet["min_density"] > 0 and cdet["triangles"] <= det["triangles"]
    assert bool(torch.isfinite(cn).all()) and float((cn.norm(dim=1) - 1).abs().max()) <= 1e-4
    # the surface lies where the room is: the mesh against the sampled cloud
    metrics = evaluation.evaluate_recon(pts, cv, cf, down_sample_res=0.02, mesh_sample_point=20000, seed=1)
    print("    evaluate_recon:", {k: round(float(v), 4) for k, v in metrics.items() if isinstance(v, (int, float))})
    assert all(np.isfinite(float(v)) for v in metrics.values() if isinstance(v, (int, float)))
    ply_io.save_mesh(tmp_path / "mesh.ply", cv, cf, normals=cn)
    lv, lf = ply_io.load_mesh(tmp_path / "mesh.ply")
    assert np.array_equal(bits(lv), bits(cv.cpu().numpy())) and np.array_equal(lf, cf.cpu().numpy())
