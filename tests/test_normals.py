"""sls_cloud_normals and its Python faces (splat_loam_amd/evaluation.py: estimate_normals, projector.py:
DeviceProjector(normals="pca"), tools/cloud_normals.py) on the device against the NumPy restatement (normals_ref.py).

Lattice inputs (multiples of 1/16, differences of magnitude <= 128) make the kernel's float32 squared distance exact, so the
restatement's brute-force lists are the kernel's, bit for bit; from equal lists the header's arithmetic — float64, a fixed
order, + - * / and sqrt only, no contraction — gives equal bits on the device, on the host and in Python.  So normals (as
float32 words), counts and eigenvalues compare with array_equal, and so do the neighbour rows the call leaves in its scratch,
which is how the search's two passes beyond k = 32 are checked directly."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import normals_ref as ref
from splat_loam_amd import evaluation, ply_io, projector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 4, 5, 20, 32, 33, 50, 64)


def lattice(rng, n, half=64.0, step=16):
    return (rng.integers(-int(half * step), int(half * step) + 1, (n, 3)) / float(step)).astype(np.float32)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(device, pts, k, radius, view, lists=True):
    out = evaluation._estimate_normals(torch.tensor(pts, device=device), radius, k, view, True, lists)
    return [t.cpu().numpy() for t in out]


def check(device, pts, full, k, radius, view, what):
    """One call against the restatement, everything bit for bit; returns the restatement's result."""
    want = ref.normals(pts, k, radius, view, full=full)
    nrm, cnt, eig, d2, idx = run(device, pts, k, radius, view)
    assert nrm.dtype == eig.dtype == np.float32 and cnt.dtype == np.int32 and nrm.shape == eig.shape == (len(pts), 3)
    assert np.array_equal(words(d2), words(full[0][:, :k])) and np.array_equal(idx, full[1][:, :k]), f"{what}: neighbour rows"
    bad = np.flatnonzero(cnt != want["count"])
    assert bad.size == 0, f"{what}: {bad.size} counts differ, first {bad[:3]}: {cnt[bad[:3]]} {want['count'][bad[:3]]}"
    for name, got, exp in (("normals", nrm, want["normals"]), ("eigenvalues", eig, want["eigenvalues"])):
        bad = np.flatnonzero((words(got) != words(exp)).any(1))
        assert bad.size == 0, f"{what}: {name} differ in {bad.size} of {len(pts)} rows, first {bad[:3]}: got {got[bad[:3]]}, " \
                              f"want {exp[bad[:3]]}, count {cnt[bad[:3]]}"
    return want


@functools.lru_cache(maxsize=None)
def lattice_case(M):
    """M lattice points in the cube |x| <= 4 (a few per unit volume at the larger M), row 5 a copy of row 9, their 64-lists,
    and two radii taken from the lists: one that cuts most lists at about five entries, one that leaves about half of the points
    fewer than three (where the cloud has that many)."""
    pts = lattice(np.random.default_rng(1000 + M), M, half=4.0)
    if M > 9:
        pts[5] = pts[9]
    full = ref.lists(pts, 64)
    rank = lambda j: float(np.sqrt(np.median(full[0][:, j]))) if M > j else 1.0
    return pts, full, (rank(5), rank(2))


# the list shorter than k, the three-point threshold, a partial last wave, one box plus one point, several boxes
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 257, 1500, 3000])
def test_lattice_clouds_bit_for_bit(device, M):
    pts, full, (r_cut, r_few) = lattice_case(M)
    view = (0.5, -3.0, 20.0)
    for k in KS:
        for radius in (r_cut, r_few, None):
            want = check(device, pts, full, k, radius, view, f"M={M} k={k} radius={radius}")
            n = want["count"]
            if radius is None:
                assert np.all(n == min(k, M))
            elif M >= 63 and k >= 20:
                if radius == r_cut:
                    assert (n < min(k, M)).mean() > 0.5 and (n >= 3).mean() > 0.5       # most lists cut short, most still solved
                else:
                    assert 0.1 < (n < 3).mean() < 0.9                                   # some fall back, some do not
            if k == 50 and radius == r_cut:                                             # two runs: equal bits
                again = run(device, pts, k, radius, view)
                first = run(device, pts, k, radius, view)
                assert all(np.array_equal(words(a), words(b)) for a, b in zip(again, first))
    if M >= 3:
        few = ref.normals(pts, 20, r_few, view, full=full)["count"] < 3
        nrm = run(device, pts, 20, r_few, view, lists=False)[0]
        assert np.array_equal(words(nrm[few]), words(ref.fallback(pts[few], view)))


def test_plain_call_and_details(device):
    """The public call: normals alone, or (normals, count, eigenvalues); radius=None counts min(k, M); defaults 0.5 / 30 / origin."""
    pts, full, _ = lattice_case(1500)
    p = torch.tensor(pts, device=device)
    nrm = evaluation.estimate_normals(p)
    assert isinstance(nrm, torch.Tensor) and nrm.shape == (1500, 3) and nrm.dtype == torch.float32
    got = evaluation.estimate_normals(p, return_details=True)
    assert len(got) == 3 and torch.equal(got[0].view(torch.int32), nrm.view(torch.int32))
    want = ref.normals(pts, 30, 0.5, (0, 0, 0), full=full)
    assert np.array_equal(words(nrm.cpu().numpy()), words(want["normals"])) and np.array_equal(got[1].cpu().numpy(), want["count"])
    for k in (1, 20, 50, 64):
        assert torch.all(evaluation.estimate_normals(p, None, k, return_details=True)[1] == k)
        assert torch.all(evaluation.estimate_normals(p[:40], None, k, return_details=True)[1] == min(k, 40))
    empty = evaluation.estimate_normals(p[:0], return_details=True)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].shape == (0, 3)
    unit = np.linalg.norm(nrm.cpu().numpy().astype(np.float64), axis=1)
    assert np.all(np.abs(unit - 1) < 1e-6)
    for bad in (dict(max_nn=0), dict(max_nn=65), dict(radius=0.0), dict(radius=float("nan")), dict(viewpoint=(0, 0))):
        with pytest.raises(ValueError):
            evaluation.estimate_normals(p, **bad)
    with pytest.raises(ValueError):
        evaluation.nearest_k(p, p, 33)                                      # the longer list is estimate_normals' alone


def eigh_normals(want):
    """(n_eigh (m,3), clear (m,), rows) for the points with n >= 3: LAPACK on the restatement's float64 covariance."""
    rows = np.flatnonzero(want["count"] >= 3)
    c = want["cov"][rows]
    w, V = np.linalg.eigh(np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1))
    return V[:, :, 0], (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2], rows


def test_plane_patch_and_sphere(device):
    """A tilted plane that lies ON the lattice (z = x / 4 + y / 2 with x on the 1/4 grid and y on the 1/8 grid) and a radius-32
    sphere snapped to it.  The device equals the restatement bit for bit; the restatement is within 1e-6 of LAPACK's
    eigenvector wherever (l1 - l0) >= 1e-3 * l2 (tests/test_normals_math.py derives the bound), which may exclude 5 % at
    most; on the plane that is the analytic normal; the orientation follows the viewpoint."""
    rng = np.random.default_rng(21)
    xy = np.unique(np.stack([rng.integers(-32, 33, 2500) / 4.0, rng.integers(-64, 65, 2500) / 8.0], 1), axis=0)
    plane = np.concatenate([xy, (xy[:, 0] / 4 + xy[:, 1] / 2)[:, None]], 1).astype(np.float32)
    analytic = np.array([-0.25, -0.5, 1.0]) / np.sqrt(0.0625 + 0.25 + 1.0)
    full = ref.lists(plane, 64)
    inner = (np.abs(plane[:, 0]) < 6) & (np.abs(plane[:, 1]) < 6)           # away from the patch's rim
    for view, sign in (((0.0, 0.0, 50.0), 1.0), ((0.0, 0.0, -50.0), -1.0)):
        for k, radius in ((20, None), (50, 2.0)):
            want = check(device, plane, full, k, radius, view, f"plane k={k} view={view}")
            assert np.all(want["count"][inner] >= 3)
            cross = np.linalg.norm(np.cross(want["normals"][inner].astype(np.float64), sign * analytic), axis=1)
            dots = want["normals"][inner].astype(np.float64) @ (sign * analytic)
            print(f"plane k={k} radius={radius} view z={view[2]}: max |n x n_analytic| {cross.max():.3g}")
            assert cross.max() <= 1e-6 and np.all(dots > 0)
    v = rng.normal(0, 1, (3000, 3))
    sphere = np.unique((np.round(v / np.linalg.norm(v, axis=1, keepdims=True) * 32 * 16) / 16).astype(np.float32), axis=0)
    radial = sphere.astype(np.float64) / np.linalg.norm(sphere.astype(np.float64), axis=1, keepdims=True)
    full = ref.lists(sphere, 64)
    for view, inside in (((0.0, 0.0, 0.0), True), ((1000.0, 0.0, 0.0), False)):
        for k in (20, 50):
            want = check(device, sphere, full, k, None, view, f"sphere k={k} view={view}")
            n_eigh, clear, rows = eigh_normals(want)
            n = want["normals"][rows].astype(np.float64)
            cross = np.linalg.norm(np.cross(n, n_eigh), axis=1)
            print(f"sphere k={k} view={view}: max |n x n_eigh| {cross[clear].max():.3g}, excluded {1 - clear.mean():.4f}")
            assert 1 - clear.mean() <= 0.05 and cross[clear].max() <= 1e-6
            to_view = np.asarray(view)[None, :] - sphere.astype(np.float64)
            assert np.all((n * to_view[rows]).sum(1) >= 0)                    # towards the viewpoint, every one
            # a coarse analytic check: the k nearest of a point cover a cap a few units wide on a sphere of radius 32,
            # whose tangent plane is the radial direction's; sampling irregularity tilts it by far less than 25 degrees
            along = (n * radial[rows]).sum(1)
            assert np.all(np.abs(along) > 0.9)
            if inside:
                assert np.all(along < 0)                                      # seen from the centre: inward


def test_massive_duplicates_and_ties(device):
    """3000 points on the 33^3 lattice |x| <= 1 (the case of test_outlier.py): duplicates and equal distances everywhere,
    across boxes; lists full of copies give rank-deficient covariances."""
    pts = lattice(np.random.default_rng(33), 3000, half=1.0)
    full = ref.lists(pts, 64)
    assert (full[0][:, 1] == 0).mean() > 0.03 and (full[0][:, 20] == full[0][:, 21]).mean() > 0.5
    for k, radius in ((5, None), (20, 0.125), (33, None), (64, 0.25), (64, None)):
        check(device, pts, full, k, radius, (0.0, 0.0, 0.0), f"33^3 lattice k={k} radius={radius}")
    same = np.tile(np.array([[2.5, -1.0, 0.25]], np.float32), (100, 1))
    want = check(device, same, ref.lists(same, 64), 64, 0.5, (9.0, 0.0, 0.0), "identical points")
    assert np.all(want["normals"] == (1, 0, 0)) and np.all(want["count"] == 64) and np.all(want["eigenvalues"] == 0)


# ---- the projector's option ---------------------------------------------------------------------------------------------
def room_scan(H=16, n_az=256, seed=3):
    """A scan of a box room from the origin, snapped to the 1/16 lattice (a wall stays a plane): H x n_az returns, ranges
    from 4 m to the corners' 6.8 m."""
    rng = np.random.default_rng(seed)
    el = np.radians(np.linspace(20.0, -20.0, H))[:, None] + rng.uniform(-0.004, 0.004, (H, n_az))
    az = np.linspace(-np.pi, np.pi, n_az, endpoint=False)[None, :] + rng.uniform(-0.004, 0.004, (H, n_az))
    ray = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1).reshape(-1, 3)
    half = np.array([5.0, 4.0, 2.5])
    t = (half / np.abs(ray)).min(1, keepdims=True)
    pts = np.round(ray * t * 16) / 16
    return pts[rng.permutation(len(pts))].astype(np.float32)


def test_device_projector_pca(device):
    H, W, lo, hi = 16, 128, 4.5, 6.0
    cloud = room_scan()
    rng32 = np.sqrt(cloud[:, 0] * cloud[:, 0] + cloud[:, 1] * cloud[:, 1] + cloud[:, 2] * cloud[:, 2])     # float32, the kernel's
    inside = (rng32 > np.float32(lo)) & (rng32 <= np.float32(hi))
    assert len(cloud) == 4096 and 0.05 < (~inside).mean() < 0.6 and (rng32 <= lo).any() and (rng32 > hi).any()
    cd = torch.tensor(cloud, device=device)
    radial = projector.DeviceProjector(H, W, lo, hi, device=device).scan_to_images(cd)
    explicit = projector.DeviceProjector(H, W, lo, hi, device=device, normals="radial").scan_to_images(cd)
    rows = np.flatnonzero(inside)
    for radius, k in ((0.5, 50), (0.15, 20)):
        got = projector.DeviceProjector(H, W, lo, hi, device=device, normals="pca", normal_radius=radius,
                                        normal_max_nn=k).scan_to_images(cd)
        for key in ("lut", "range_image", "valid", "K"):
            assert torch.equal(got[key], radial[key]), key                  # bit for bit
        lut = got["lut"].cpu().numpy()
        valid = lut >= 0
        assert np.array_equal(got["valid"].cpu().numpy(), valid) and 0.5 < valid.mean() < 1.0
        assert inside[lut[valid]].all()
        want = ref.normals(cloud[rows], k, radius, (0.0, 0.0, 0.0))         # the in-window points alone: each other's neighbours
        per_point = np.zeros_like(cloud)
        per_point[rows] = want["normals"]
        image = np.where(valid[..., None], per_point[np.maximum(lut, 0)], np.float32(0))
        img = got["normals_image"].cpu().numpy()
        assert img.shape == (H, W, 3) and img.dtype == np.float32
        assert np.array_equal(words(img[valid]), words(image[valid]))
        assert np.all(img[~valid] == 0)
        # most normals are a wall's; the fallback rows are the radial default
        solved = np.zeros(len(cloud), bool)
        solved[rows] = want["count"] >= 3
        print(f"pca radius={radius} max_nn={k}: {valid.sum()} pixels, {solved[lut[valid]].mean():.3f} of them solved")
        share = solved[lut[valid]].mean()
        assert share > 0.9 if radius == 0.5 else 0.2 < share < 0.8          # the small radius leaves many returns alone
        axis = np.abs(img[valid][solved[lut[valid]]]).max(1)
        assert np.median(axis) > 0.99
    # "radial", given or by default, is today's output: -unit(point), bit for bit
    for key in ("lut", "range_image", "valid", "K", "normals_image"):
        assert torch.equal(explicit[key], radial[key]), key
    lut = radial["lut"].cpu().numpy()
    valid = lut >= 0
    exp = np.where(valid[..., None], -cloud[lut] / rng32[lut][..., None], np.float32(0)).astype(np.float32)
    assert np.array_equal(words(radial["normals_image"].cpu().numpy()), words(exp))


def test_cloud_normals_tool_round_trip(device, tmp_path):
    pts, full, _ = lattice_case(1500)
    ply_io.save_point_cloud(tmp_path / "in.ply", pts, np.zeros_like(pts))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cloud_normals.py"), str(tmp_path / "in.ply"),
                          str(tmp_path / "out.ply"), "--radius", "0.75", "--max-nn", "40", "--viewpoint", "1", "2", "30"],
                         check=True, capture_output=True, text=True, timeout=300)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    want = ref.normals(pts, 40, 0.75, (1.0, 2.0, 30.0), full=full)
    got_p, got_n = ply_io.load_point_cloud(tmp_path / "out.ply")
    assert np.array_equal(words(got_p), words(pts)) and np.array_equal(words(got_n), words(want["normals"]))
    assert line["points"] == 1500 and line["max_nn"] == 40 and line["fallback_points"] == int((want["count"] < 3).sum())
    assert abs(line["mean_neighbours"] - want["count"].mean()) < 1e-9
