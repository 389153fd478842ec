"""sls_nn_query_k / sls_outlier_statistical / sls_outlier_radius and their Python faces (splat_loam_amd/evaluation.py,
meshing.py) on the device against the NumPy restatement (outlier_ref.py).

Lattice inputs (multiples of 1/16, differences of magnitude <= 128) make the kernel's float32 squared distance exact, so
the restatement's float64 values are its bits: neighbour indices, distances, means, kept rows compare with array_equal.
cloud_mean, std and thr are float64 sums taken in another order than NumPy's: 1e-12 relative, and the kept mask is compared
only where the restatement says no mean lies within 1e-6 (relative) of the threshold — asserted, for every input used."""
import functools

import numpy as np
import pytest
import torch

import nn_ref
import outlier_ref as ref
from splat_loam_amd import evaluation, knn, meshing

pytestmark = pytest.mark.gpu
KS = (1, 2, 3, 8, 9, 16, 17, 20, 32)


def lattice(rng, n, half=64.0, step=16):
    return (rng.integers(-int(half * step), int(half * step) + 1, (n, 3)) / float(step)).astype(np.float32)


def check_nearest_k(device, target, query, what, ks=KS):
    """nearest_k at every k of `ks` against the restatement (one brute force at k = 32: a shorter list is its head), and
    k = 1 against `nearest`.  query None: the cloud queried by itself (the same tensor: the self-query path)."""
    t = torch.tensor(target, device=device)
    q = t if query is None else torch.tensor(query, device=device)
    want2, wanti = ref.nearest_k(target, target if query is None else query, 32)
    for k in ks:
        d2, idx = evaluation.nearest_k(t, q, k)
        assert d2.shape == idx.shape == (len(q), k) and d2.dtype == torch.float32 and idx.dtype == torch.int32
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        bad = np.flatnonzero(((d2.view(np.uint32) != want2[:, :k].view(np.uint32)) | (idx != wanti[:, :k])).any(1))
        assert bad.size == 0, f"{what} k={k}: {bad.size} of {len(q)} rows differ, first {bad[:3]}: got {d2[bad[:3]]} {idx[bad[:3]]}, " \
                              f"want {want2[bad[:3], :k]} {wanti[bad[:3], :k]}"
        if k == 1:
            n2, ni = evaluation.nearest(t, q)
            assert np.array_equal(n2.cpu().numpy().view(np.uint32), d2[:, 0].view(np.uint32)) and np.array_equal(ni.cpu().numpy(), idx[:, 0])
        if k == 8:
            d2n, none = evaluation.nearest_k(t, q, k, return_index=False)
            assert none is None and np.array_equal(d2n.cpu().numpy().view(np.uint32), d2.view(np.uint32))
    return want2, wanti


# Mt < k, every list length's boundary, a partial last wave, one box plus one point, several boxes
@pytest.mark.parametrize("Mt", [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1500, 3000])
def test_nearest_k_lattice_bit_for_bit(device, Mt):
    rng = np.random.default_rng(Mt)
    target = lattice(rng, Mt, half=32.0)
    check_nearest_k(device, target, None, f"self Mt={Mt}")
    check_nearest_k(device, target, lattice(rng, 150, half=64.0), f"second cloud Mt={Mt}")      # partly outside the target's cube


def test_nearest_k_identical_points(device):
    """100 copies of one point: every distance is 0 and the k lowest indices must come out, in order."""
    target = np.tile(np.array([[2.5, -1.0, 0.25]], np.float32), (100, 1))
    _, wanti = check_nearest_k(device, target, None, "identical")
    assert np.array_equal(wanti, np.tile(np.arange(32, dtype=np.int32), (100, 1)))


def test_nearest_k_massive_ties(device):
    """3000 points on the 33^3 lattice |x| <= 1: duplicates and equal distances everywhere, across boxes."""
    rng = np.random.default_rng(33)
    target = lattice(rng, 3000, half=1.0)
    want2, _ = check_nearest_k(device, target, None, "33^3 lattice")
    assert (want2[:, 1] == 0).mean() > 0.03 and (want2[:, 20] == want2[:, 21]).mean() > 0.5
    check_nearest_k(device, target, lattice(rng, 500, half=1.0), "33^3 lattice, second cloud", ks=(1, 3, 20, 32))


@functools.lru_cache(maxsize=None)
def lidar_cloud():
    """A dense slab and isolated far points, 6000 in all, on the lattice: the far points' bounds are a thousand times the
    slab's, which is what the bounds per group of 8 lanes exist for."""
    rng = np.random.default_rng(77)
    slab = rng.integers(-128, 129, (5900, 3)) / 16.0
    slab[:, 2] = rng.integers(-2, 3, 5900) / 16.0
    far = rng.integers(-1024, 1025, (100, 3)) / 16.0
    pts = np.concatenate([slab, far]).astype(np.float32)
    return pts[rng.permutation(6000)]


def test_nearest_k_lidar_like(device):
    check_nearest_k(device, lidar_cloud(), None, "lidar-like", ks=(1, 3, 9, 20, 32))


def test_self_query_at_4_gives_distCUDA2(device):
    """On a duplicate-free cloud the three nearest OTHERS are slots 1..3 of the self-query: their float32 mean, summed in
    list order, is distCUDA2 bit for bit."""
    rng = np.random.default_rng(4)
    pts = np.unique(np.concatenate([lattice(rng, 3000, half=8.0), lidar_cloud()]), axis=0)
    pts = pts[rng.permutation(len(pts))]
    t = torch.tensor(pts, device=device)
    d2 = evaluation.nearest_k(t, t, 4, return_index=False)[0].cpu().numpy()
    assert np.all(d2[:, 0] == 0) and np.all(d2[:, 1] > 0)
    mine = (d2[:, 1] + d2[:, 2] + d2[:, 3]) / np.float32(3.0)
    assert mine.dtype == np.float32
    assert np.array_equal(mine.view(np.uint32), knn.distCUDA2(t).cpu().numpy().view(np.uint32))


def test_nearest_k_continuous_coordinates(device):
    """5000 normal-distributed points against a float64 brute force: the index SETS agree wherever the k-th and the
    (k+1)-th distance differ by more than 1e-6 relative, the distances to the project's 1e-5 float bar."""
    rng = np.random.default_rng(50)
    pts = rng.normal(0, 10, (5000, 3)).astype(np.float32)
    t = torch.tensor(pts, device=device)
    D = np.concatenate([nn_ref.dist2_matrix(pts[a:a + 500], pts) for a in range(0, 5000, 500)])
    order = np.argsort(D, axis=1, kind="stable")[:, :33]
    Ds = np.take_along_axis(D, order, 1)
    for k in (8, 20, 32):
        d2, idx = evaluation.nearest_k(t, t, k)
        d2, idx = d2.cpu().numpy().astype(np.float64), idx.cpu().numpy()
        assert np.all(np.abs(d2 - Ds[:, :k]) <= 1e-5 * Ds[:, :k] + 1e-30)
        clear = (Ds[:, k] - Ds[:, k - 1]) > 1e-6 * Ds[:, k]
        assert clear.mean() > 0.99
        assert np.array_equal(np.sort(idx[clear], 1), np.sort(order[clear, :k], 1))
        assert np.all(idx[:, 0] == np.arange(5000)) and np.all(np.diff(d2, axis=1) >= 0)


# ---- the filters ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filter_case(M):
    pts = ref.filter_cloud(M, M)
    nrm = np.random.default_rng(M + 1).normal(0, 1, (M, 3)).astype(np.float32)
    return pts, nrm


def bits64(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("M", [63, 257, 1500, 3000])
def test_remove_statistical_outlier(device, M):
    pts, nrm = filter_case(M)
    p, n = torch.tensor(pts, device=device), torch.tensor(nrm, device=device)
    for k in (2, 3, 20, 32):
        want = ref.statistical(pts, k, 2.0)
        removed = 1.0 - want["keep"].mean()
        print(f"M={M} k={k}: margin {want['margin']:.3g}, removed {removed:.3f}, zero means {want['zero_mean']}")
        assert want["margin"] > 1e-6                                    # no mean at the threshold: the masks must be equal
        assert 0 < want["keep"].sum() < M and (k > 2 or want["zero_mean"] >= 2)
        out, out_n, index, det = evaluation.remove_statistical_outlier(p, k, 2.0, normals=n, return_index=True, details=True)
        keep = np.flatnonzero(want["keep"])
        assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), keep)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), pts[keep].view(np.uint32))
        assert np.array_equal(out_n.cpu().numpy().view(np.uint32), nrm[keep].view(np.uint32))
        assert det["kept"] == len(keep) and det["removed"] == M - len(keep) and det["zero_mean"] == want["zero_mean"]
        for key, w in (("cloud_mean", want["cloud_mean"]), ("std", want["std"]), ("threshold", want["thr"])):
            assert abs(det[key] - w) <= 1e-12 * abs(w), (key, det[key], w)
        # a second run: the same bits; the plain form returns the rows alone
        out2, det2 = evaluation.remove_statistical_outlier(p, k, 2.0, details=True)
        assert torch.equal(out2, out) and all(bits64(det2[key]) == bits64(det[key]) for key in ("cloud_mean", "std", "threshold"))
        assert torch.equal(evaluation.remove_statistical_outlier(p, k), out)


def test_statistical_consequences(device):
    """k = 1 removes everything, a single point is removed, M < k works, and an empty cloud stays empty."""
    pts, _ = filter_case(257)
    p = torch.tensor(pts, device=device)
    out, index, det = evaluation.remove_statistical_outlier(p, 1, 2.0, return_index=True, details=True)
    assert out.shape == (0, 3) and index.shape == (0,) and det["zero_mean"] == 257 and det["kept"] == 0 and det["threshold"] == 0.0
    out, det = evaluation.remove_statistical_outlier(p[:1], 3, 2.0, details=True)
    assert out.shape == (0, 3) and det["kept"] == 0 and np.isnan(det["threshold"]) and det["zero_mean"] == 1
    small = pts[20:30]
    want = ref.statistical(small, 32, 1.0)
    assert want["margin"] > 1e-6 and 0 < want["keep"].sum() < 10
    index = evaluation.remove_statistical_outlier(p[20:30], 32, 1.0, return_index=True)[1]
    assert np.array_equal(index.cpu().numpy(), np.flatnonzero(want["keep"]))
    out, det = evaluation.remove_statistical_outlier(p[:0], 20, 2.0, details=True)
    assert out.shape == (0, 3) and det["kept"] == 0 and det["removed"] == 0
    for bad in (dict(nb_neighbors=0), dict(nb_neighbors=33), dict(std_ratio=0.0), dict(std_ratio=float("nan"))):
        with pytest.raises(ValueError):
            evaluation.remove_statistical_outlier(p, **bad)
    with pytest.raises(ValueError):
        evaluation.remove_statistical_outlier(p, normals=p[:5])
    with pytest.raises(ValueError):
        evaluation.nearest_k(p, p, 33)


@pytest.mark.parametrize("M", [63, 257, 1500, 3000])
def test_remove_radius_outlier(device, M):
    pts, nrm = filter_case(M)
    p, n = torch.tensor(pts, device=device), torch.tensor(nrm, device=device)
    dense = {63: 2.0, 257: 1.0, 1500: 0.5, 3000: 0.375}[M]
    for nb, radius in ((0, 0.0625), (1, 0.0625), (3, dense), (19, 3 * dense), (31, 4 * dense), (31, 1000.0)):
        want = ref.radius(pts, nb, radius)
        print(f"M={M} nb_points={nb} radius={radius}: kept {want.sum()}")
        out, out_n, index, det = evaluation.remove_radius_outlier(p, nb, radius, normals=n, return_index=True, details=True)
        keep = np.flatnonzero(want)
        assert np.array_equal(index.cpu().numpy(), keep) and det == {"kept": len(keep), "removed": M - len(keep)}
        assert np.array_equal(out.cpu().numpy().view(np.uint32), pts[keep].view(np.uint32))
        assert np.array_equal(out_n.cpu().numpy().view(np.uint32), nrm[keep].view(np.uint32))
        assert torch.equal(evaluation.remove_radius_outlier(p, nb, radius), out)
        if nb == 0:
            assert len(keep) == M                                           # every point is within any radius of itself
        elif nb == 1 and radius == 0.0625:
            assert 0 < len(keep) < M and want[5] and want[9]              # the copies keep each other
        elif radius == 1000.0:
            assert len(keep) == (M if M > 31 else 0)
        else:
            assert 0 < len(keep) < M
    # the boundary is inside: a point at exactly the radius counts
    pair = torch.tensor([[0.0, 0, 0], [0.75, 0, 0]], device=device)
    assert evaluation.remove_radius_outlier(pair, 1, 0.75).shape[0] == 2 and evaluation.remove_radius_outlier(pair, 1, 0.7499).shape[0] == 0
    for bad in (dict(nb_points=-1, radius=1.0), dict(nb_points=32, radius=1.0), dict(nb_points=3, radius=0.0),
                dict(nb_points=3, radius=float("inf"))):
        with pytest.raises(ValueError):
            evaluation.remove_radius_outlier(p, **bad)


def test_sample_surface_outlier_option(device, tmp_path):
    """sample_surface(outlier_nb=20) is remove_statistical_outlier of sample_surface(); None is the unfiltered cloud; mesh_tsdf
    hands the option on, so the filtered samples name its blocks."""
    from test_tsdf import K2, SEED, VS2, _write_room
    _write_room(tmp_path, True)
    pts, nrm = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    pts0, nrm0, det0 = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, outlier_nb=None, details=True)
    assert torch.equal(pts0.view(torch.int32), pts.view(torch.int32)) and torch.equal(nrm0.view(torch.int32), nrm.view(torch.int32))
    assert "outlier" not in det0
    want_p, want_n, want_i, want_d = evaluation.remove_statistical_outlier(pts, 20, 2.0, normals=nrm, return_index=True, details=True)
    got_p, got_n, det = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, outlier_nb=20, details=True)
    assert torch.equal(got_p.view(torch.int32), want_p.view(torch.int32)) and torch.equal(got_n.view(torch.int32), want_n.view(torch.int32))
    assert torch.equal(det["outlier"].pop("index"), want_i) and det["outlier"] == want_d
    print(f"room: {want_d['kept']} of {pts.shape[0]} samples kept, threshold {want_d['threshold']:.4f} m")
    assert 0 < want_d["kept"] < pts.shape[0]
    assert torch.equal(meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, outlier_nb=20, outlier_std=1.0)[0],
                       evaluation.remove_statistical_outlier(pts, 20, 1.0))
    v, f, mdet = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, outlier_nb=20)
    assert mdet["samples"] == want_d["kept"] and mdet["outlier"]["kept"] == want_d["kept"] and f.shape[0] > 0
