"""sls_cloud_dbscan / sls_cloud_select and their Python faces (splat_loam_amd/evaluation.py: cluster_dbscan, keep_clusters;
meshing.py: the cluster_* options) on the device against include/sls_cluster_math.h compiled for the host — its serial
all-pairs routine, on ANY finite input — and against the NumPy restatement (cluster_ref.py) where the input is a lattice.

Everything is integers and one float32 comparison, so labels, counts and status words are compared with array_equal: no
tolerance anywhere.  The sizes are the smallest that reach every level of the sweep: runs of 32 points, boxes of 256, chunks
of 64 boxes (16 384 points), waves of 64 queries — M = 1, 31, 33, 65, 257, 1 000 and 20 000 (two chunks), rows shuffled."""
import functools

import numpy as np
import pytest
import torch

import cluster_ref as ref
from splat_loam_amd import evaluation, meshing

pytestmark = pytest.mark.gpu
SIZES = (1, 31, 33, 65, 257, 1000, 20000)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the header's serial routine as a host program; None without gcc — the lattice cases are then held against the NumPy
    restatement alone, and only a case that has no restatement (a non-lattice cloud) skips"""
    return ref.build_host(tmp_path_factory.mktemp("cluster_host"))


@functools.lru_cache(maxsize=None)
def cloud(M):
    return ref.lattice_cloud(M, M)


@functools.lru_cache(maxsize=None)
def restated(name, eps, min_points):
    """the NumPy restatement of a named lattice cloud, computed once for all tests"""
    pts = {"line": ref.line_cloud, "dense": ref.dense_cloud}[name]() if isinstance(name, str) else cloud(name)
    return ref.dbscan(pts, eps, min_points)


def run_device(device, pts, eps, min_points):
    labels, counts, det = evaluation.cluster_dbscan(torch.tensor(pts, device=device), eps, min_points, return_counts=True, details=True)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.shape == (len(pts),)
    return labels.cpu().numpy(), counts.cpu().numpy(), det


def check(device, exe, tmp_path, pts, eps, min_points, what, want=None):
    """device == the header's serial routine (and == `want`, the restatement, where given); returns the host's result (the
    restatement's where there is no compiler)"""
    if exe is None and want is None:
        pytest.skip("no gcc, and this cloud has no restatement")
    labels, counts, det = run_device(device, pts, eps, min_points)
    host = ref.run_host(exe, tmp_path, pts, eps, min_points) if exe is not None else None
    assert host is None or host["rc"] == 0
    status = np.array([det["clusters"], det["core"], det["border"], det["noise"], det["largest"], len(pts), 0, 1], np.uint32)
    print(f"{what}: M={len(pts)} eps={eps} min_points={min_points}: status {status[:5].tolist()}")
    for other, name in ((host, "header"), (want, "restatement")):
        if other is None:
            continue
        bad = np.flatnonzero(labels != other["labels"])
        assert bad.size == 0, f"{what}: {bad.size} labels differ from the {name}, first rows {bad[:5]}: {labels[bad[:5]]} / {other['labels'][bad[:5]]}"
        assert np.array_equal(counts, other["counts"]), f"{what}: counts differ from the {name}"
        assert np.array_equal(status, other["status"]), f"{what}: status {status} / {name} {other['status']}"
    return host if host is not None else want


@pytest.mark.parametrize("M", SIZES)
def test_lattice_clouds_bit_for_bit(device, exe, tmp_path, M):
    pts = cloud(M)
    for eps, mp in ((0.25, 4), (0.5, 10)):
        host = check(device, exe, tmp_path, pts, eps, mp, "lattice", restated(M, eps, mp))
    if M >= 1000:
        assert host["status"][0] > 1 and host["status"][2] > 0 and host["status"][3] > 0      # clusters, borders and noise


@pytest.mark.parametrize("M", SIZES)
def test_min_points_1_100_and_beyond_M(device, exe, tmp_path, M):
    pts = cloud(M)
    host = check(device, exe, tmp_path, pts, 0.25, 1, "min_points=1", restated(M, 0.25, 1))
    assert host["status"][1] == M and host["status"][2] == 0 and host["status"][3] == 0         # components of the eps-graph
    host = check(device, exe, tmp_path, pts, 1.0, 100, "min_points=100", restated(M, 1.0, 100))   # beyond the 32 of the k-lists
    assert M < 20000 or host["status"][0] >= 1
    host = check(device, exe, tmp_path, pts, 0.5, M + 1, "min_points>M", ref.dbscan(pts, 0.5, M + 1))
    assert host["status"][:5].tolist() == [0, 0, 0, M, 0] and np.all(host["labels"] == -1)


@pytest.mark.parametrize("mp", [3, 10, 33, 100])
def test_saturation_boundary_at_exactly_eps(device, exe, tmp_path, mp):
    """neighbour counts of min_points - 1, min_points, min_points + 1, every neighbour AT eps = 0.25 or an exact copy"""
    pts, centres = ref.saturation_cloud(mp)
    host = check(device, exe, tmp_path, pts, 0.25, mp, "saturation", ref.dbscan(pts, 0.25, mp))
    assert host["status"][0] == 2 and host["counts"].tolist() == [mp, mp + 1] and np.all(host["labels"][:centres[1]] == -1)
    # ... and the same stars inside a cloud of several boxes
    big = np.concatenate([cloud(1000) + np.float32(30.0), pts]).astype(np.float32)
    big = big[np.random.default_rng(mp).permutation(len(big))]
    check(device, exe, tmp_path, big, 0.25, mp, "saturation in a cloud", ref.dbscan(big, 0.25, mp))


def test_exact_duplicates(device, exe, tmp_path):
    pts = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (300, 1))
    host = check(device, exe, tmp_path, pts, 0.0625, 300, "copies", ref.dbscan(pts, 0.0625, 300))
    assert host["status"].tolist() == [1, 300, 0, 0, 300, 300, 0, 1]
    assert check(device, exe, tmp_path, pts, 0.0625, 301, "copies, one short", ref.dbscan(pts, 0.0625, 301))["status"][3] == 300
    mixed = np.concatenate([cloud(1000), cloud(1000)[:400]])                                   # 400 rows twice
    check(device, exe, tmp_path, mixed, 0.25, 6, "a cloud with copies", ref.dbscan(mixed, 0.25, 6))


def test_bridge_and_numbering_by_core(device, exe, tmp_path):
    pts = ref.bridge_cloud()
    host = check(device, exe, tmp_path, pts, 0.25, 20, "bridge", ref.dbscan(pts, 0.25, 20))
    assert host["status"].tolist() == [2, 54, 1, 0, 28, 55, 0, 1] and host["labels"][0] == 0 and host["counts"].tolist() == [28, 27]
    front = np.concatenate([pts[:1], pts[1:28] + np.float32(8.0), pts[28:]])                   # (test_cluster_math.py says why)
    host = check(device, exe, tmp_path, front, 0.25, 20, "front border", ref.dbscan(front, 0.25, 20))
    assert host["labels"][0] == 1 and host["counts"].tolist() == [27, 28]
    # ... and with 2 000 other points around them, so that the blobs lie in different boxes than the bridge
    big = np.concatenate([front[:1], cloud(1000) + np.float32(20.0), front[1:], cloud(1000) - np.float32(20.0)]).astype(np.float32)
    host = check(device, exe, tmp_path, big, 0.25, 20, "front border in a cloud", ref.dbscan(big, 0.25, 20))
    assert host["labels"][0] >= 0 and host["labels"][0] == host["labels"][-1001]


def test_line_across_many_boxes(device, exe, tmp_path):
    """5 000 points at 0.8 eps spacing, shuffled: one cluster that crosses every box — a deep union-find"""
    host = check(device, exe, tmp_path, ref.line_cloud(), 5 / 16, 2, "line", restated("line", 5 / 16, 2))
    assert host["status"].tolist() == [1, 5000, 0, 0, 5000, 5000, 0, 1]
    host = check(device, exe, tmp_path, ref.line_cloud(), 5 / 16, 3, "line, ends are borders", restated("line", 5 / 16, 3))
    assert host["status"].tolist() == [1, 4998, 2, 0, 5000, 5000, 0, 1]


def test_one_dense_component_of_20000(device, exe, tmp_path):
    """contention: every unite lands in one component; at min_points = 100 the block's skin is border"""
    host = check(device, exe, tmp_path, ref.dense_cloud(), 2 / 16, 10, "dense", restated("dense", 2 / 16, 10))
    assert host["status"].tolist() == [1, 20000, 0, 0, 20000, 20000, 0, 1]
    host = check(device, exe, tmp_path, ref.dense_cloud(), 3 / 16, 100, "dense, min_points=100", restated("dense", 3 / 16, 100))
    assert host["status"][0] == 1 and host["status"][2] > 1000 and host["status"][4] > 19000


@pytest.mark.parametrize("M", SIZES)
def test_random_float_clouds_against_the_header(device, exe, tmp_path, M):
    """non-lattice float32 coordinates: no restatement, the header's serial routine on the same bits"""
    rng = np.random.default_rng(1000 + M)
    n = max(1, M // 40)
    pts = (rng.normal(0, 3.0, (n, 3))[rng.integers(0, n, M)] + rng.normal(0, 0.15, (M, 3)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    host = check(device, exe, tmp_path, pts, 0.31, 12, "random")
    if M >= 1000:
        assert host["status"][0] > 1 and host["status"][2] > 0 and host["status"][3] > 0
    lidar = (pts * np.array([1, 1, 0.02], np.float32)).astype(np.float32)                      # a thin slab
    lidar[: M // 50] *= np.float32(40.0)                                                      # ... and far, isolated returns
    check(device, exe, tmp_path, lidar, 0.1, 8, "slab")


def test_the_same_call_twice_gives_equal_bytes(device):
    pts = torch.tensor(ref.dense_cloud(), device=device)
    a = evaluation.cluster_dbscan(pts, 2 / 16, 10, return_counts=True, details=True)
    b = evaluation.cluster_dbscan(pts, 2 / 16, 10, return_counts=True, details=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    pts = torch.tensor(cloud(20000), device=device)
    a, b = (evaluation.cluster_dbscan(pts, 0.25, 4, return_counts=True, details=True) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    ka, kb = (evaluation.keep_clusters(pts, 0.25, 4, keep=3, return_index=True) for _ in range(2))
    assert torch.equal(ka[0], kb[0]) and torch.equal(ka[1], kb[1])


def test_empty_cloud_and_return_shapes(device):
    empty = torch.zeros((0, 3), device=device)
    labels, counts, det = evaluation.cluster_dbscan(empty, 0.5, return_counts=True, details=True)
    assert labels.shape == (0,) and counts.shape == (0,) and det == {"clusters": 0, "core": 0, "border": 0, "noise": 0, "largest": 0}
    out, out_n, index, det = evaluation.keep_clusters(empty, 0.5, min_cluster_points=7, normals=empty, return_index=True, details=True)
    assert out.shape == out_n.shape == (0, 3) and index.shape == (0,) and det["kept"] == 0 and det["removed"] == 0 and det["n_min"] == 7
    pts = torch.tensor(cloud(257), device=device)
    assert isinstance(evaluation.cluster_dbscan(pts, 0.5), torch.Tensor) and isinstance(evaluation.keep_clusters(pts, 0.5), torch.Tensor)
    assert len(evaluation.cluster_dbscan(pts, 0.5, details=True)) == 2
    for bad in (dict(eps=0.0), dict(eps=float("nan")), dict(eps=0.5, min_points=0)):
        with pytest.raises(ValueError):
            evaluation.cluster_dbscan(pts, **bad)
    with pytest.raises(ValueError):
        evaluation.keep_clusters(pts, 0.5, normals=pts[:5])


# ---- selection -------------------------------------------------------------------------------------------------------
def tie_cloud():
    """two blobs of 27 points, one of 20, one lone point: at eps = 0.25, min_points = 5 three clusters of 27, 27, 20 and noise"""
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float32) / 16
    pts = np.concatenate([g, g + np.float32(4.0), (g + np.float32(8.0))[:20], [[20.0, 0, 0]]]).astype(np.float32)
    return pts[np.random.default_rng(8).permutation(len(pts))]


@pytest.mark.parametrize("keep,floor,kept", [(1, 0, 54), (2, 0, 54), (3, 0, 74), (0, 0, 74), (0, 21, 54), (1, 28, 0), (5, 0, 74), (-2, 27, 54)])
def test_selection_ties_keep_0_and_the_floor(device, exe, tmp_path, keep, floor, kept):
    pts = tie_cloud()
    nrm = np.random.default_rng(9).normal(0, 1, pts.shape).astype(np.float32)
    if exe is not None:
        host = ref.run_host(exe, tmp_path, pts, 0.25, 5, keep, floor)
    else:
        host = ref.dbscan(pts, 0.25, 5)
        host["index"], host["select_status"] = ref.select(host["labels"], host["counts"], keep, floor)
    assert host["status"][0] == 3 and host["select_status"][0] == kept
    p, n = torch.tensor(pts, device=device), torch.tensor(nrm, device=device)
    out, out_n, index, det = evaluation.keep_clusters(p, 0.25, 5, keep=keep, min_cluster_points=floor, normals=n, return_index=True, details=True)
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), host["index"])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pts[host["index"]].view(np.uint32))        # rows and normals travel along
    assert np.array_equal(out_n.cpu().numpy().view(np.uint32), nrm[host["index"]].view(np.uint32))
    assert [det["kept"], det["n_min"], det["kept"] + det["removed"]] == host["select_status"][:3].tolist() and det["clusters"] == 3
    assert torch.equal(evaluation.keep_clusters(p, 0.25, 5, keep=keep, min_cluster_points=floor), out)


def test_selection_of_all_noise_is_empty(device):
    pts = torch.tensor(cloud(1000), device=device)
    out, index, det = evaluation.keep_clusters(pts, 0.5, 1001, return_index=True, details=True)
    assert out.shape == (0, 3) and index.shape == (0,) and det["kept"] == 0 and det["clusters"] == 0 and det["noise"] == 1000 and det["n_min"] == 0


@pytest.mark.parametrize("M", [257, 1000, 20000])
def test_keep_clusters_is_cluster_dbscan_then_the_rule(device, M):
    pts = cloud(M)
    p = torch.tensor(pts, device=device)
    labels, counts = evaluation.cluster_dbscan(p, 0.25, 4, return_counts=True)
    for keep, floor in ((1, 0), (3, 0), (0, 6), (10, 5)):
        want, status = ref.select(labels.cpu().numpy(), counts.cpu().numpy(), keep, floor)
        out, index, det = evaluation.keep_clusters(p, 0.25, 4, keep=keep, min_cluster_points=floor, return_index=True, details=True)
        assert np.array_equal(index.cpu().numpy(), want) and [det["kept"], det["n_min"]] == status[:2].tolist()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), pts[want].view(np.uint32))


# ---- the pipeline hook -----------------------------------------------------------------------------------------------
def test_sample_surface_cluster_option(device, tmp_path):
    """cluster_eps=None is the cloud it always was.  Then a floater is planted in the room — a patch of surfels 1 m from the
    model's origin, where the room's shell is 2.4 - 2.6 m away.  Its samples pass the statistical filter, which removes
    only the thin rim of mixed-depth samples around it; the cluster stage behind that filter then drops exactly the
    floater's samples, and mesh_tsdf hands the options on."""
    from splat_loam_amd import ply_io, synth
    from test_tsdf import H2, K2, SEED, VS2, W2, _write_room
    _write_room(tmp_path, True)
    pts, nrm = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    pts0, nrm0, det0 = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, cluster_eps=None, details=True)
    assert torch.equal(pts0.view(torch.int32), pts.view(torch.int32)) and torch.equal(nrm0.view(torch.int32), nrm.view(torch.int32))
    assert "cluster" not in det0
    # the room again, with a floater: the surfels within 20 degrees of -x once more at 0.4 of their range and size
    sc = synth.make_scene(6000, H2, W2, seed=77, range_lo=2.4, range_hi=2.6, scale_lo=0.06, scale_hi=0.15, opac_lo=0.6, max_tilt_deg=10.0)
    ray = sc["means"] / np.linalg.norm(sc["means"], axis=1, keepdims=True)
    patch = ray[:, 0] < -np.cos(np.radians(20.0))
    assert 100 < patch.sum() < 1500
    cat = lambda a, s: np.concatenate([a, a[patch] * np.float32(s)]).astype(np.float32)
    opac = cat(sc["opac"], 1.0)
    ply_io.save_ply(tmp_path / "models/model_0.ply", cat(sc["means"], 0.4), np.log(opac / (1 - opac)), np.log(cat(sc["scales"], 0.4)),
                    cat(sc["rots"], 1.0))
    pts, nrm = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    # the unfiltered cloud: the hook is keep_clusters of it
    want_p, want_n, want_i, want_d = evaluation.keep_clusters(pts, 0.3, 10, normals=nrm, return_index=True, details=True)
    got_p, got_n, det = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, cluster_eps=0.3, details=True)
    assert torch.equal(got_p.view(torch.int32), want_p.view(torch.int32)) and torch.equal(got_n.view(torch.int32), want_n.view(torch.int32))
    assert torch.equal(det["cluster"].pop("index"), want_i) and det["cluster"] == want_d and 0 < want_d["kept"] < pts.shape[0]
    # behind the outlier stage: the floater (within 1.3 m of the origin) has passed it, nothing is left between it and the room
    stat_p, stat_n = evaluation.remove_statistical_outlier(pts, 20, 2.0, normals=nrm)
    rng_m = stat_p.norm(dim=1).cpu().numpy()
    floater = rng_m < 1.3
    print(f"room with a floater: {len(rng_m)} of {pts.shape[0]} samples pass the statistical filter, {floater.sum()} of them on the floater, "
          f"{((rng_m >= 1.3) & (rng_m < 2.3)).sum()} in between; unfiltered at eps 0.3: {want_d}")
    assert floater.sum() >= 50 and not ((rng_m >= 1.3) & (rng_m < 2.3)).any()
    both_p, both_n, det = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, outlier_nb=20, cluster_eps=0.5, details=True)
    room = torch.from_numpy(np.flatnonzero(~floater)).to(device)
    assert torch.equal(det["cluster"]["index"].long(), room)                                   # exactly the floater's samples go
    assert torch.equal(both_p.view(torch.int32), stat_p[room].view(torch.int32)) and torch.equal(both_n.view(torch.int32), stat_n[room].view(torch.int32))
    assert det["outlier"]["kept"] == stat_p.shape[0] and det["cluster"]["kept"] == both_p.shape[0] and det["cluster"]["clusters"] == 2
    # its own options arrive: every cluster of at least 30 points, the floater among them
    all_p = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device, outlier_nb=20, cluster_eps=0.5, cluster_min_points=5,
                                   cluster_keep=0, cluster_min_size=30)[0]
    assert torch.equal(all_p, evaluation.keep_clusters(stat_p, 0.5, 5, keep=0, min_cluster_points=30)) and all_p.shape[0] > both_p.shape[0]
    v, f, mdet = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, outlier_nb=20, cluster_eps=0.5)
    v0, f0, mdet0 = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, outlier_nb=20)
    print(f"    mesh_tsdf: {mdet['blocks']} blocks with cluster_eps, {mdet0['blocks']} without")
    assert mdet["samples"] == both_p.shape[0] and mdet["cluster"]["kept"] == both_p.shape[0] and f.shape[0] > 0
    assert mdet["blocks"] < mdet0["blocks"] and "cluster" not in mdet0


def test_cloud_cluster_tool(device, tmp_path):
    """tools/cloud_cluster.py: the kept cloud with its normals as a child process, the whole cloud coloured by label through
    the tool's own main in this process — noise grey, one colour per cluster."""
    import json
    import os
    import runpy
    import subprocess
    import sys
    from splat_loam_amd import ply_io
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pts = cloud(1000)
    nrm = np.random.default_rng(12).normal(0, 1, pts.shape).astype(np.float32)
    ply_io.save_point_cloud(tmp_path / "in.ply", pts, nrm)
    want = ref.dbscan(pts, 0.5, 10)
    index, status = ref.select(want["labels"], want["counts"], 2, 40)
    assert want["status"][0] > 2 and want["status"][3] > 0 and 0 < len(index) < 1000
    tool = [sys.executable, os.path.join(root, "tools", "cloud_cluster.py"), str(tmp_path / "in.ply")]
    out = subprocess.run(tool + [str(tmp_path / "out.ply"), "--eps", "0.5", "--min-points", "10", "--keep", "2", "--min-cluster", "40"],
                         check=True, capture_output=True, text=True, timeout=300)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    got_p, got_n = ply_io.load_point_cloud(tmp_path / "out.ply")
    assert np.array_equal(got_p.view(np.uint32), pts[index].view(np.uint32)) and np.array_equal(got_n.view(np.uint32), nrm[index].view(np.uint32))
    assert [line["points"], line["kept"], line["n_min"], line["clusters"], line["noise"]] == [1000, len(index), int(status[1]), int(want["status"][0]),
                                                                                             int(want["status"][3])]
    # --labels, in this process (the tool's own main, its arguments in sys.argv)
    argv = sys.argv
    sys.argv = tool[1:] + [str(tmp_path / "labels.ply"), "--eps", "0.5", "--min-points", "10", "--labels", "--device", str(device)]
    try:
        runpy.run_path(tool[1], run_name="__main__")
    finally:
        sys.argv = argv
    all_p, all_n, rgb = ply_io.load_point_cloud(tmp_path / "labels.ply", return_colors=True)
    assert np.array_equal(all_p.view(np.uint32), pts.view(np.uint32)) and np.array_equal(all_n.view(np.uint32), nrm.view(np.uint32))
    assert rgb.dtype == np.uint8 and rgb.shape == (1000, 3)
    noise = want["labels"] < 0
    assert np.all(rgb[noise] == 128) and np.all(rgb[~noise].min(1) >= 96) and not np.any(np.all(rgb[~noise] == 128, 1))
    for c in range(int(want["status"][0])):                                     # one colour per cluster, a function of the label alone
        rows = rgb[want["labels"] == c]
        assert np.all(rows == rows[0])
    assert len(np.unique(rgb[~noise], axis=0)) == int(want["status"][0])
