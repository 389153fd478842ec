"""sls_voxel_downsample / sls_mesh_sample / evaluation.evaluate_recon on the device against the NumPy restatement
(cloud_ref.py).

Lattice inputs (multiples of 1/16, magnitude <= 64) make every float64 sum of a voxel exact in any order, so there
rows, counts and centroids are compared with array_equal on the bits.  Open3D is not installed: both operations are
pinned against the restatement of their documented behaviour, not against Open3D itself."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_ref
import nn_ref
from splat_loam_amd import evaluation, ply_io
from test_nn_query import lattice, lidar_cloud

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- voxel down-sampling ---------------------------------------------------------------------------------------------
def run_voxel(device, points, voxel_size):
    rows, counts = evaluation.voxel_down_sample(torch.tensor(points, device=device), voxel_size, return_counts=True)
    assert rows.dtype == torch.float32 and counts.dtype == torch.int32 and rows.shape == (counts.shape[0], 3)
    return rows.cpu().numpy(), counts.cpu().numpy()


def assert_voxels_bitwise(device, points, voxel_size, what):
    rows, counts = run_voxel(device, points, voxel_size)
    want_rows, want_counts = cloud_ref.voxel_down_sample(points, voxel_size)
    assert len(rows) == len(want_rows), f"{what}: {len(rows)} voxels, want {len(want_rows)}"
    assert np.array_equal(counts, want_counts), what
    bad = np.flatnonzero((rows.view(np.uint32) != want_rows.view(np.uint32)).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(rows)} rows differ, first {bad[:5]}: got {rows[bad[:5]]}, want {want_rows[bad[:5]]}"
    return rows, counts


# the granularities of the wave (64), the workgroup (256) and the sorter's and the scan's chunk (1024)
@pytest.mark.parametrize("voxel_size", [0.125, 0.3, 1.0, 200.0])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 6000])
def test_voxel_lattice_bit_for_bit(device, M, voxel_size):
    """0.125 puts lattice points exactly on voxel faces, 0.3 is not representable (the double division decides), 1.0 gives
    voxels of a few points, 200 one voxel for the whole cloud (its extent, 64, is below half the voxel: the long-segment
    path from 65 points on)."""
    rng = np.random.default_rng(100 * M + int(voxel_size * 1000))
    points = lattice(rng, M, half=32.0 if voxel_size == 200.0 else 64.0)
    rows, counts = assert_voxels_bitwise(device, points, voxel_size, f"M={M} voxel_size={voxel_size}")
    assert counts.sum() == M
    if voxel_size == 200.0:
        assert len(rows) == 1 and counts[0] == M
    if voxel_size == 0.125 and M >= 1000:
        on_face = ((points.astype(np.float64) - points.min(0)) / 0.125 + 0.5) % 1.0 == 0.0
        assert on_face.any()


def test_voxel_segments(device):
    rng = np.random.default_rng(3)
    # 5000 copies and neighbours inside ONE voxel (coordinates 0 .. 7/16 at voxel size 1: the cell is [-0.5, 0.5)), next to
    # 700 points elsewhere: the long-segment path beside short ones
    dense = rng.integers(0, 8, (5000, 3)) / 16.0
    dense[:1500] = dense[0]
    points = np.concatenate([dense, lattice(rng, 700, half=20.0) + np.float32(30.0)]).astype(np.float32)
    points = points[rng.permutation(len(points))]
    rows, counts = assert_voxels_bitwise(device, points, 1.0, "one dense voxel")
    assert counts[0] == 5000 and counts.max() == 5000 and (counts[1:] <= 64).all()
    # segments of exactly 64, 65 and 128 points (the threshold between the two paths)
    parts = [np.tile([[4.0 * k, 0, 0]], (n, 1)) + rng.integers(0, 8, (n, 3)) / 16.0 for k, n in enumerate((64, 65, 128, 1, 63))]
    points = np.concatenate(parts).astype(np.float32)
    _, counts = assert_voxels_bitwise(device, points[rng.permutation(len(points))], 1.0, "threshold segments")
    assert counts.tolist() == [64, 65, 128, 1, 63]
    # every point in a voxel of its own
    g = np.stack(np.meshgrid(np.arange(13), np.arange(11), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
    points = (g[rng.permutation(len(g))] - 5.0).astype(np.float32)
    rows, counts = assert_voxels_bitwise(device, points, 0.5, "a voxel per point")
    assert len(rows) == len(points) == 1287 and (counts == 1).all()
    assert np.array_equal(rows, points[np.lexsort((points[:, 0], points[:, 1], points[:, 2]))])     # key order: z, then y, then x
    # only negative coordinates
    points = lattice(rng, 3000, half=16.0) - np.float32(40.0)
    assert points.max() < 0
    assert_voxels_bitwise(device, points, 0.3, "negative coordinates")
    # the output depends on the SET: a shuffled copy gives the same rows (lattice: bit for bit)
    points = lattice(rng, 5000, half=8.0)
    rows, counts = run_voxel(device, points, 0.3)
    rows2, counts2 = run_voxel(device, points[rng.permutation(len(points))], 0.3)
    assert np.array_equal(rows.view(np.uint32), rows2.view(np.uint32)) and np.array_equal(counts, counts2)
    # without the counts: the same rows; an empty cloud
    only = evaluation.voxel_down_sample(torch.tensor(points, device=device), 0.3)
    assert np.array_equal(only.cpu().numpy().view(np.uint32), rows.view(np.uint32))
    empty = evaluation.voxel_down_sample(torch.zeros((0, 3), device=device), 0.3)
    assert empty.shape == (0, 3) and empty.dtype == torch.float32


@pytest.mark.parametrize("voxel_size", [0.02, 0.5])
def test_voxel_lidar_like_cloud(device, voxel_size):
    """Not on a lattice: the voxel set and the counts equal the restatement's (the same float64 index arithmetic), the
    centroids agree within one float32 ulp of the cloud's largest |coordinate| (the double sums differ by their order, far
    below the final rounding to float32), and two runs give the same bits."""
    points = lidar_cloud()
    assert len(points) == 13340
    rows, counts = run_voxel(device, points, voxel_size)
    want_rows, want_counts = cloud_ref.voxel_down_sample(points, voxel_size)
    assert len(rows) == len(want_rows) and np.array_equal(counts, want_counts)
    assert counts.max() > 64 and (counts == 1).any()                            # both summation paths
    ulp = float(np.spacing(np.float32(np.abs(points).max())))
    err = float(np.abs(rows.astype(np.float64) - want_rows.astype(np.float64)).max())
    print(f"voxel_size {voxel_size}: {len(rows)} voxels, largest voxel {counts.max()}, centroid error {err:.3g} (one ulp: {ulp:.3g})")
    assert err <= ulp
    rows2, counts2 = run_voxel(device, points, voxel_size)
    assert np.array_equal(rows.view(np.uint32), rows2.view(np.uint32)) and np.array_equal(counts, counts2)


def test_voxel_errors_are_status_paths(device):
    rng = np.random.default_rng(4)
    points = lattice(rng, 3000)
    for bad in (np.nan, np.inf, -np.inf):
        p = points.copy()
        p[1234, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            evaluation.voxel_down_sample(torch.tensor(p, device=device), 0.3)
    with pytest.raises(ValueError, match="non-finite"):
        evaluation.voxel_down_sample(torch.full((100, 3), float("nan"), device=device), 0.3)
    with pytest.raises(ValueError, match="2\\^21"):
        evaluation.voxel_down_sample(torch.tensor([[0.0, 0, 0], [64.0, 0, 0]], device=device), 2.0 ** -16)
    with pytest.raises(ValueError, match="2\\^21"):
        evaluation.voxel_down_sample(torch.tensor([[0.0, 0, 0], [0, 3e38, 0]], device=device), 1e-30)
    for vs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            evaluation.voxel_down_sample(torch.tensor(points, device=device), vs)
    assert_voxels_bitwise(device, points, 0.3, "after the errors")             # the device is fine


# ---- mesh sampling ---------------------------------------------------------------------------------------------------
def run_mesh(device, vertices, faces, n, seed=0, crop_box=None):
    pts, face = evaluation.sample_mesh(torch.tensor(vertices, device=device), torch.tensor(faces, device=device), n, seed=seed,
                                       crop_box=crop_box, return_faces=True)
    assert pts.dtype == torch.float32 and pts.shape == (n, 3) and face.dtype == torch.int32 and face.shape == (n,)
    return pts.cpu().numpy(), face.cpu().numpy()


MESHES = {
    "one triangle": (np.array([[1.25, -3, 0.5], [40, 2.0625, -7], [-12.5, 9, 33]], np.float32), np.array([[0, 1, 2]], np.int32)),
    "1 : 3": cloud_ref.ONE_TO_THREE,
    "grid": cloud_ref.grid_mesh()[:2],
}


@pytest.mark.parametrize("n", [1, 64, 65, 1000, 20000])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_mesh_sample_against_the_restatement(device, mesh, n):
    vertices, faces = MESHES[mesh]
    pts, face = run_mesh(device, vertices, faces, n, seed=11)
    want64, want_face = cloud_ref.sample_mesh(vertices, faces, n, seed=11)
    assert np.array_equal(face, want_face)
    scale = float(np.abs(vertices).max())
    err = float(np.abs(pts.astype(np.float64) - want64).max())
    assert err <= 1e-5 * scale, f"{mesh} n={n}: {err} against a scale of {scale}"
    want32 = cloud_ref.sample_mesh(vertices, faces, n, seed=11, float32=True)[0]
    assert np.array_equal(pts.view(np.uint32), want32.view(np.uint32))          # the header's float32 arithmetic: the same bits
    if mesh == "grid" and n == 20000:
        zero = cloud_ref.grid_mesh()[2]
        assert not np.isin(face, zero).any() and len(np.unique(face)) == 128 - len(zero)
        assert np.isin([9, 10, 11, 60, 3], face).all()                          # (repeated faces are faces of their own)


def test_mesh_sample_is_a_pure_function_of_the_index(device):
    vertices, faces = MESHES["grid"]
    pts, face = run_mesh(device, vertices, faces, 5000, seed=3)
    again, face_again = run_mesh(device, vertices, faces, 5000, seed=3)
    assert np.array_equal(pts.view(np.uint32), again.view(np.uint32)) and np.array_equal(face, face_again)
    other, face_other = run_mesh(device, vertices, faces, 5000, seed=4)
    assert (face != face_other).mean() > 0.9 and (pts != other).any(1).mean() > 0.99
    big, face_big = run_mesh(device, vertices, faces, 5000, seed=3 + (1 << 32))        # the seed's high word counts
    assert (face != face_big).mean() > 0.9
    longer, face_longer = run_mesh(device, vertices, faces, 12345, seed=3)
    assert np.array_equal(longer[:5000].view(np.uint32), pts.view(np.uint32)) and np.array_equal(face_longer[:5000], face)
    only = evaluation.sample_mesh(torch.tensor(vertices, device=device), torch.tensor(faces, device=device).long(), 5000, seed=3)
    assert np.array_equal(only.cpu().numpy().view(np.uint32), pts.view(np.uint32))     # int64 faces, no face output
    none = evaluation.sample_mesh(torch.tensor(vertices, device=device), torch.tensor(faces, device=device), 0)
    assert none.shape == (0, 3)


def test_mesh_sample_crop_box(device):
    vertices, faces = MESHES["grid"]
    box = [-4, -4, -1, 0, 4, 1]                                                 # x <= 0: the left half, its edge ON the box face
    pts, face = run_mesh(device, vertices, faces, 20000, seed=5, crop_box=box)
    want64, want_face = cloud_ref.sample_mesh(vertices, faces, 20000, seed=5, crop_box=box)
    assert np.array_equal(face, want_face) and np.abs(pts - want64).max() <= 1e-5 * 4
    drawn = vertices[faces[np.unique(face)]]
    assert (drawn[:, :, 0] <= 0).all() and (drawn[:, :, 0] == 0).any()          # a vertex exactly on the box face is inside
    assert pts[:, 0].max() <= 0 and pts[:, 0].max() > -0.01
    outside = (vertices[faces][:, :, 0] > 0).any(1)
    assert outside.sum() == 64 and not np.isin(face, np.flatnonzero(outside)).any()
    # the box as a device tensor; a box that holds one row of vertices only: no face is left
    dev_box = torch.tensor(box, dtype=torch.float32, device=device)
    assert np.array_equal(run_mesh(device, vertices, faces, 20000, seed=5, crop_box=dev_box)[1], face)
    with pytest.raises(ValueError, match="no area"):
        run_mesh(device, vertices, faces, 100, crop_box=[-4, -4, -1, -4, 4, 1])


def test_mesh_sample_proportions(device):
    """Areas 1 : 3, n = 200 000: the share of the small face within 5 sigma of 0.25, sigma = sqrt(.25 .75 / n) = 0.00097
    (test_cloud_host.py checks that the restatement alone meets this with the same seed)."""
    vertices, faces = cloud_ref.ONE_TO_THREE
    n = cloud_ref.PROPORTION_N
    pts, face = run_mesh(device, vertices, faces, n, seed=cloud_ref.PROPORTION_SEED)
    share, sigma = float((face == 0).mean()), float(np.sqrt(0.25 * 0.75 / n))
    print(f"share of the small face {share:.5f} ({(share - 0.25) / sigma:+.2f} sigma)")
    assert abs(share - 0.25) <= 5 * sigma
    assert np.array_equal(face, cloud_ref.sample_mesh(vertices, faces, n, seed=cloud_ref.PROPORTION_SEED)[1])


def test_mesh_sample_errors(device):
    vertices, faces, zero = cloud_ref.grid_mesh()
    for index in (-1, len(vertices), 2 ** 31 - 1):
        bad = faces.copy()
        bad[17, 1] = index
        with pytest.raises(ValueError, match="index outside"):
            run_mesh(device, vertices, bad, 100)
    with pytest.raises(ValueError, match="no area"):
        run_mesh(device, vertices, faces[zero], 100)                            # every face degenerate
    with pytest.raises(ValueError, match="no area"):
        run_mesh(device, vertices, np.zeros((0, 3), np.int32), 100)             # no face
    nanv = np.full_like(vertices, np.nan)
    with pytest.raises(ValueError, match="no area"):
        run_mesh(device, nanv, faces, 100)                                      # no finite area
    with pytest.raises(ValueError):
        evaluation.sample_mesh(torch.tensor(vertices, device=device), torch.zeros((4, 2), dtype=torch.int32, device=device), 10)
    with pytest.raises(ValueError):
        evaluation.sample_mesh(torch.tensor(vertices, device=device), torch.tensor(faces, device=device), -1)
    pts, face = run_mesh(device, vertices, faces, 1000, seed=1)                 # the device is fine
    assert np.array_equal(face, cloud_ref.sample_mesh(vertices, faces, 1000, seed=1)[1])


# ---- end to end ------------------------------------------------------------------------------------------------------
SETTINGS = dict(down_sample_res=0.25, threshold=0.28125, truncation_acc=0.34375, truncation_com=0.40625, mesh_sample_point=20000, seed=9)
KEYS = ["MAE_accuracy (cm)", "MAE_completeness (cm)", "Chamfer_L1 (cm)", "Precision [Accuracy] (%)", "Recall [Completeness] (%)",
        "F-score (%)", "Inlier_threshold (m)", "Outlier_truncation_acc (m)", "Outlier_truncation_com (m)"]


@functools.lru_cache(maxsize=None)
def scene():
    """The grid mesh and a lattice reference cloud 0.25 above its plane: longer than the mesh along x (reference points
    without an estimate), shorter along y (faces outside the reference's bounding box)."""
    rng = np.random.default_rng(41)
    vertices, faces, _ = cloud_ref.grid_mesh()
    reference = np.stack([rng.integers(-64, 97, 3000) / 16.0, rng.integers(-48, 65, 3000) / 16.0, np.full(3000, 0.25)], 1)
    return reference.astype(np.float32), vertices, faces


@functools.lru_cache(maxsize=None)
def numpy_chain(crop):
    reference, vertices, faces = scene()
    return cloud_ref.evaluate_recon(reference, vertices, faces, nn_ref, crop_to_reference=crop, **SETTINGS)


@pytest.mark.parametrize("crop", [False, True])
def test_evaluate_recon(device, crop, monkeypatch):
    reference, vertices, faces = scene()
    r, v, f = (torch.tensor(a, device=device) for a in (reference, vertices, faces))
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    got = evaluation.evaluate_recon(r, v, f, crop_to_reference=crop, **SETTINGS)
    monkeypatch.undo()
    print(f"host reads: {reads}")
    assert len(reads) <= 2
    assert list(got) == KEYS
    # the composition of the public pieces: the same kernels on the same input, the same bits
    box = None
    if crop:
        box = np.concatenate([reference.min(0) - np.float32([0, 0, 0.25]), reference.max(0) + np.float32([0, 0, 0.25])])
    sampled = evaluation.sample_mesh(v, f, SETTINGS["mesh_sample_point"], seed=SETTINGS["seed"], crop_box=box)
    m = evaluation.cloud_metrics(evaluation.voxel_down_sample(r, 0.25), evaluation.voxel_down_sample(sampled, 0.25),
                                 threshold=SETTINGS["threshold"], truncation_acc=SETTINGS["truncation_acc"],
                                 truncation_com=SETTINGS["truncation_com"])
    assert got == {
        "MAE_accuracy (cm)": m["accuracy_m"] * 100, "MAE_completeness (cm)": m["completeness_m"] * 100,
        "Chamfer_L1 (cm)": m["chamfer_l1_m"] * 100, "Precision [Accuracy] (%)": m["precision"] * 100.0,
        "Recall [Completeness] (%)": m["recall"] * 100.0, "F-score (%)": m["fscore"] * 100.0,
        "Inlier_threshold (m)": SETTINGS["threshold"], "Outlier_truncation_acc (m)": SETTINGS["truncation_acc"],
        "Outlier_truncation_com (m)": SETTINGS["truncation_com"]}
    # the all-NumPy chain: precision and recall are ratios of integers (exact), the means are sums of float32 roots
    want = numpy_chain(crop)
    print({k: (got[k], want[k]) for k in KEYS[:6]})
    assert 0 < want["Precision [Accuracy] (%)"] <= 100 and 0 < want["Recall [Completeness] (%)"] < 100
    for k in KEYS:
        if k in ("Precision [Accuracy] (%)", "Recall [Completeness] (%)") or k.endswith("(m)"):
            assert got[k] == want[k], k
        else:
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), k
    assert numpy_chain(True) != numpy_chain(False)                             # the crop is not a no-op here
    # down_sample_res <= 0 skips the down-sampling, as the reference does
    raw = evaluation.evaluate_recon(r, v, f, **{**SETTINGS, "down_sample_res": 0.0, "mesh_sample_point": 3000})
    m = evaluation.cloud_metrics(r, evaluation.sample_mesh(v, f, 3000, seed=SETTINGS["seed"]), threshold=SETTINGS["threshold"],
                                 truncation_acc=SETTINGS["truncation_acc"], truncation_com=SETTINGS["truncation_com"])
    assert raw["MAE_accuracy (cm)"] == m["accuracy_m"] * 100 and raw["Recall [Completeness] (%)"] == m["recall"] * 100.0


def write_mesh_ply(path, vertices, faces):
    header = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(vertices)}\nproperty float x\nproperty float y\n" \
             f"property float z\nelement face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n"
    rec = np.empty(len(faces), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, faces
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii") + np.asarray(vertices, "<f4").tobytes() + rec.tobytes())


def test_eval_recon_tool(device, tmp_path):
    reference, vertices, faces = scene()
    ply_io.save_point_cloud(tmp_path / "reference.ply", reference, np.zeros_like(reference))
    write_mesh_ply(tmp_path / "mesh.ply", vertices, faces)
    v2, f2 = ply_io.load_mesh(tmp_path / "mesh.ply")
    assert np.array_equal(v2, vertices) and np.array_equal(f2, faces)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_recon.py"), str(tmp_path / "reference.ply"),
                          str(tmp_path / "mesh.ply"), "--down-sample-res", "0.25", "--threshold", "0.28125", "--truncation-acc",
                          "0.34375", "--truncation-com", "0.40625", "--mesh-sample-point", "20000", "--seed", "9"],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out.strip().splitlines()[-1])
    want = evaluation.evaluate_recon(*(torch.tensor(a, device=device) for a in (reference, vertices, faces)), **SETTINGS)
    assert got == want                              # the same kernels on the same input: the same bits
    # eval_cloud.py --voxel: the same down-sampling in front of the two-cloud metrics
    sampled = evaluation.sample_mesh(torch.tensor(vertices, device=device), torch.tensor(faces, device=device), 20000, seed=9)
    ply_io.save_point_cloud(tmp_path / "estimate.ply", sampled, torch.zeros_like(sampled))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_cloud.py"), str(tmp_path / "reference.ply"),
                          str(tmp_path / "estimate.ply"), "--voxel", "0.25", "--threshold", "0.28125", "--truncation-acc", "0.34375",
                          "--truncation-com", "0.40625"], check=True, capture_output=True, text=True, timeout=300).stdout
    cloud = json.loads(out.strip().splitlines()[-1])
    assert cloud["accuracy_m"] * 100 == want["MAE_accuracy (cm)"] and cloud["recall"] * 100.0 == want["Recall [Completeness] (%)"]
