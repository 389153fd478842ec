"""sls_ground_segment and its Python faces (splat_loam_amd/evaluation.py: segment_ground, ground_normals, projector.py:
DeviceProjector(ground=True), tools/cloud_ground.py) on the device against the NumPy restatement (ground_ref.py).

The rule is float64 with + - * / sqrt and floor alone, one fixed order of every sum (64 strided lanes, the xor butterfly) and
no contraction, and the order inside a bin is an integer sort — so labels, bin numbers, info, status and the words of the
planes compare with array_equal, and two runs give equal bits.  tests/test_ground_math.py holds the header compiled for the
host to the same restatement on the same clouds."""
import json
import os
import runpy
import subprocess
import sys

import numpy as np
import pytest
import torch

import ground_ref as ref
from splat_loam_amd import evaluation, ply_io, projector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run(device, pts, **kw):
    height = kw.pop("sensor_height", 1.723)
    out = evaluation.segment_ground(torch.tensor(pts, device=device).reshape(-1, 3), height, return_details=True, **kw)
    mask, bins, planes, info, status = (t.cpu().numpy() for t in out)
    return {"label": mask.astype(np.uint8), "bin": bins, "planes": planes, "info": info, "status": status.view(np.uint32)}


def check(device, pts, what, **kw):
    """One call against the restatement, everything bit for bit, and a second call against the first."""
    want = ref.segment(pts, **kw)
    got, again = run(device, pts, **dict(kw)), run(device, pts, **dict(kw))
    assert got["label"].shape == (len(pts),) and got["bin"].dtype == np.int32 and got["planes"].shape == (ref.BINS, 8)
    for key in ("label", "bin", "info", "status"):
        bad = np.flatnonzero(np.atleast_1d(got[key] != want[key]).reshape(len(got[key]), -1).any(1))
        assert bad.size == 0, f"{what}: {key} differ at {bad[:5]}: got {got[key][bad[:3]]}, want {want[key][bad[:3]]}"
        assert np.array_equal(got[key], again[key]), f"{what}: {key} differ between two runs"
    bad = np.flatnonzero((words(got["planes"]) != words(want["planes"])).any(1))
    assert bad.size == 0, f"{what}: planes differ in bins {bad[:5]}: got {got['planes'][bad[:2]]}, want {want['planes'][bad[:2]]}"
    assert np.array_equal(words(got["planes"]), words(again["planes"])), f"{what}: planes differ between two runs"
    return want


@pytest.mark.parametrize("M", ref.SMALL)
def test_small_clouds_bit_for_bit(device, M):
    want = check(device, ref.small_cloud(M), f"M={M}")
    assert (want["info"][:, 3] >= ref.DEGENERATE).any() == (M >= 10)        # a fitted bin from ten points on
    check(device, np.tile(np.array([[3.0, 0.5, -1.7]], np.float32), (M, 1)), f"M={M} identical")


def test_empty_cloud(device):
    got = run(device, np.zeros((0, 3), np.float32))
    assert got["status"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1] and got["label"].shape == (0,) and not got["planes"].any()
    assert evaluation.ground_normals(torch.zeros((0, 3), device=device)).shape == (0, 3)


def test_one_crowded_bin(device):
    want = check(device, ref.one_bin(), "one bin")
    assert (want["info"][:, 0] == 3000).sum() == 1 and want["status"][1] > 1000


def test_every_bin_occupied(device):
    pts = ref.all_bins()
    want = check(device, pts, "all bins")
    n, state = want["info"][:, 0], want["info"][:, 3]
    assert [int(n[b]) for b in (3, 40, 200, 400, 503, 100)] == [9, 10, 64, 65, 11, 0]
    assert state[3] == ref.FEW and state[100] == ref.EMPTY and (n > 0).sum() == ref.BINS - 1
    assert want["status"][2] == 24 and (want["bin"] < 0).sum() == 60
    # the tie rule: -0.0 before +0.0, equal z in row order — the restatement's order is the key's, and equal planes say
    # the device summed in it
    rows = np.flatnonzero((want["bin"] == 7) & (pts[:, 2] == 0))
    assert len(rows) == 6 and np.signbit(pts[rows, 2]).sum() == 3


def test_states_worked_by_hand(device):
    """The clouds of tests/test_ground_math.py that reach what no scan above does: the elevated branch of the bin test with
    both of its outcomes, the noise skip, NOT_UPRIGHT, FEW and DEGENERATE."""
    flat, rough = check(device, ref.elevated_patch("flat"), "elevated flat"), check(device, ref.elevated_patch("rough"), "elevated rough")
    k = int(flat["bin"][0])
    assert flat["planes"][k, 4] > -1.723 + 0.523 and flat["info"][k, 3] == ref.GROUND and flat["label"].all()
    assert rough["planes"][k, 4] > -1.723 + 0.523 and rough["info"][k, 3] == ref.ELEVATED_ROUGH and not rough["label"].any()
    assert check(device, ref.elevated_patch("low"), "rough at ground level")["info"][k, 3] == ref.GROUND
    mid = check(device, ref.elevated_patch("ring1"), "elevated ring 1")
    k1 = int(mid["bin"][0])
    assert ref.place(k1)[1] == 1 and mid["info"][k1, 3] == ref.GROUND       # rough by ring 0's bound, flat by ring 1's
    near, far = check(device, ref.noise_patch(5.0), "noise zone 0"), check(device, ref.noise_patch(13.0), "noise zone 1")
    kn, kf = int(near["bin"][0]), int(far["bin"][0])
    assert near["info"][kn].tolist() == [300, 288, 300, ref.GROUND]         # 12 skipped: skip > 0
    assert far["info"][kf].tolist() == [300, 12, 12, ref.GROUND]            # zone 1 does not skip
    assert check(device, ref.noise_patch(5.0), "noise margin off", noise_margin=5.0)["info"][kn].tolist() == [300, 12, 12, ref.GROUND]
    wall = check(device, ref.wall(), "wall")
    assert (wall["info"][:, 3] == ref.NOT_UPRIGHT).sum() >= 2 and wall["status"][1] == 0
    ten = ref.ten_points()
    kt = int(ref.bins(ten, ref.params())[0])
    assert check(device, ten[:9], "nine")["info"][kt, 3] == ref.FEW and check(device, ten, "ten")["info"][kt, 3] == ref.GROUND
    assert check(device, np.tile(ten[:1], (10, 1)), "ten identical")["info"][kt].tolist() == [10, 10, 10, ref.DEGENERATE]


@pytest.mark.parametrize("kw", ref.VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters(device, kw):
    check(device, ref.bumpy(4000, 9), str(kw), **kw)


def test_street_scan(device):
    pts, truth = ref.street_scan()
    want = check(device, pts, "street")
    assert len(pts) == 64 * 1024 and want["status"][1] > 30000
    normals = evaluation.ground_normals(torch.tensor(pts, device=device)).cpu().numpy()
    assert np.array_equal(words(normals), words(ref.normals(pts, want)))
    g = want["label"] != 0
    assert np.all(normals[~g] == 0) and np.all(normals[g, 2] >= np.float32(0.707))
    assert np.all(np.abs(np.linalg.norm(normals[g].astype(np.float64), axis=1) - 1) < 1e-6)
    mask = evaluation.segment_ground(torch.tensor(pts, device=device))
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), g)


def test_device_projector_ground(device):
    H, W, lo, hi = 32, 512, 0.5, 100.0
    cloud, _ = ref.street(H, W, seed=2)
    cd = torch.tensor(cloud, device=device)
    for kw, gkw in (({}, {}), ({"normals": "pca", "normal_radius": 0.5, "normal_max_nn": 20},
                               {"sensor_height": 1.7, "ground_params": {"max_range": 60.0, "num_iter": 2}})):
        plain = projector.DeviceProjector(H, W, lo, hi, device=device, **kw).scan_to_images(cd)
        got = projector.DeviceProjector(H, W, lo, hi, device=device, ground=True, **kw, **gkw).scan_to_images(cd)
        assert "ground" not in plain and set(got) == set(plain) | {"ground"}
        for key in ("lut", "range_image", "valid", "K"):
            assert torch.equal(got[key], plain[key]), key                   # bit for bit
        want = ref.segment(cloud, sensor_height=gkw.get("sensor_height", 1.723), **gkw.get("ground_params", {}))
        lut = got["lut"].cpu().numpy()
        valid = lut >= 0
        assert 0.5 < valid.mean()
        ground = valid & (want["label"][np.maximum(lut, 0)] != 0)
        assert got["ground"].dtype == torch.bool and np.array_equal(got["ground"].cpu().numpy(), ground)
        assert 0.2 < ground.mean() < 0.9
        img, before = got["normals_image"].cpu().numpy(), plain["normals_image"].cpu().numpy()
        assert img.shape == (H, W, 3) and img.dtype == np.float32
        assert np.array_equal(words(img[ground]), words(ref.normals(cloud, want)[lut[ground]]))
        assert np.array_equal(words(img[~ground]), words(before[~ground]))  # untouched elsewhere
        assert np.all(img[ground][:, 2] > 0.7)
        if not kw:                                                          # the radial default lies almost in the ground
            assert np.median(np.abs(before[ground][:, 2])) < 0.5


def test_cloud_ground_tool_round_trip(device, tmp_path):
    pts = ref.bumpy(4000, 9)
    ply_io.save_point_cloud(tmp_path / "in.ply", pts, np.zeros_like(pts))
    tool = [sys.executable, os.path.join(ROOT, "tools", "cloud_ground.py"), str(tmp_path / "in.ply")]
    out = subprocess.run(tool + [str(tmp_path / "out.ply"), "--sensor-height", "1.5", "--max-range", "50", "--min-range", "1"],
                         check=True, capture_output=True, text=True, timeout=300)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    want = ref.segment(pts, sensor_height=1.5, max_range=50.0, min_range=1.0)
    got_p, got_n = ply_io.load_point_cloud(tmp_path / "out.ply")
    assert np.array_equal(words(got_p), words(pts)) and np.array_equal(words(got_n), words(ref.normals(pts, want)))
    assert line["points"] == 4000 and line["ground"] == int(want["status"][1]) and line["with_bin"] == int(want["status"][0])
    assert line["bins"]["GROUND"] == int(want["status"][3])
    # --split, in this process (the tool's own main, its arguments in sys.argv)
    argv = sys.argv
    sys.argv = tool[1:] + [str(tmp_path / "split.ply"), "--sensor-height", "1.5", "--max-range", "50", "--min-range", "1", "--split",
                           "--device", str(device)]
    try:
        runpy.run_path(tool[1], run_name="__main__")
    finally:
        sys.argv = argv
    g = want["label"] != 0
    a_p, a_n = ply_io.load_point_cloud(tmp_path / "split.ply")
    b_p, b_n = ply_io.load_point_cloud(tmp_path / "split_rest.ply")
    assert np.array_equal(words(a_p), words(pts[g])) and np.array_equal(words(a_n), words(ref.normals(pts, want)[g]))
    assert np.array_equal(words(b_p), words(pts[~g])) and not b_n.any()
