"""sls_surface_samples / meshing.sample_keyframe / meshing.sample_surface on the GPU against the NumPy restatement
(tests/surface_ref.py): the valid count and the selected pixels without tolerance, points and normals within 1e-5 of
scale of float64 (floats <= 1e-5 of scale)."""
import functools

import numpy as np
import pytest
import torch

import surface_ref as ref
from splat_loam_amd import meshing, ply_io, synth, traj_io
from splat_loam_amd.scene import Camera, SurfelModel

pytestmark = pytest.mark.gpu

SEED = 0x123456789ABCDEF
FRAME = 17
MIN_OPACITY, MAX_DIST = 0.5, 0.1


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    t = np.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


WORLD_T_MODEL = np.eye(4)
WORLD_T_MODEL[:3, :3] = _rot([0.3, -0.5, 0.8], 37.0)
WORLD_T_MODEL[:3, 3] = [80.0, -60.0, 5.0]                   # 100 m of translation
POSE = synth.keyframe_poses(4)[3]


@functools.lru_cache(maxsize=None)
def _planes(H, W):
    """Seven random planes: alpha in [0, 1], dist in [0, 0.2], depths 2 - 30 m, normals in [-1, 1]^3.  Read-only."""
    rng = np.random.default_rng(H * 10007 + W)
    am = np.empty((7, H, W), np.float32)
    am[1] = rng.uniform(0.0, 1.0, (H, W))
    am[0] = rng.uniform(2.0, 30.0, (H, W)) * am[1]           # the alpha-weighted depth
    am[2:5] = rng.uniform(-1.0, 1.0, (3, H, W))
    am[5] = rng.uniform(2.0, 30.0, (H, W))
    am[6] = rng.uniform(0.0, 0.2, (H, W))
    am.setflags(write=False)
    return am


def _camera(H, W, device):
    z = np.zeros((1, H, W), np.float32)
    return Camera(synth.spherical_K(H, W), z, None, None, POSE, data_device=device)


def _view32():
    return np.linalg.inv(POSE).astype(np.float32)            # as scene.Camera rounds it


def _run(am, device, k, **kw):
    H, W = am.shape[1:]
    kw.setdefault("min_opacity", MIN_OPACITY)
    kw.setdefault("max_depth_dist", MAX_DIST)
    kw.setdefault("seed", SEED)
    kw.setdefault("frame_id", FRAME)
    pts, nrm, det = meshing.sample_keyframe(torch.from_numpy(np.array(am)).to(device), _camera(H, W, device), WORLD_T_MODEL,
                                            kf_samples=k, details=True, **kw)
    return pts.cpu().numpy(), nrm.cpu().numpy(), det["n_valid"], det["pixels"].cpu().numpy().astype(np.int64), det["status"]


def _check(am, got, k, use_median=False, min_opacity=MIN_OPACITY, max_dist=MAX_DIST, seed=SEED, frame=FRAME, floats=True):
    pts, nrm, n_valid, pix, status = got
    H, W = am.shape[1:]
    want_n, want_pix = ref.select_pixels(am, min_opacity, max_dist, k, seed, frame)
    print(f"{H}x{W} k={k}: n_valid {n_valid} (restatement {want_n})")
    assert n_valid == want_n
    assert list(status) == [want_n, k if want_n else 0, 0, 1]
    assert np.array_equal(pix, want_pix)                     # every sample, no tolerance
    if not floats or want_n == 0:
        return want_pix
    wp, wn = ref.points_normals(am, want_pix, synth.spherical_K(H, W), _view32(), WORLD_T_MODEL, 1.0 if use_median else 0.0)
    ep = np.abs(pts - wp).max() / np.abs(wp).max()
    en = np.abs(nrm - wn).max() / np.abs(wn).max()
    print(f"    points {ep:.2e} of scale {np.abs(wp).max():.1f}, normals {en:.2e} of scale {np.abs(wn).max():.2f}")
    assert ep <= 1e-5 and en <= 1e-5
    return want_pix


@pytest.mark.parametrize("use_median", [False, True])
@pytest.mark.parametrize("k", [1, 257, 5000])
@pytest.mark.parametrize("H,W", [(8, 64), (50, 333), (64, 1024)])
def test_synthetic_planes(device, H, W, k, use_median):
    am = _planes(H, W)
    _check(am, _run(am, device, k, use_median_depth=use_median), k, use_median)


def test_no_valid_pixel_writes_nothing(device):
    H, W, k = 50, 333, 300
    am = _planes(H, W).copy()
    am[1] = 0.25                                             # every alpha below min_opacity
    cam = _camera(H, W, device)
    pts = torch.full((k, 3), -7.0, device=device)
    nrm = torch.full((k, 3), -7.0, device=device)
    pix = torch.full((k,), -7, dtype=torch.int32, device=device)
    status = torch.full((4,), -7, dtype=torch.int32, device=device)
    out = meshing.sample_keyframe(torch.from_numpy(am).to(device), cam, WORLD_T_MODEL, kf_samples=k, min_opacity=MIN_OPACITY,
                                  max_depth_dist=MAX_DIST, seed=SEED, frame_id=FRAME, out=(pts, nrm, pix, status))
    assert out[0] is pts
    assert status.cpu().tolist() == [0, 0, 0, 1]
    assert bool((pts == -7.0).all()) and bool((nrm == -7.0).all()) and bool((pix == -7).all())
    p2, n2 = meshing.sample_keyframe(torch.from_numpy(am).to(device), cam, WORLD_T_MODEL, kf_samples=k, min_opacity=MIN_OPACITY,
                                     max_depth_dist=MAX_DIST)
    assert p2.shape == (0, 3) and n2.shape == (0, 3)


def test_one_valid_pixel_is_every_row(device):
    H, W, k = 50, 333, 300
    am = _planes(H, W).copy()
    am[6] = 0.15                                             # every dist above max_depth_dist ...
    am[6, -1, -1] = 0.01                                     # ... but the image's last pixel (in the partial last word)
    am[1, -1, -1] = 0.9
    got = _run(am, device, k)
    pix = _check(am, got, k)
    assert got[2] == 1 and (pix == H * W - 1).all()
    assert (got[0] == got[0][0]).all() and (got[1] == got[1][0]).all()


def test_all_pixels_valid_and_more_samples_than_pixels(device):
    H, W = 50, 333
    am = _planes(H, W).copy()
    am[1] = np.maximum(am[1], 0.6)
    am[6] = np.minimum(am[6], 0.05)
    got = _run(am, device, 5000)
    _check(am, got, 5000)
    assert got[2] == H * W
    # kf_samples > n_valid: with replacement — 41 valid pixels, 300 rows
    am2 = _planes(H, W).copy()
    am2[1] = 0.1
    am2.reshape(7, -1)[1, 400::401] = 0.8
    am2.reshape(7, -1)[6, 400::401] = 0.02
    got = _run(am2, device, 300)
    pix = _check(am2, got, 300)
    assert 1 < got[2] < 300 and len(np.unique(pix)) <= got[2]


def test_thresholds_equal_to_a_value_keep_the_pixel_and_nan_alpha_stays(device):
    H, W, k = 50, 333, 2000
    am = _planes(H, W).copy()
    a, d = np.float32(0.3125), np.float32(0.0625)
    am[1] = 0.1                                              # invalid by alpha everywhere ...
    am[6] = 0.5                                              # ... and by dist
    flat = am.reshape(7, -1)
    flat[1, 100], flat[6, 100] = a, d                        # both exactly at the thresholds: valid
    flat[1, 5000], flat[6, 5000] = a, np.nextafter(d, np.float32(1))       # dist one ulp above: invalid
    flat[1, 9000], flat[6, 9000] = np.nextafter(a, np.float32(0)), d       # alpha one ulp below: invalid
    flat[1, 12000], flat[6, 12000] = np.nan, d               # NaN alpha: neither comparison holds, valid
    got = _run(am, device, k, min_opacity=float(a), max_depth_dist=float(d))
    pix = _check(am, got, k, min_opacity=float(a), max_dist=float(d), floats=False)
    assert got[2] == 2 and set(np.unique(pix)) == {100, 12000}


def test_purity(device):
    H, W = 50, 333
    am = _planes(H, W)
    a = _run(am, device, 5000)
    b = _run(am, device, 5000)
    for x, y in zip(a[:2] + (a[3],), b[:2] + (b[3],)):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert not np.array_equal(_run(am, device, 5000, seed=SEED + 1)[3], a[3])
    assert not np.array_equal(_run(am, device, 5000, frame_id=FRAME + 1)[3], a[3])
    c = _run(am, device, 257)
    assert np.array_equal(c[3], a[3][:257])
    assert np.array_equal(c[0].view(np.uint32), a[0][:257].view(np.uint32))
    assert np.array_equal(c[1].view(np.uint32), a[1][:257].view(np.uint32))


# ---- end to end: a results directory -> the cloud ---------------------------------------------------------------------
H2, W2, K2 = 16, 256, 300


def _world_T_model(i):
    T = np.eye(4)
    T[:3, :3] = _rot([0.1 + i, 0.4, 1.0], 20.0 + 70.0 * i)
    T[:3, 3] = [30.0 * (i + 1), -20.0 * i, 2.0 + i]
    return T


def _write_results(d):
    K = synth.spherical_K(H2, W2)
    intr = [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])]
    poses = synth.keyframe_poses(6)
    models, frames = [], []
    for mi in range(2):
        sc = synth.make_scene(3000, H2, W2, seed=40 + mi, range_lo=2.0, range_hi=20.0, scale_lo=0.03, scale_hi=0.2, opac_lo=0.3)
        name = f"models/model_{mi}.ply"
        ply_io.save_ply(d / name, sc["means"], np.log(sc["opac"] / (1 - sc["opac"])), np.log(sc["scales"]), sc["rots"])
        ids = [3 * mi + j for j in range(3)]
        models.append({"id": mi, "world_T_model": _world_T_model(mi), "filename": name, "frame_ids": ids})
        frames += [{"id": i, "timestamp": 0.1 * i, "model_T_frame": poses[i], "projmatrix": intr, "model_id": mi} for i in ids]
    traj_io.write_graph(d / "graph.yaml", models, frames)
    with open(d / "cfg.yaml", "w") as f:
        f.write(f"preprocessing:\n  image_height: {H2}\n  image_width: {W2}\n")
    return models, frames


def _render(d, model, frame, device):
    """The keyframe's raw allmap, rendered by the test itself: renderer.render's rasterizer call with the full allmap."""
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    raw = ply_io.load_ply(d / model["filename"])
    gm = SurfelModel(*(np.array(raw[k]) for k in ("xyz", "scaling", "rotation", "opacity")), device=device)
    fx, fy, cx, cy = frame["projmatrix"]
    cam = Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32), np.zeros((1, H2, W2), np.float32), None, None,
                 np.asarray(frame["model_T_frame"], dtype=np.float64).reshape(4, 4), data_device=device)
    settings = GaussianRasterizationSettings(H2, W2, 1.0, cam.world_view_transform, cam.projection_matrix, lean_allmap=False)
    with torch.no_grad():
        _, allmap = GaussianRasterizer(raster_settings=settings)(means3D=gm.get_xyz, means2D=gm.get_xyz, opacities=gm.get_opacity,
                                                                 scales=gm.get_scaling, rotations=gm.get_rotation)
    return cam, allmap


def test_sample_surface_end_to_end(device, tmp_path):
    """A results directory (write_graph + save_ply: 2 models of 3000 surfels with 3 frames each, 16x256) through
    sample_surface.  The pixels are compared on an allmap the test renders itself: the forward is an ordered per-pixel blend
    without atomics and gave the same bits in both calls where this was measured (valid counts 4011 / 3863 / 3361 of 4096,
    every selected pixel equal), so no `allmap` entry in `details` is needed."""
    from splat_loam_amd.renderer import depth_to_points, postprocess
    models, frames = _write_results(tmp_path)
    pts, nrm, det = meshing.sample_surface(tmp_path, kf_interval=2, kf_samples=K2, seed=SEED, device=device, details=True)
    assert det["frame_ids"] == [1, 3, 5]                     # the reference's rule: counter across models, from 1
    assert det["kept"].all() and (det["n_valid"] > 0).all()
    assert pts.shape == (K2 * 3, 3) and nrm.shape == (K2 * 3, 3) and pts.dtype == torch.float32 and pts.device == device
    for i, fid in enumerate(det["frame_ids"]):
        model = models[frames[fid]["model_id"]]
        cam, allmap = _render(tmp_path, model, frames[fid], device)
        am = allmap.cpu().numpy()
        n_valid, pix = ref.select_pixels(am, 0.5, 0.1, K2, SEED, fid)
        print(f"frame {fid}: n_valid {det['n_valid'][i]} (restatement on the test's own render {n_valid})")
        assert int(det["n_valid"][i]) == n_valid and n_valid < H2 * W2          # (the filter does filter)
        assert np.array_equal(det["pixels"][i].cpu().numpy().astype(np.int64), pix)
        # torch float32: postprocess -> depth_to_points (model frame) -> world_T_model, the reference's composition
        pkg = postprocess(cam, allmap, 0.0)
        T = torch.tensor(np.asarray(model["world_T_model"]), dtype=torch.float32, device=device)
        sel = torch.from_numpy(pix).to(device)
        p_model = depth_to_points(cam, pkg["surf_depth"], True).reshape(3, -1)[:, sel].T
        want_p = p_model @ T[:3, :3].T + T[:3, 3]
        want_n = pkg["rend_normal"].reshape(3, -1)[:, sel].T @ T[:3, :3].T
        rows = slice(i * K2, (i + 1) * K2)
        ep = float((pts[rows] - want_p).abs().max() / want_p.abs().max())
        en = float((nrm[rows] - want_n).abs().max() / want_n.abs().max())
        print(f"    points {ep:.2e} of scale, normals {en:.2e} of scale")
        assert ep <= 2e-5 and en <= 2e-5
    pts2, nrm2 = meshing.sample_surface(tmp_path, kf_interval=2, kf_samples=K2, seed=SEED, device=device)
    assert torch.equal(pts, pts2) and torch.equal(nrm, nrm2)
    # an empty keyframe leaves whole: nothing passes a dist threshold below zero
    pts3, _, det3 = meshing.sample_surface(tmp_path, kf_interval=3, kf_samples=K2, seed=SEED, device=device, max_depth_dist=-1.0,
                                           details=True)
    assert det3["frame_ids"] == [2, 5] and pts3.shape == (0, 3) and not det3["kept"].any()
