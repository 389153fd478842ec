"""The seeded densify draw on the device (sls_densify_draw; DESIGN.md section 2, "The densify draw") against its NumPy
restatement (tests/densify_draw_ref.py).  The reference consumes the weight bits the device wrote, so the drawn pixel
lists are compared WITHOUT tolerance and without an excluded pixel."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import densify_draw_ref as ref
from splat_loam_amd import fused_mapper, slam_rules, synth
from splat_loam_amd.scene import Camera, SurfelModel

pytestmark = pytest.mark.gpu

SEED, INDEX = 0x1234_5678_9ABC_DEF0, 3


def _camera(H, W, dev, seed=0, n_surfels=None, invalid=0.05, pose=None):
    """A synth keyframe (some pixels invalid), a model that covers part of it, and the alpha that model renders."""
    from splat_loam_amd.renderer import depth_to_points, render
    n = n_surfels or max(2000, (H * W) // 6)
    sc = synth.make_scene(n, H, W, seed=seed, range_lo=2.0, range_hi=30.0)
    depth, valid = synth.make_targets(H, W, sc)
    valid = valid.copy()
    valid[0][np.random.default_rng(seed + 1).random((H, W)) < invalid] = 0
    pose = np.eye(4) if pose is None else pose
    cam = Camera(sc["K"], depth, None, valid, pose, data_device=dev)
    pts = depth_to_points(cam, cam.image_depth)
    cam.image_normal = (-pts / pts.norm(dim=0, keepdim=True).clamp_min(1e-9)).contiguous()
    model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=dev)
    model.training_setup(fused=True)
    with torch.no_grad():
        alpha = render(cam, model, 0.0)["rend_alpha"].clone()
    frame = SimpleNamespace(camera=cam, model_T_frame=torch.tensor(pose, dtype=torch.float32, device=dev))
    return cam, frame, model, alpha


def _draw(cam, alpha, pct, seed=SEED, index=INDEX, thr=0.5):
    pixels, n_cand, det = fused_mapper._densify_draw_device(cam, alpha, thr, pct, seed, index, details=True)
    return (None if pixels is None else pixels.cpu().numpy()), n_cand, det["weights"].cpu().numpy(), det["stats"]


def _reference(w, stats, pct, seed=SEED, index=INDEX):
    gmax, total = (float(v) for v in stats[1:3].view(np.float32))
    return ref.draw(w, pct, seed, index, n_cand=int(stats[0]), gmax=gmax, total=total)


def _weights_call(cam, alpha, thr=0.5):
    """sls_densify_weights, as `_densify_draw_hip` calls it."""
    from splat_loam_amd import _abi
    from splat_loam_amd.fused import camera_aux
    H, W = int(cam.image_height), int(cam.image_width)
    dev = cam.image_depth.device
    aux = camera_aux(cam)
    w = torch.empty((H * W,), dtype=torch.float32, device=dev)
    stats = torch.empty((4,), dtype=torch.int32, device=dev)
    _abi.check(_abi.lib().sls_densify_weights(H, W, aux.gt.data_ptr(), aux.valid.data_ptr(),
                                              None if alpha is None else alpha.reshape(-1).float().contiguous().data_ptr(), thr,
                                              w.data_ptr(), stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "sls_densify_weights")
    return w.cpu().numpy(), stats.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("pct", [0.15, 0.3])
@pytest.mark.parametrize("H,W", [(64, 1024), (128, 1024), (64, 2048), (50, 333)])
def test_device_draw_equals_the_reference_bit_for_bit(device, H, W, pct):
    """Every size the reference's configs use and a ragged one, both percentages, with the alpha a model renders and with
    rend_alpha = NULL (a first keyframe): the device's pixel list IS the reference's for the device's own weight bits;
    n_cand and n_drawn = int(percentage * n_cand) equal; the list strictly ascending and of candidates only; the
    weights and the three statistics' integer word those of sls_densify_weights."""
    cam, _, _, alpha = _camera(H, W, str(device), seed=H + W)
    for a in (alpha, None):
        pix, n_cand, w, stats = _draw(cam, a, pct)
        cand = slam_rules.densify_candidates(cam.image_valid, alpha, None, cam.image_depth, 0.5, -1.0, a is None)
        assert n_cand == int(stats[0]) == int(cand.sum()) == int((w > 0).sum())
        assert np.array_equal(w > 0, cand.reshape(-1).cpu().numpy())
        w_old, stats_old = _weights_call(cam, a)
        assert np.array_equal(w.view(np.uint32), w_old.view(np.uint32))
        assert int(stats_old[0]) == n_cand and int(stats_old[1]) == int(stats[1])          # (the sum is a float-atomic sum)
        k = int(pct * n_cand)
        assert k >= 2 and int(stats[3]) == int(stats[4]) == k == pix.size and int(stats[7]) == 1
        want = _reference(w, stats, pct)
        assert want is not None and np.array_equal(pix, want), f"{int((np.setdiff1d(pix, want)).size)} pixels differ"
        assert pix.dtype == np.int64 and bool((np.diff(pix) > 0).all()) and bool((w[pix] > 0).all())
        keys = ref.keys(w, SEED, INDEX).view(np.uint32)
        assert int(stats[5]) == int(keys[pix].max()) and int(stats[6]) == int((keys[pix] == keys[pix].max()).sum())


def test_fallback_to_zero_gradient_candidates(device):
    """Structure confined to a small patch, so that k exceeds the number of positive-weight candidates: every one of those
    is drawn, the rest are zero-gradient candidates (weight 1e-30) — the reference's — and never a non-candidate."""
    H, W = 64, 1024
    rng = np.random.default_rng(3)
    depth = np.full((1, H, W), 10.0, np.float32)
    depth[0, 20:30, 100:140] = rng.uniform(5.0, 20.0, (10, 40)).astype(np.float32)
    valid = np.ones((1, H, W), np.uint8)
    valid[0][rng.random((H, W)) < 0.2] = 0
    cam = Camera(synth.spherical_K(H, W), depth, None, valid, np.eye(4), data_device=str(device))
    pix, n_cand, w, stats = _draw(cam, None, 0.15)
    positive = np.flatnonzero(w > np.float32(1.0e-30))
    k = int(0.15 * n_cand)
    assert 0 < positive.size < k == pix.size
    assert np.isin(positive, pix).all()
    rest = np.setdiff1d(pix, positive)
    assert rest.size == k - positive.size and bool((w[rest] == np.float32(1.0e-30)).all())
    assert bool((valid.reshape(-1)[pix] == 1).all())
    assert np.array_equal(pix, _reference(w, stats, 0.15))


def test_no_draw_cases(device):
    """k < 2, a flat range image (the gradient's maximum is 0) and weight mass below the 1e-5 rule: n_drawn = 0 where
    `_densify_draw_hip` (today's rules) draws nothing and, for the first and third, `slam_rules.densify_sample` returns None
    (on a flat image the torch form divides 0 by 0 before it tests the sum: the rule `not gmax > 0` is the HIP path's)."""
    H, W = 64, 1024
    dev = str(device)
    K = synth.spherical_K(H, W)
    rng = np.random.default_rng(4)
    textured = rng.uniform(5.0, 20.0, (1, H, W)).astype(np.float32)
    few = np.zeros((1, H, W), np.uint8)
    few[0, 10, 10:15] = 1
    flat = np.full((1, H, W), 7.0, np.float32)
    patch = flat.copy()
    patch[0, 30:33, 500:503] = rng.uniform(5.0, 20.0, (3, 3)).astype(np.float32)
    alpha = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
    alpha[0, 27:36, 497:506] = 1.0                      # the structure and everything its differences reach: no candidates
    ones = np.ones((1, H, W), np.uint8)
    for name, depth, valid, a, sample_rule in (("k < 2", textured, few, None, True), ("flat", flat, ones, None, False),
                                                ("no mass", patch, ones, alpha, True)):
        cam = Camera(K, depth, None, valid, np.eye(4), data_device=dev)
        pix, n_cand, w, stats = _draw(cam, a, 0.15)
        gmax, total = (float(v) for v in stats[1:3].view(np.float32))
        assert pix is None and int(stats[3]) == 0 and int(stats[7]) == 1, name
        assert int(stats[4]) == int(0.15 * n_cand), name
        assert _reference(w, stats, 0.15) is None, name
        assert fused_mapper._densify_draw_hip(cam, a, 0.5, 0.15)[0] is None, name
        if sample_rule:
            cand = slam_rules.densify_candidates(cam.image_valid, a, None, cam.image_depth, 0.5, -1.0, a is None)
            assert slam_rules.densify_sample(cand, cam.image_depth, cam.image_valid, 0.15) is None, name
        if name == "k < 2":
            assert n_cand == 5
        elif name == "flat":
            assert n_cand == H * W and gmax == 0.0
        else:
            assert gmax > 0.0 and total / gmax <= 1e-5 and int(0.15 * n_cand) >= 2


def test_same_seed_same_bits_other_seed_other_set(device):
    cam, _, _, alpha = _camera(64, 1024, str(device), seed=9)
    first, _, w, _ = _draw(cam, alpha, 0.15)
    again, _, w2, _ = _draw(cam, alpha, 0.15)
    assert np.array_equal(first, again) and np.array_equal(w.view(np.uint32), w2.view(np.uint32))
    fused_mapper._DRAW_BUFFERS.clear()                   # fresh status words, mirror and scratch
    fresh, _, _, _ = _draw(cam, alpha, 0.15)
    assert np.array_equal(first, fresh)
    for seed, index in ((SEED, INDEX + 1), (SEED + 1, INDEX), (SEED ^ (1 << 40), INDEX)):
        other, _, _, _ = _draw(cam, alpha, 0.15, seed=seed, index=index)
        assert other.size == first.size and not np.array_equal(other, first)
        assert np.intersect1d(other, first).size < 0.9 * first.size


def _cfg(num_iterations=3, egeom=-1.0):
    mapping = SimpleNamespace(num_iterations=num_iterations, densify_threshold_egeom=egeom, densify_threshold_opacity=0.5,
                              densify_percentage=0.15, prob_view_last_keyframe=0.4, pruning_min_opacity=0.0, pruning_min_size=0.0,
                              opt_lambda_alpha=0.1, opt_lambda_normal=0.1, opt_scaling_max=0.5, opt_scaling_max_penalty=0.2)
    return SimpleNamespace(mapping=mapping, opt=SimpleNamespace(depth_ratio=0.0))


def _params(model):
    return [getattr(model, a).detach().clone() for a in ("_xyz", "_opacity", "_scaling", "_rotation")]


def test_update_model_with_the_device_draw(device, monkeypatch):
    """update_model(draw="device", seed, draw_index): added == n_drawn; the appended centres and quaternions are, bit for
    bit, `_densify_rows_hip` on the MASK of the reference's set; a second model under the same seed and index and
    SLS_DETERMINISTIC=1 ends the keyframe with identical parameters; the result names the seed and index used, and the
    model's own counter advances only where no index was passed."""
    monkeypatch.setenv("SLS_DETERMINISTIC", "1")
    dev = str(device)
    H, W = 64, 1024
    pose = synth.keyframe_poses(2)[1]
    cfg = _cfg()
    seen = {}
    inner = fused_mapper.fused_optimize

    def spy(gmodel, *args, **kwargs):                    # the model as densify left it, before the iterations move it
        seen["xyz"], seen["rot"] = gmodel._xyz.detach().clone(), gmodel._rotation.detach().clone()
        return inner(gmodel, *args, **kwargs)
    monkeypatch.setattr(fused_mapper, "fused_optimize", spy)
    finals = []
    for run in range(2):
        cam, frame, model, alpha = _camera(H, W, dev, seed=21, pose=pose)
        n_old = int(model._xyz.shape[0])
        pix, n_cand, w, stats = _draw(cam, alpha, 0.15, seed=77, index=5)
        want = _reference(w, stats, 0.15, seed=77, index=5)
        mask = torch.zeros((H * W,), dtype=torch.bool, device=dev)
        mask[torch.tensor(want, device=dev)] = True
        xyz, quat = fused_mapper._densify_rows_hip(frame, mask.view(H, W))
        res = fused_mapper.update_model(model, [frame], frame, cfg, draw="device", seed=77, draw_index=5,
                                        rng=np.random.default_rng(0))
        assert res["added"] == int(stats[3]) == want.size and res["draw"] == "device"
        assert (res["seed"], res["draw_index"]) == (77, 5) and res["candidates"] is None
        assert not hasattr(model, fused_mapper._DRAW_INDEX_ATTR)
        assert int(seen["xyz"].shape[0]) == n_old + want.size
        assert torch.equal(seen["xyz"][n_old:], xyz) and torch.equal(seen["rot"][n_old:], quat)
        finals.append(_params(model))
    for a, b in zip(*finals):
        assert torch.equal(a, b)
    # the defaults: torch.initial_seed() and the model's counter
    torch.manual_seed(4242)
    r0 = fused_mapper.update_model(model, [frame], frame, cfg, draw="device", rng=np.random.default_rng(0))
    r1 = fused_mapper.update_model(model, [frame], frame, cfg, draw="device", rng=np.random.default_rng(0))
    assert (r0["seed"], r0["draw_index"], r1["seed"], r1["draw_index"]) == (4242, 0, 4242, 1)
    assert getattr(model, fused_mapper._DRAW_INDEX_ATTR) == 2


def test_torch_draw_stays_torchs_and_the_switch(device, monkeypatch):
    """draw="torch" (the default) with a generator takes today's path — sls_densify_draw is not called, SLS_DEVICE_DRAW=1
    or not; the switch turns the device draw on only for a caller who passed neither `drawn` nor `generator`; what the
    device draw does not serve raises."""
    dev = str(device)
    cam, frame, model, _ = _camera(64, 1024, dev, seed=22)
    cfg = _cfg(num_iterations=1)
    calls = []
    inner = fused_mapper._densify_draw_device

    def counted(*args, **kwargs):
        calls.append(1)
        return inner(*args, **kwargs)
    monkeypatch.setattr(fused_mapper, "_densify_draw_device", counted)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    for env in ("0", "1"):
        monkeypatch.setenv("SLS_DEVICE_DRAW", env)
        res = fused_mapper.update_model(model, [frame], frame, cfg, generator=gen, rng=np.random.default_rng(0))
        assert res["draw"] == "torch" and res["seed"] is None and res["draw_index"] is None and res["added"] > 0
        res = fused_mapper.update_model(model, [frame], frame, cfg, draw="torch", rng=np.random.default_rng(0))
        assert res["draw"] == "torch" and not calls
    res = fused_mapper.update_model(model, [frame], frame, cfg, rng=np.random.default_rng(0))         # SLS_DEVICE_DRAW=1
    assert res["draw"] == "device" and len(calls) == 1 and res["draw_index"] == 0 and res["added"] > 0
    monkeypatch.setenv("SLS_DEVICE_DRAW", "0")
    with pytest.raises(RuntimeError, match="densify_threshold_egeom"):
        fused_mapper.update_model(model, [frame], frame, _cfg(egeom=0.5), draw="device")
    with pytest.raises(ValueError, match="generator"):
        fused_mapper.update_model(model, [frame], frame, cfg, draw="device", generator=gen)
    # a pixel list and its mask append the same rows
    pix, _ = inner(cam, None, 0.5, 0.15, 1, 0)
    mask = torch.zeros((64 * 1024,), dtype=torch.bool, device=dev)
    mask[pix] = True
    a = fused_mapper._densify_rows_hip(frame, pix)
    b = fused_mapper._densify_rows_hip(frame, mask.view(64, 1024))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_an_image_beyond_the_cap_raises(device):
    """More than 2^18 pixels: SLS_E_UNSUPPORTED from the library, an exception in Python — never a silent torch draw."""
    H, W = 257, 1024
    cam = Camera(synth.spherical_K(H, W), np.full((1, H, W), 5.0, np.float32), None, np.ones((1, H, W), np.uint8), np.eye(4),
                 data_device=str(device))
    with pytest.raises(RuntimeError, match="code -4"):
        fused_mapper._densify_draw_device(cam, None, 0.5, 0.15, 1, 0)
