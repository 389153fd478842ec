"""The pose gradient on the GPU: dL/dxi for the left perturbation T_vw -> Exp(xi) T_vw, reduced
inside the projection's backward.

Reference: the functional of tests/pose_ref.py applied to the FLOAT64 checker's surfel gradients (pinned on the CPU by
tests/test_pose_math.py against autograd through the rigid motion and against finite differences over the camera).
g is a cancelling sum, so the bar is the project's RTOL = 1e-5 applied per component to S_k = sum_i |term_i,k|, computed
here from the float64 reference: |g_hip - g_ref|_k <= 1e-5 S_k.  The float32 checker's own functional stays within
8.1e-7 S_k of the float64 one on these scenes (1.9e-6 S_k on the checker chain at 50 000 surfels).  No pixel or surfel
is excluded except where a test says so.  Every figure is printed before it is asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_ref
import test_timed_path as ttp
from helpers import RTOL, hip_forward, tangent

pytestmark = pytest.mark.gpu


def _threads(o):
    o.set_threads(min(16, o.max_threads()))


def _settings(device, view, proj, H, W, **kw):
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device), **kw)


def _render_with_pose(device, settings, sc, dL, with_pose=True):
    """One forward + backward through GaussianRasterizer; returns (radii, allmap, surfel gradients, pose gradient)."""
    from splat_loam_amd.rasterizer import GaussianRasterizer
    t = {k: torch.tensor(sc[k], device=device).requires_grad_(True) for k in ("means", "scales", "rots", "opac")}
    xi = torch.zeros(6, dtype=torch.float32, device=device, requires_grad=True) if with_pose else None
    extra = {"pose_delta": xi} if with_pose else {}
    radii, am = GaussianRasterizer(raster_settings=settings)(means3D=t["means"], means2D=t["means"], opacities=t["opac"],
                                                            scales=t["scales"], rotations=t["rots"], **extra)
    (am * torch.tensor(dL, device=device)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().numpy().copy() for k, v in t.items()}
    return radii.cpu().numpy(), am.detach().cpu().numpy(), grads, (xi.grad.cpu().numpy().copy() if with_pose else None)


def _checker_pose_gradient(oracle64, sc, view, proj, H, W, dL):
    _threads(oracle64)
    cam = oracle64.camera(H, W, np.asarray(view, np.float64), proj)
    a64 = [np.asarray(sc[k], np.float64) for k in ("means", "scales", "rots", "opac")]
    st = oracle64.forward(cam, *a64)
    bw = oracle64.backward(st, np.asarray(dL, np.float64), threads=min(16, oracle64.max_threads()), want_abs=False)
    return pose_ref.functional(view, a64[0], a64[2], bw["dmeans"], bw["drots"]), cam


SCENES = [(2000, 64, 512, 1), (6000, 64, 1024, 3), (50000, 64, 1024, 2)]


@pytest.mark.parametrize("hfov", [360.0, 120.0], ids=["360", "120"])
@pytest.mark.parametrize("N,H,W,pose_k", SCENES, ids=["2000-64x512", "6000-64x1024", "50000-64x1024"])
def test_pose_delta_grad_matches_the_float64_functional(device, oracle64, monkeypatch, N, H, W, pose_k, hfov):
    """Drop-in path, workspace AND staged calls: pose_delta.grad against the functional of the float64 checker's gradients
    for the same dL/dallmap (planes 5 and 6 zero).  Bar: 1e-5 S_k per component."""
    from splat_loam_amd import rasterizer, synth
    sc = synth.make_scene(N, H, W, seed=0)
    if hfov != 360.0:
        sc["K"] = synth.spherical_K(H, W, hfov_deg=hfov)
    view, proj = synth.camera_matrices(sc["K"], synth.keyframe_poses(4)[pose_k])
    dL = np.random.default_rng(7).normal(size=(7, H, W)).astype(np.float32)
    dL[5:] = 0
    (g_ref, S), cam = _checker_pose_gradient(oracle64, sc, view, proj, H, W, dL)
    assert cam.wrap == (1 if hfov == 360.0 else 0)
    print(f"\n[{N}@{H}x{W} hfov {hfov:.0f}] g_ref {g_ref}\n    S {S}  (S / |g|: {S / np.abs(g_ref)})")
    worst = {}
    for staged in ("0", "1"):
        monkeypatch.setenv("SLS_STAGED_FORWARD", staged)
        rasterizer._WS_CACHE.clear()
        _, _, _, g = _render_with_pose(device, _settings(device, view, proj, H, W), sc, dL)
        e = pose_ref.in_units_of_S(g, g_ref, S)
        worst[staged] = e
        print(f"    {'staged' if staged == '1' else 'workspace'} path: |g - g_ref| / S = {e}")
    for staged, e in worst.items():
        assert (e <= RTOL).all(), (staged, e)


def test_pose_delta_grad_matches_autograd_through_the_float64_formulation(device, oracle64):
    """Against oracle/torch_ref.dense_forward_tiled — a float64 torch formulation that shares no arithmetic with the
    kernels — differentiated by autograd through the rigid motion of the surfels, on the scene and with the givens of
    test_hip_against_the_float64_autograd_formulation[seed21-2000-64x512] (integer decisions and centre pixels from the HIP
    forward's own buffers; dL/dallmap zero on the median plane and, as there, at the checker's fragile pixels).  Same bar."""
    from oracle import torch_ref
    from splat_loam_amd import synth
    from splat_loam_amd.rasterizer import rasterize_backward
    N, H, W, seed = 2000, 64, 512, 21
    sc = synth.make_scene(N, H, W, seed=seed, range_lo=2.0, range_hi=15.0, scale_lo=0.05, scale_hi=0.3)
    view, proj = synth.camera_matrices(sc["K"], np.eye(4))
    st, t = hip_forward(device, sc, view, proj, H, W)
    cam = oracle64.camera(H, W, view.astype(np.float64), proj)
    a64 = [np.asarray(sc[k], np.float64) for k in ("means", "scales", "rots", "opac")]
    ost = oracle64.forward(cam, *a64)
    pre_hip = {"rec": st.rec.cpu().numpy().astype(np.float64), "radii": st.radii.cpu().numpy(), "rect": st.rect.cpu().numpy(),
               "depth": st.depth.cpu().numpy()}
    xi, m1, q1 = pose_ref.rigid_motion_leaves(view, a64[0], a64[2])
    leaves = [torch.tensor(a, requires_grad=True) for a in a64]
    # (the surfels' own leaves ride along: S_k comes from THIS formulation's gradients)
    am64 = torch_ref.dense_forward_tiled(cam, ost["tables"], pre_hip, m1 + (leaves[0] - leaves[0].detach()), leaves[1],
                                         q1 + (leaves[2] - leaves[2].detach()), leaves[3])
    dL = np.random.default_rng(3).normal(size=(7, H, W))
    dL[5] = 0
    dL[:, ost["fwd"]["fragile"]] = 0
    (am64 * torch.tensor(dL)).sum().backward()
    g_ref = xi.grad.numpy()
    g_fun, S = pose_ref.functional(view, a64[0], a64[2], leaves[0].grad.numpy(), leaves[2].grad.numpy())
    print(f"\n[f64 autograd {N}@{H}x{W}] g_ref {g_ref}\n    functional of its own surfel gradients: {pose_ref.in_units_of_S(g_fun, g_ref, S)} S")
    assert (pose_ref.in_units_of_S(g_fun, g_ref, S) <= 1e-10).all()
    pg = torch.empty(6, dtype=torch.float32, device=device)
    rasterize_backward(st, t["means"], t["scales"], t["rots"], torch.tensor(dL.astype(np.float32), device=device), pose_grad=pg)
    torch.cuda.synchronize()
    e = pose_ref.in_units_of_S(pg.cpu().numpy(), g_ref, S)
    print(f"    HIP: |g - g_ref| / S = {e}")
    assert (e <= RTOL).all(), e


@pytest.mark.parametrize("staged", ["0", "1"], ids=["workspace", "staged"])
def test_a_call_with_pose_delta_returns_what_the_call_without_returns(device, monkeypatch, staged):
    """radii, allmap and the surfel gradients WITH pose_delta against the call without: bit for bit with the
    deterministic accumulation (staged calls; SLS_DETERMINISTIC=1 routes the workspace setting there too), within the
    float-atomic bar (5e-6 of the tensor's maximum, the bar of test_workspace_path_matches_staged_path) otherwise."""
    from splat_loam_amd import rasterizer, synth
    N, H, W = 6000, 64, 1024
    sc = synth.make_scene(N, H, W, seed=0)
    view, proj = synth.camera_matrices(sc["K"], synth.keyframe_poses(4)[3])
    dL = np.random.default_rng(7).normal(size=(7, H, W)).astype(np.float32)
    for det in ("1", "0"):
        monkeypatch.setenv("SLS_STAGED_FORWARD", staged)
        monkeypatch.setenv("SLS_DETERMINISTIC", det)
        rasterizer._WS_CACHE.clear()
        settings = _settings(device, view, proj, H, W)
        r0, a0, g0, _ = _render_with_pose(device, settings, sc, dL, with_pose=False)
        r1, a1, g1, pg = _render_with_pose(device, settings, sc, dL, with_pose=True)
        assert np.array_equal(r0, r1) and np.array_equal(a0, a1)
        assert np.isfinite(pg).all() and np.abs(pg).max() > 0
        for k in g0:
            if det == "1":
                assert np.array_equal(g0[k], g1[k]), k
            else:
                e = np.abs(g0[k] - g1[k]).max() / np.abs(g0[k]).max()
                print(f"\n[{'staged' if staged == '1' else 'workspace'}, float atomics] d{k}: {e:.2e}")
                assert e <= 5e-6, (k, e)


def test_pose_gradient_is_deterministic_where_the_records_are(device, monkeypatch):
    """SLS_DETERMINISTIC=1 (drop-in path) and engine deterministic = 1 and 2: two runs, identical bits of g; and a second
    walk of a retained graph returns the first walk's bits."""
    from splat_loam_amd import rasterizer, synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.rasterizer import GaussianRasterizer
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 50000, 64, 1024
    sc = synth.make_scene(N, H, W, seed=0)
    view, proj = synth.camera_matrices(sc["K"], synth.keyframe_poses(4)[2])
    dL = np.random.default_rng(7).normal(size=(7, H, W)).astype(np.float32)
    monkeypatch.setenv("SLS_DETERMINISTIC", "1")
    rasterizer._WS_CACHE.clear()
    settings = _settings(device, view, proj, H, W)
    runs = [_render_with_pose(device, settings, sc, dL)[3] for _ in range(2)]
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), runs
    # a retained graph, walked twice (the second walk repeats the forward through the staged calls)
    for det in ("1", "0"):
        monkeypatch.setenv("SLS_DETERMINISTIC", det)
        rasterizer._WS_CACHE.clear()
        t = {k: torch.tensor(sc[k], device=device).requires_grad_(True) for k in ("means", "scales", "rots", "opac")}
        xi = torch.zeros(6, dtype=torch.float32, device=device, requires_grad=True)
        _, am = GaussianRasterizer(raster_settings=settings)(means3D=t["means"], means2D=t["means"], opacities=t["opac"],
                                                            scales=t["scales"], rotations=t["rots"], pose_delta=xi)
        loss = (am * torch.tensor(dL, device=device)).sum()
        loss.backward(retain_graph=True)
        first = xi.grad.clone()
        xi.grad = None
        loss.backward()
        if det == "1":
            assert torch.equal(first, xi.grad) and np.array_equal(first.cpu().numpy().view(np.uint32), runs[0].view(np.uint32))
        else:
            assert float((first - xi.grad).abs().max()) <= 1e-4 * float(first.abs().max())
    monkeypatch.setenv("SLS_DETERMINISTIC", "0")
    # the engine: deterministic = 1 (two launches) and 2 (one launch with predicted scales, after a first two-launch one)
    _, raw, depth, valid = ttp._raw_scene(N, H, W, seed=23)
    pose = synth.keyframe_poses(2)[1]
    for det in (1, 2):
        got = []
        for _ in range(2):
            cam = Camera(sc["K"], depth, None, valid, pose, data_device=str(device))
            eng = MappingEngine(SurfelModel(raw["xyz"], raw["scaling"], raw["rotation"], raw["opacity"], device=str(device)), MappingConfig())
            eng.deterministic = det
            seq = []
            for _ in range(3):
                st = eng.pose_step(cam)
                assert not st["overflow"]
                seq.append(eng.pose_grad.cpu().numpy().copy())
            got.append(seq)
            # (the model is frozen: every iteration is the same function of the same inputs)
            assert np.array_equal(seq[0].view(np.uint32), seq[1].view(np.uint32)) or det == 2
        for a, b in zip(*got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (det, a, b)


def _engine_pose_case(device, name, N, H, W, kw):
    """pose_step and step(pose_grad=True) against the functional applied to the float64 checker chain's RAW gradients, in
    the same-allmap formulation (the consumer evaluated at the engine's image: both sides differentiate the same function)."""
    import oracle.torch_function as otf
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    sc, raw, depth, valid = ttp._raw_scene(N, H, W, seed=23, **kw)
    valid = valid.copy(); valid[0, :2, :9] = 0
    pose = synth.keyframe_poses(2)[1]
    view, proj = synth.camera_matrices(sc["K"], pose)
    cfg = MappingConfig()
    cam = Camera(sc["K"], depth, None, valid, pose, data_device=str(device))
    model = SurfelModel(raw["xyz"], raw["scaling"], raw["rotation"], raw["opacity"], device=str(device))
    eng = MappingEngine(model, cfg)
    before = [p.detach().clone() for p in (model._xyz, model._scaling, model._rotation, model._opacity)]
    st_p = eng.pose_step(cam)
    g_pose = eng.pose_grad.cpu().numpy().astype(np.float64)
    am = eng.allmap(H, W).cpu().numpy()
    # the model is frozen: parameters, moments and step count bit-identical
    for p, b in zip((model._xyz, model._scaling, model._rotation, model._opacity), before):
        assert torch.equal(p.detach(), b)
    assert eng.t == 0 and float(eng.exp_avg.abs().max()) == 0.0 and float(eng.exp_avg_sq.abs().max()) == 0.0
    st_s = eng.step(cam, pose_grad=True)
    g_step = eng.pose_grad.cpu().numpy().astype(np.float64)
    assert eng.t == 1 and not torch.equal(model._xyz.detach(), before[0])
    assert abs(st_p["loss"] - st_s["loss_pixel"]) <= 1e-6 * abs(st_s["loss_pixel"]) and st_p["loss_reg"] == 0.0
    nt = min(16, otf._oracle(np.float64).max_threads())
    for dt in (np.float32, np.float64):
        otf._oracle(dt).set_threads(nt)
    otf.BACKWARD_THREADS = nt
    try:
        same64 = ttp.reference_iteration(raw, sc["K"], view, proj, H, W, depth[0], valid[0] == 1, cfg, allmap_value=am, dtype=np.float64)
        own64 = ttp.reference_iteration(raw, sc["K"], view, proj, H, W, depth[0], valid[0] == 1, cfg, dtype=np.float64)
    finally:
        otf.BACKWARD_THREADS = 1
    g_same, S = pose_ref.functional(view, raw["xyz"], raw["rotation"], same64["grads"]["xyz"], same64["grads"]["rotation"])
    g_own, S_own = pose_ref.functional(view, raw["xyz"], raw["rotation"], own64["grads"]["xyz"], own64["grads"]["rotation"])
    out = {"same_pose_step": pose_ref.in_units_of_S(g_pose, g_same, S), "same_step": pose_ref.in_units_of_S(g_step, g_same, S),
           "own_pose_step": pose_ref.in_units_of_S(g_pose, g_own, S_own)}
    print(f"\n[{name}] g (float64 chain, same-allmap) {g_same}\n    S {S}")
    for k, v in out.items():
        print(f"    {k}: |g - g_ref| / S = {v}")
    return out


@pytest.mark.parametrize("name,N,H,W,kw", [("small", 6000, 32, 256, dict(range_lo=2.0, range_hi=15.0, scale_hi=0.25)),
                                           ("c2", 50000, 64, 1024, {})], ids=["small", "c2"])
def test_engine_pose_gradient_matches_the_checker_chain(device, name, N, H, W, kw):
    """Bar (same-allmap): 1e-5 S_k per component, for pose_step and for step(pose_grad=True).  The own-allmap figure (each
    side differentiates its own image) is printed and recorded (profiles/r11a_pose_grad.json), without a bar."""
    out = _engine_pose_case(device, name, N, H, W, kw)
    assert (out["same_pose_step"] <= RTOL).all(), out
    assert (out["same_step"] <= RTOL).all(), out


def test_step_batch_returns_each_keyframes_own_pose_gradient(device):
    """step_batch with G = 4: row g is what pose_step on keyframe g gives on the same model — bit for bit with the
    deterministic accumulation (same records, same rows, same order of the sum); within the float-atomic noise otherwise."""
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W, G = 6000, 32, 256, 4
    sc, raw, depth, valid = ttp._raw_scene(N, H, W, seed=23, range_lo=2.0, range_hi=15.0, scale_hi=0.25)
    for det in (1, 0):
        cams = [Camera(sc["K"], depth, None, valid, p, data_device=str(device)) for p in synth.keyframe_poses(G)]
        eng = MappingEngine(SurfelModel(raw["xyz"], raw["scaling"], raw["rotation"], raw["opacity"], device=str(device)), MappingConfig())
        eng.deterministic = det
        single = []
        for c in cams:
            eng.pose_step(c)
            single.append(eng.pose_grad.cpu().numpy().copy())
        st = eng.step_batch(cams, pose_grad=True)
        assert not st["overflow"] and tuple(eng.pose_grad.shape) == (G, 6)
        rows = eng.pose_grad.cpu().numpy()
        assert len({tuple(r) for r in rows}) == G, "every keyframe has its own camera: four different gradients"
        for g in range(G):
            if det:
                assert np.array_equal(rows[g].view(np.uint32), single[g].view(np.uint32)), (g, rows[g], single[g])
            else:
                assert np.abs(rows[g] - single[g]).max() <= 1e-4 * np.abs(single[g]).max(), (g, rows[g], single[g])
        # without the flag the attribute does not keep a stale gradient
        eng.step_batch(cams)
        assert eng.pose_grad is None


def test_pose_argument_errors(device):
    """Wrong shape / dtype / device of pose_delta raise before any launch; configurations that are not served say so."""
    from splat_loam_amd import _abi, synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.rasterizer import GaussianRasterizer
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 500, 32, 256
    sc = synth.make_scene(N, H, W, seed=1, range_lo=2.0, range_hi=15.0, scale_hi=0.25)
    view, proj = synth.camera_matrices(sc["K"])
    settings = _settings(device, view, proj, H, W)
    t = {k: torch.tensor(sc[k], device=device) for k in ("means", "scales", "rots", "opac")}

    def call(xi):
        return GaussianRasterizer(raster_settings=settings)(means3D=t["means"], means2D=t["means"], opacities=t["opac"],
                                                            scales=t["scales"], rotations=t["rots"], pose_delta=xi)
    with pytest.raises(ValueError, match="shape"):
        call(torch.zeros(7, device=device, requires_grad=True))
    with pytest.raises(ValueError, match="shape"):
        call(torch.zeros((1, 6), device=device, requires_grad=True))
    with pytest.raises(ValueError, match="float32"):
        call(torch.zeros(6, device=device, dtype=torch.float64, requires_grad=True))
    with pytest.raises(ValueError, match="is on"):
        call(torch.zeros(6, requires_grad=True))
    with pytest.raises(TypeError):
        call(np.zeros(6, np.float32))
    # a pose_delta that does not require grad is a plain render
    _, am = call(torch.zeros(6, device=device))
    assert not am.requires_grad
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, None, data_device=str(device))
    eng = MappingEngine(SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device)), MappingConfig())
    with pytest.raises(ValueError, match="sync=True"):
        eng.step(cam, sync=False, pose_grad=True)
    with pytest.raises(ValueError, match="sync=True"):
        eng.step(cam, sync="lagged", pose_grad=True)
    # the C-ABI: a pose pointer without its scratch, or with too little of it, is refused before anything is enqueued
    lib = _abi.lib()
    pg = torch.zeros(6, device=device)
    small = torch.zeros(8, dtype=torch.uint8, device=device)
    scam = _abi.SlsCamera()
    dummy = pg.data_ptr()
    args = [C.byref(scam), N, 0] + [dummy] * 7 + [1] + [dummy] * 11 + [0]
    assert lib.sls_backward_pose(*args, pg.data_ptr(), None, 0, None) == -1 and b"pose_scratch" in lib.sls_last_error()
    assert lib.sls_backward_pose(*args, pg.data_ptr(), small.data_ptr(), 8, None) == -3 and b"pose-gradient scratch" in lib.sls_last_error()


def test_pose_refinement_on_a_room(device):
    """End to end on a scene whose render is a surface.  The float64 checker chain with the functional as the gradient
    takes this configuration from loss 0.08549 to 0.06095 and from 3.0 cm / 0.236 deg to 0.046 cm / 0.0094 deg in 40
    iterations (not monotonically: Adam's fixed step overshoots); with the gradient negated it is at loss 0.1309, 8.2 cm /
    0.457 deg after 15.  Conditions here (engine deterministic = 1): the final loss below the initial loss; both error
    components at most 1/4 of their initial values (the reference's 1/25 with a factor of six for float32 and the
    overshoot); with the gradient negated the loss after 15 iterations above the initial loss."""
    out = pose_ref.run_refinement(device)
    m0, r0 = out["start_error"]
    m1, r1 = out["refined"]["error"]
    print(f"\n[room] {out['surfels']} surfels, {100 * out['valid_fraction']:.1f} % of the pixels valid")
    print(f"    refined: loss {out['refined']['loss_start']:.5f} -> {out['refined']['loss_end']:.5f}; "
          f"{100 * m0:.3f} cm / {np.degrees(r0):.4f} deg -> {100 * m1:.4f} cm / {np.degrees(r1):.4f} deg; {out['refined']['stats']}")
    mn, rn = out["negated"]["error"]
    print(f"    negated gradient, 15 iterations: loss {out['negated']['loss_start']:.5f} -> {out['negated']['loss_end']:.5f}; "
          f"{100 * mn:.3f} cm / {np.degrees(rn):.4f} deg")
    assert out["surfels"] == 9560 and out["valid_fraction"] == 1.0
    assert abs(m0 - 0.03) <= 1e-3 and abs(np.degrees(r0) - 0.236) <= 1e-3
    assert out["refined"]["loss_end"] < out["refined"]["loss_start"]
    assert m1 <= m0 / 4 and r1 <= r0 / 4, (m1, r1)
    assert out["negated"]["loss_end"] > out["negated"]["loss_start"]
