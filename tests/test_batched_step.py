"""The keyframe-batched mapping step (MappingEngine.step_batch / sls_mapping_step_batch): G keyframes, gradients
summed, the regulariser once, ONE Adam update — pinned to the single-keyframe step and to float64."""
import datetime
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LRS = (5e-4, 5e-2, 5e-3, 1e-3)
BETAS = (0.9, 0.999)
EPS = 1e-15
C5 = dict(N=50000, H=64, W=1024, G=8)      # config 5's geometry: 8 keyframes of a 64x1024 LiDAR window
RAGGED = dict(N=4999, H=32, W=256, G=3)    # odd N (the separate optimiser kernel), a small image, three keyframes


def _scene(N, H, W):
    from splat_loam_amd import synth
    sc = synth.make_scene(N, H, W, seed=31, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    return sc, depth, valid


def _cameras(scene, G, device, first=0):
    from splat_loam_amd import synth
    from splat_loam_amd.scene import Camera
    sc, depth, valid = scene
    poses = synth.keyframe_poses(8)
    return [Camera(sc["K"], depth, None, valid, poses[k], data_device=str(device)) for k in range(first, first + G)]


def _engine(scene, device, flat=None, deterministic=False, depth_ratio=0.0):
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import SurfelModel
    sc = scene[0]
    if flat is None:
        model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
    else:
        N = flat.size // 10
        model = SurfelModel(flat[:3 * N].reshape(N, 3), flat[4 * N:6 * N].reshape(N, 2), flat[6 * N:].reshape(N, 4),
                            flat[3 * N:4 * N].reshape(N, 1), device=str(device))
    eng = MappingEngine(model, MappingConfig(depth_ratio=depth_ratio), lrs=LRS, betas=BETAS, eps=EPS)
    if deterministic:
        eng.deterministic = True
    return eng, model


def _flat(model):
    return torch.cat([model._xyz.detach().reshape(-1), model._opacity.detach().reshape(-1),
                      model._scaling.detach().reshape(-1), model._rotation.detach().reshape(-1)]).cpu().numpy()


def _groups(N):
    return ((0, 3 * N, "xyz"), (3 * N, 4 * N, "opacity"), (4 * N, 6 * N, "scaling"), (6 * N, 10 * N, "rotation"))


def _single(eng, cam, with_regulariser):
    """One keyframe's gradient at the engine's parameters (no update), with the engine's void protocol."""
    eng._enqueue(cam, apply_adam=False, with_regulariser=with_regulariser)
    st = eng._parse_status(eng.status.cpu())
    if st["too_small"]:
        eng.capacity = eng._grown(st["R"])
        eng.workspace = None
        eng._enqueue(cam, apply_adam=False, with_regulariser=with_regulariser, allow_reuse=False)
        st = eng._parse_status(eng.status.cpu())
    assert not st["overflow"], st
    return eng.grads[:-2].cpu().numpy().astype(np.float64), st


def _batch_grad(eng, cams):
    """The batch's summed gradient (apply_adam = 0) at the engine's parameters, with the engine's void protocol."""
    for _ in range(3):
        status = eng._enqueue_batch(cams, apply_adam=False, with_regulariser=True)
        h = status[:len(cams) + 1].cpu()
        st = eng._parse_status(h[0])
        if not st["too_small"]:
            break
        eng.capacity = eng._grown(st["R"])
    assert not st["overflow"], st
    assert eng.grads[-2:].abs().sum().item() == 0.0            # the batch's void flags
    return eng.grads[:-2].cpu().numpy().astype(np.float64), st, [eng._parse_status(h[1 + g]) for g in range(len(cams))]


def _compare(got, ref, N, what):
    for a, b, name in _groups(N):
        scale = np.abs(ref[a:b]).max()
        err = np.abs(got[a:b] - ref[a:b]).max()
        assert scale > 0, f"{what}: {name} has no gradient"
        assert err <= 1e-5 * scale, f"{what}: {name} off by {err} (scale {scale})"


# (depth_ratio 1: the batch's keyframes through the non-lean tile kernels and the launched loss stage, kernels B and C)
@pytest.mark.parametrize("geo,depth_ratio", [(C5, 0.0), (RAGGED, 0.0), (C5, 1.0), (RAGGED, 1.0)],
                         ids=["config5", "ragged", "config5-ratio1", "ragged-ratio1"])
def test_batch_gradient_is_the_sum_of_singles(device, geo, depth_ratio):
    """Sum over the keyframes of the single-keyframe gradient (float64; the regulariser on keyframe 0 only) = the batch's
    gradient, and each keyframe's loss sums = its single step's."""
    N, H, W, G = geo["N"], geo["H"], geo["W"], geo["G"]
    scene = _scene(N, H, W)
    cams = _cameras(scene, G, device)
    eng, _ = _engine(scene, device, depth_ratio=depth_ratio)
    total = np.zeros(10 * N, np.float64)
    singles = []
    for g, cam in enumerate(cams):
        grad, st = _single(eng, cam, with_regulariser=(g == 0))
        total += grad
        singles.append(st)
    eng2, _ = _engine(scene, device, depth_ratio=depth_ratio)
    got, bst, kst = _batch_grad(eng2, cams)
    _compare(got, total, N, f"G={G}")
    for g in range(G):
        for a, b in zip(kst[g]["sums"] + [kst[g]["loss_pixel"]], singles[g]["sums"] + [singles[g]["loss_pixel"]]):
            assert abs(a - b) <= 1e-6 * max(abs(b), 1e-30), f"keyframe {g}: loss sums {kst[g]} vs {singles[g]}"
        assert kst[g]["R"] == singles[g]["R"]
    assert abs(bst["loss_pixel"] - sum(s["loss_pixel"] for s in singles)) <= 1e-5 * abs(bst["loss_pixel"])
    assert bst["R"] == max(s["R"] for s in singles)
    assert bst["loss_reg"] == singles[0]["loss_reg"]


def test_one_adam_per_batch_matches_float64(device):
    """Three batched steps: each step's parameters and moments against a float64 Adam fed that step's float32 batched
    gradient, chained from the dumped state; the Adam step count advances by one per batch."""
    N, H, W, G = C5["N"], C5["H"], C5["W"], C5["G"]
    scene = _scene(N, H, W)
    cams = _cameras(scene, G, device)
    eng, model = _engine(scene, device)
    eng.keep_grads = True
    lr = np.concatenate([np.full(b - a, LRS[k]) for k, (a, b, _) in enumerate(_groups(N))])
    b1, b2 = BETAS
    for s in range(3):
        p = _flat(model).astype(np.float64)
        m0, v0 = eng.exp_avg.cpu().numpy().astype(np.float64), eng.exp_avg_sq.cpu().numpy().astype(np.float64)
        st = eng.step_batch(cams)
        assert not st["overflow"] and eng.t == s + 1
        g = eng.grads[:-2].cpu().numpy().astype(np.float64)
        t = s + 1
        m_ref = b1 * m0 + (1 - b1) * g
        v_ref = b2 * v0 + (1 - b2) * g * g
        p_ref = p - lr / (1 - b1 ** t) * m_ref / (np.sqrt(v_ref) / np.sqrt(1 - b2 ** t) + EPS)
        p1 = _flat(model).astype(np.float64)
        tol = 2 * np.spacing(np.abs(p_ref).astype(np.float32)).astype(np.float64) + 1e-5 * np.abs(p_ref - p)
        bad = np.abs(p1 - p_ref) > tol
        assert not bad.any(), f"step {s}: {int(bad.sum())} parameters off the float64 Adam step"
        for a, b, name in _groups(N):
            for got, ref, what in ((eng.exp_avg, m_ref, "exp_avg"), (eng.exp_avg_sq, v_ref, "exp_avg_sq")):
                got = got[a:b].cpu().numpy().astype(np.float64)
                assert np.abs(got - ref[a:b]).max() <= 2e-6 * np.abs(ref[a:b]).max(), f"step {s}: {what} {name}"


def _state(eng, model):
    return [t.detach().clone() for t in (model._xyz, model._scaling, model._rotation, model._opacity, eng.exp_avg,
                                         eng.exp_avg_sq)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_g1_is_step_bit_for_bit(device):
    """Deterministic mode 1: a batch of one keyframe IS the single step — parameters, moments and loss sums after three
    iterations."""
    _g1_is_step(device, 0.0)


def test_g1_is_step_bit_for_bit_depth_ratio_1(device):
    """The same at depth_ratio 1 (the median depth: kernels B and C launched, the non-lean tile kernels)."""
    _g1_is_step(device, 1.0)


def _g1_is_step(device, depth_ratio):
    N, H, W = C5["N"], C5["H"], C5["W"]
    scene = _scene(N, H, W)
    cam_a, cam_b = _cameras(scene, 1, device)[0], _cameras(scene, 1, device)[0]
    ea, ma = _engine(scene, device, deterministic=True, depth_ratio=depth_ratio)
    eb, mb = _engine(scene, device, deterministic=True, depth_ratio=depth_ratio)
    for s in range(3):
        sa = ea.step(cam_a)
        sb = eb.step_batch([cam_b])
        assert sa["sums"] == sb["sums"] == sb["keyframes"][0]["sums"], s
        assert sa["loss_pixel"] == sb["loss_pixel"] and sa["loss_reg"] == sb["loss_reg"], s
    assert ea.t == eb.t == 3
    assert _same(_state(ea, ma), _state(eb, mb))


@pytest.mark.parametrize("N", [258, 4999], ids=["two_workgroups", "odd_n_fallback"])
def test_g1_is_step_bit_for_bit_with_pose_and_kept_grads(device, N):
    """The same equality through the chain, the pose rows and the Adam tail together, at the smallest sizes that cross a
    workgroup (258: Adam fused into the projection's backward) and take the separate optimiser kernel (4999, odd):
    state, gradient bucket and pose row after each of three iterations."""
    H, W = RAGGED["H"], RAGGED["W"]
    scene = _scene(N, H, W)
    cam_a, cam_b = _cameras(scene, 1, device)[0], _cameras(scene, 1, device)[0]
    ea, ma = _engine(scene, device, deterministic=True)
    eb, mb = _engine(scene, device, deterministic=True)
    ea.keep_grads = eb.keep_grads = True
    for s in range(3):
        sa = ea.step(cam_a, pose_grad=True)
        sb = eb.step_batch([cam_b], pose_grad=True)
        assert not sa["overflow"] and not sb["overflow"], s
        assert sa["sums"] == sb["sums"] == sb["keyframes"][0]["sums"], s
        assert torch.equal(ea.grads[:-2], eb.grads[:-2]), f"iteration {s}: gradient bucket"
        assert ea.grads[:-2].abs().max().item() > 0.0, f"iteration {s}: no gradient"
        assert ea.pose_grad.shape == (6,) and eb.pose_grad.shape == (1, 6)
        assert torch.equal(ea.pose_grad, eb.pose_grad[0]), f"iteration {s}: pose row"
        assert _same(_state(ea, ma), _state(eb, mb)), f"iteration {s}: parameters or moments"
    assert ea.t == eb.t == 3


def test_deterministic_batches_are_reproducible(device):
    N, H, W, G = C5["N"], C5["H"], C5["W"], C5["G"]
    scene = _scene(N, H, W)
    runs = []
    for _ in range(2):
        eng, model = _engine(scene, device, deterministic=True)
        cams = _cameras(scene, G, device)
        for _ in range(2):
            assert not eng.step_batch(cams)["overflow"]
        runs.append(_state(eng, model))
    assert _same(runs[0], runs[1])


def test_void_keyframe_voids_the_batch(device):
    """Instance buffers too small for some keyframe: bit 0 of the batch, nothing changes; through step_batch the batch
    is repeated with more room and equals, bit for bit (deterministic mode), the same batch on a fresh engine."""
    N, H, W, G = C5["N"], C5["H"], C5["W"], C5["G"]
    scene = _scene(N, H, W)
    cams = _cameras(scene, G, device)
    eng, model = _engine(scene, device, deterministic=True)
    assert not eng.step_batch(cams)["overflow"]
    Rs = [k["R"] for k in eng.last["keyframes"]]
    before = _state(eng, model)
    p1 = _flat(model)
    cap0 = eng._bws["cap"]
    # a capacity below the one the batch workspace was laid out for: the workspace is carved anew
    eng.capacity = (min(Rs) + max(Rs)) // 2 if min(Rs) < max(Rs) else max(Rs) - 1
    assert eng.capacity < cap0
    status = eng._enqueue_batch(cams, apply_adam=True, with_regulariser=True)
    h = status[:G + 1].cpu()
    st = eng._parse_status(h[0])
    assert st["too_small"], st
    per = [eng._parse_status(h[1 + g]) for g in range(G)]
    assert any(not k["overflow"] for k in per) and any(k["too_small"] for k in per)
    assert _same(before, _state(eng, model)), "a void batch changed parameters or moments"
    assert eng.t == 1
    n0 = eng.stats["repeated_too_small"]
    st = eng.step_batch(cams)
    assert not st["overflow"] and eng.t == 2 and eng.stats["repeated_too_small"] == n0 + 1
    assert eng._bws["cap"] == eng.capacity
    # the same second step on a fresh engine holding the state after the first
    ref, ref_model = _engine(scene, device, flat=p1, deterministic=True)
    ref.exp_avg.copy_(before[4]); ref.exp_avg_sq.copy_(before[5]); ref.t = 1
    assert not ref.step_batch(_cameras(scene, G, device))["overflow"]
    assert _same(_state(eng, model), _state(ref, ref_model)), "the repeated batch differs from a fresh one"


def test_batch_after_step_repairs_the_keyframes_orders(device):
    """step() on each keyframe leaves its depth order; the batch that follows repairs them (reuse >= 1) and equals, bit
    for bit in deterministic mode, a batch that sorts every keyframe from scratch."""
    N, H, W, G = C5["N"], C5["H"], C5["W"], 4
    scene = _scene(N, H, W)
    out = []
    for repair in (True, False):
        eng, model = _engine(scene, device, deterministic=True)
        cams = _cameras(scene, G, device)
        for cam in cams:
            assert not eng.step(cam)["overflow"]
        if not repair:
            for cam in cams:
                eng._forget_order(cam)
        assert not eng.step_batch(cams)["overflow"]
        assert all(r >= 1 for r in eng.last_batch_reuse) if repair else all(r == 0 for r in eng.last_batch_reuse)
        # and back: step() after the batch repairs the order the batch left
        assert not eng.step(cams[0])["overflow"]
        out.append(_state(eng, model))
    assert _same(out[0], out[1])


def test_batch_argument_errors(device):
    N, H, W = RAGGED["N"], RAGGED["H"], RAGGED["W"]
    scene = _scene(N, H, W)
    eng, _ = _engine(scene, device)
    cams = _cameras(scene, 3, device)
    with pytest.raises(ValueError):
        eng.step_batch(cams, sync="lagged")
    with pytest.raises(ValueError):
        eng.step_batch([cams[0], cams[1], cams[0]])
    with pytest.raises(ValueError):
        eng.step_batch([])
    other = _cameras(_scene(N, H, 2 * W), 1, device)
    with pytest.raises(ValueError):
        eng.step_batch([cams[0], other[0]])
    assert eng.t == 0


# ---- fewer GPUs than keyframes: two gloo ranks on cuda:0, four keyframes each ---------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_main(rank, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=180))
    try:
        N, H, W = C5["N"], C5["H"], C5["W"]
        scene = _scene(N, H, W)
        eng, model = _engine(scene, "cuda:0")
        eng.dp_mode = "allreduce"
        cams = _cameras(scene, 4, "cuda:0", first=4 * rank)
        grads, params = [], []
        for _ in range(3):
            params.append(_flat(model))
            st = eng.step_batch(cams, group=dist.group.WORLD)
            assert not st["overflow"]
            grads.append(eng.grads[:-2].cpu().numpy())
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), g=np.stack(grads), p=np.stack(params), final=_flat(model),
                 t=eng.t)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_of_four_keyframes_match_one_batch_of_eight(device, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_rank_main, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    R = [np.load(tmp_path / f"r{r}.npz") for r in range(2)]
    assert int(R[0]["t"]) == int(R[1]["t"]) == 3
    assert np.array_equal(R[0]["final"], R[1]["final"]), "replicas diverged"
    N, H, W = C5["N"], C5["H"], C5["W"]
    scene = _scene(N, H, W)
    for s in range(3):
        assert np.array_equal(R[0]["g"][s], R[1]["g"][s]) and np.array_equal(R[0]["p"][s], R[1]["p"][s])
        eng, _ = _engine(scene, device, flat=R[0]["p"][s])
        ref, _, _ = _batch_grad(eng, _cameras(scene, 8, device))
        _compare(R[0]["g"][s].astype(np.float64), ref, N, f"step {s}")
