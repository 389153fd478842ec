"""Host side of the pose gradient, without a GPU: splat_loam_amd/pose.py, and the identity
the GPU tests use as their reference — the pose gradient as a linear functional of the checker's surfel gradients —
pinned against autograd through the float64 torch formulation and against finite differences over the CAMERA."""
import numpy as np
import torch

import pose_ref
from splat_loam_amd import pose, synth


def _expm_series(M, terms=40):
    out, term = np.eye(4), np.eye(4)
    for k in range(1, terms):
        term = term @ M / k
        out = out + term
    return out


def _twist_matrix(xi):
    M = np.zeros((4, 4))
    M[:3, :3] = pose._hat(xi[3:])
    M[:3, 3] = xi[:3]
    return M


def test_se3_exp_is_the_matrix_exponential():
    rng = np.random.default_rng(0)
    cases = [np.zeros(6), np.array([0.02, -0.02, 0.01, 0.002, -0.002, 0.003])]
    cases += [np.concatenate([rng.normal(size=3), rng.normal(size=3) * s]) for s in (1e-9, 1e-6, 5e-5, 1e-4, 2e-4, 1e-2, 0.1, 0.12, 0.5, 2.0)]
    for xi in cases:
        T = pose.se3_exp(xi)
        assert T.dtype == np.float64 and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
        # (float64 rounding of a handful of operations on entries of size max(1, |xi|); the closed forms lose eps / t^2,
        #  3e-15 at the switch to the series)
        tol = 1e-13 * max(1.0, np.abs(xi).max()) ** 2
        assert np.abs(T - _expm_series(_twist_matrix(xi))).max() <= tol, xi
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= tol
        assert np.abs(T @ pose.se3_exp(-xi) - np.eye(4)).max() <= tol


def test_the_two_retractions_are_inverse_transposes():
    rng = np.random.default_rng(1)
    for p in synth.keyframe_poses(4):
        view, _ = synth.camera_matrices(synth.spherical_K(16, 64), p)
        view = np.asarray(view, np.float64)
        model_T_frame = np.linalg.inv(view.T)
        xi = rng.normal(size=6) * np.array([0.05] * 3 + [0.01] * 3)
        small = 1e-3 * xi
        v2 = pose.retract_view(view, xi)
        p2 = pose.retract_pose(model_T_frame, xi)
        assert v2.dtype == np.float64 and p2.dtype == np.float64
        assert np.abs(np.linalg.inv(v2.T) - p2).max() <= 1e-13 * max(1.0, np.abs(p2).max())
        # the layout of Camera.world_view_transform: R^T in [:3,:3], t in the last ROW; first order in xi: p -> p + w x p + v
        Rm, t = pose_ref.view_Rt(view)
        R2, t2 = pose_ref.view_Rt(pose.retract_view(view, small))
        pw = rng.normal(size=3)
        pv = Rm @ pw + t
        # (second order in the twist: |xi|^2 |p_v|)
        assert np.abs((R2 @ pw + t2) - (pv + np.cross(small[3:], pv) + small[:3])).max() <= (small @ small) * (1.0 + np.linalg.norm(pv))
        assert np.array_equal(v2[:, 3], [0.0, 0.0, 0.0, 1.0])
        # torch tensors are accepted as they come out of a Camera
        assert np.array_equal(pose.retract_view(torch.tensor(view), xi), v2)


def test_pose_error_measures_metres_and_radians():
    A = np.linalg.inv(synth.keyframe_poses(3)[2])
    xi = np.array([0.02, -0.02, 0.01, 0.002, -0.002, 0.003])
    dm, dr = pose.pose_error(np.eye(4), pose.se3_exp(xi))
    # (3.0 cm, 0.236 degrees: the start of the refinement test)
    assert abs(dr - np.linalg.norm(xi[3:])) <= 1e-12 and abs(dm - 0.03) <= 1e-4
    assert abs(np.degrees(dr) - 0.236) <= 1e-3
    dm2, dr2 = pose.pose_error(A, A @ pose.se3_exp(xi))            # (relative: the same step from any pose)
    assert abs(dm2 - dm) <= 1e-12 and abs(dr2 - dr) <= 1e-12
    assert max(pose.pose_error(A, A)) <= 1e-15
    # tiny angles survive (the angle comes from the skew part, not from acos of the trace)
    _, dr = pose.pose_error(np.eye(4), pose.se3_exp(np.array([0, 0, 0, 1e-9, 0, 0])))
    assert abs(dr - 1e-9) <= 1e-15


def test_twist_adam_is_adam():
    opt = pose.TwistAdam(2e-3, 2e-4, eps=1e-15)
    x = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    ref = torch.optim.Adam([{"params": [x], "lr": 1.0}], eps=1e-15)
    rng = np.random.default_rng(2)
    acc = np.zeros(6)
    for _ in range(5):
        g = rng.normal(size=6)
        acc += opt.step(g)
        x.grad = torch.tensor(g)
        ref.step()
    assert np.abs(acc - x.detach().numpy() * np.array([2e-3] * 3 + [2e-4] * 3)).max() <= 1e-12


def test_pose_gradient_is_a_functional_of_the_surfel_gradients(oracle64):
    """The reference of tests/test_pose_grad.py, pinned: 40 surfels on 16 x 64, wrapping camera, random dL/dallmap."""
    from oracle import torch_ref
    N, H, W = 40, 16, 64
    sc = synth.make_scene(N, H, W, seed=1, range_lo=2.0, range_hi=6.0, scale_lo=0.05, scale_hi=0.4)
    rots = sc["rots"].astype(np.float64)
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    view = np.linalg.inv(synth.keyframe_poses(2)[1]).T
    _, proj = synth.camera_matrices(sc["K"])
    cam = oracle64.camera(H, W, view, proj)
    assert cam.wrap == 1
    args = [np.asarray(sc["means"], np.float64), np.asarray(sc["scales"], np.float64), rots, np.asarray(sc["opac"], np.float64)]
    st = oracle64.forward(cam, *args)
    Wt = np.random.default_rng(5).normal(size=(7, H, W))
    Wt[5] = 0
    bw = oracle64.backward(st, Wt)
    g, S = pose_ref.functional(view, args[0], args[2], bw["dmeans"], bw["drots"])
    assert np.abs(g).min() > 1.0 and (S > np.abs(g)).all()       # (a cancelling sum of sizeable terms)

    # == autograd through the dense float64 formulation under the rigid motion of the surfels
    xi, m1, q1 = pose_ref.rigid_motion_leaves(view, args[0], args[2])
    am = torch_ref.dense_forward(cam, st["tables"], st["pre"], m1, torch.tensor(args[1]), q1, torch.tensor(args[3]))
    (am * torch.tensor(Wt)).sum().backward()
    err = np.abs(g - xi.grad.numpy()).max()
    print(f"\nfunctional vs autograd through the rigid motion: {err:.2e}")
    assert err <= 1e-10

    # == central differences of the checker's forward over the CAMERA: viewmatrix' = (Exp(xi) T_vw)^T
    def loss_at(x):
        cam2 = oracle64.camera(H, W, np.ascontiguousarray(pose.retract_view(view, x)), proj)
        return float((oracle64.forward(cam2, *args)["allmap"] * Wt).sum())

    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        fd = (loss_at(e) - loss_at(-e)) / (2 * h)
        print(f"component {k}: functional {g[k]:+.6f}  camera finite difference {fd:+.6f}")
        assert abs(fd - g[k]) <= 2e-5 * max(1.0, abs(fd)), (k, fd, g[k])


def test_pose_arguments_are_refused_before_anything_is_enqueued():
    """The C-ABI's checks of the pose arguments come before the first launch, so they can be exercised without a GPU
    (the other pointers only have to be non-null): a pose pointer without scratch, with too little of it, a batch with
    the single-keyframe pointer, a batch with a gradient asked for on some keyframes only, two keyframes sharing one."""
    import ctypes as C
    from splat_loam_amd import _abi
    lib = _abi.lib()
    N, P = 1000, 4096                       # (P: a non-null, 256-byte aligned value that is never dereferenced)
    need = lib.sls_pose_grad_scratch_bytes(N)
    assert need == 256 + 32 * ((N + 255) // 256) and lib.sls_pose_grad_scratch_bytes(0) == 0
    cam = _abi.SlsCamera()
    cam.H, cam.W = 32, 256
    for name, head in (("sls_backward_pose", [C.byref(cam), N, 0] + [P] * 7 + [1] + [P] * 11 + [0]),
                       ("sls_backward_det_pose", [C.byref(cam), N, 0] + [P] * 7 + [1] + [P] * 10 + [0, P, 1 << 30]),
                       ("sls_backward_ws_pose", [C.byref(cam), N] + [P] * 7 + [1 << 16, P, 1 << 30, P, 1, 3] + [P] * 5)):
        fn = getattr(lib, name)
        assert fn(*head, P, None, 0, None) == -1 and b"pose_scratch" in lib.sls_last_error(), name
        assert fn(*head, P, P + 4, need, None) == -1 and b"aligned" in lib.sls_last_error(), name
        assert fn(*head, P, P, need - 1, None) == -3 and b"pose-gradient scratch too small" in lib.sls_last_error(), name
    cfg = _abi.SlsMappingConfig()
    cfg.pose_grad = P
    step = [C.byref(cam), N] + [P] * 7 + [1, P, P, 10] + [P] * 4 + [C.byref(cfg), 1 << 16, P, 1 << 30, P, None, None]
    assert lib.sls_mapping_step(*step) == -1 and b"pose_scratch" in lib.sls_last_error()
    cfg.pose_scratch, cfg.pose_scratch_bytes = P, need - 1
    assert lib.sls_mapping_step(*step) == -3
    kfs = (_abi.SlsKeyframeInputs * 2)()
    for g, k in enumerate(kfs):
        k.cam = cam
        k.gt_depth = k.valid = k.col_cs = k.row_cs = k.col_cs_half = k.row_cs_half = P
        k.depth_order = P + 4096 * g
    batch = lambda G: [G, kfs, N] + [P] * 7 + [1, C.byref(cfg), 1 << 16, P, 1 << 30, P, None]
    cfg.pose_scratch_bytes = 2 * need
    assert lib.sls_mapping_step_batch(*batch(2)) == -1 and b"per keyframe" in lib.sls_last_error()
    cfg.pose_grad = None
    kfs[0].pose_grad = P
    assert lib.sls_mapping_step_batch(*batch(2)) == -1 and b"every keyframe" in lib.sls_last_error()
    kfs[1].pose_grad = P
    assert lib.sls_mapping_step_batch(*batch(2)) == -1 and b"share one pose_grad" in lib.sls_last_error()
    kfs[1].pose_grad = P + 64
    cfg.pose_scratch_bytes = 2 * need - 1
    assert lib.sls_mapping_step_batch(*batch(2)) == -3
