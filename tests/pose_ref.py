"""Reference side of the pose-gradient tests — shared by tests/test_pose_math.py (CPU) and
tests/test_pose_grad.py (GPU).  Not a test module.

Moving the sensor by Exp(xi) is the same as moving every surfel rigidly the other way, so g = dL/dxi is a LINEAR
FUNCTIONAL of gradients the checker already produces.  With f_i = R dL/dmu_i, quaternion q = (q_w, q_v) and its gradient
(h_w, h_v):

    tau_i = 1/2 (-h_w q_v + q_w h_v + q_v x h_v)        world-frame torque (a multiple of q in h contributes 0)
    g_v   = sum_i f_i
    g_w   = sum_i (p_v,i x f_i + R tau_i)

g is a cancelling sum: errors are measured per component against S_k = sum_i |term_i,k|.
"""
import numpy as np
import torch


def view_Rt(view):
    """(R, t) of p_view = R p_world + t from a viewmatrix (the transpose of the view transform)."""
    V = np.asarray(view, np.float64)
    return V[:3, :3].T.copy(), V[3, :3].copy()


def functional(view, means, quats, dmeans, dquats):
    """(g, S): the pose gradient [v | w] from the surfels' gradients, and the scale sum_i |term_i| per component.
    `quats` / `dquats` may be raw (un-normalised) quaternions with their raw gradients: normalisation commutes with a
    left rotation."""
    R, t = view_Rt(view)
    mu, q = np.asarray(means, np.float64), np.asarray(quats, np.float64)
    f = np.asarray(dmeans, np.float64) @ R.T
    h = np.asarray(dquats, np.float64)
    pv = mu @ R.T + t
    tau = 0.5 * (-h[:, :1] * q[:, 1:] + q[:, :1] * h[:, 1:] + np.cross(q[:, 1:], h[:, 1:]))
    tw = tau @ R.T
    pf = np.cross(pv, f)
    g = np.concatenate([f.sum(0), (pf + tw).sum(0)])
    S = np.concatenate([np.abs(f).sum(0), (np.abs(pf) + np.abs(tw)).sum(0)])
    return g, S


def rigid_motion_leaves(view, means, quats):
    """xi (a float64 leaf at zero) and the surfels moved by the rigid WORLD motion that equals the left twist xi of the
    view transform, to first order: (xi, means(xi), quats(xi)) as torch tensors."""
    R, t = view_Rt(view)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    v, w = xi[:3], xi[3:]
    Rt, tt = torch.tensor(R), torch.tensor(t)
    m0, q0 = torch.tensor(np.asarray(means, np.float64)), torch.tensor(np.asarray(quats, np.float64))
    pv = m0 @ Rt.T + tt
    dpv = torch.linalg.cross(w.expand_as(pv), pv) + v
    m1 = m0 + dpv @ Rt                               # R^T dpv, as rows
    ww = Rt.T @ w                                    # the rotation vector in the world
    q0w, q0v = q0[:, 0:1], q0[:, 1:]
    dq = 0.5 * torch.cat([-(q0v * ww).sum(1, keepdim=True), q0w * ww + torch.linalg.cross(ww.expand_as(q0v), q0v)], 1)
    return xi, m1, q0 + dq


def in_units_of_S(g, g_ref, S):
    """|g - g_ref|_k / S_k per component"""
    return np.abs(np.asarray(g, np.float64) - np.asarray(g_ref, np.float64)) / np.asarray(S, np.float64)


def box_room(step=0.15, half=(6.0, 4.0), z=(-1.7, 1.3), sigma=0.1, opacity=0.9):
    """A room whose render is a SURFACE: surfels on a `step` grid on the floor and the four walls of a 12 x 8 x 3 m box,
    the sensor at the origin 1.7 m above the floor, normals inward.  RAW parameters (float32) as the engine takes them:
    xyz (N,3), scaling (N,2) = log sigma, rotation (N,4; w,x,y,z), opacity (N,1) = logit."""
    from splat_loam_amd import synth
    X, Y = half
    Z0, Z1 = z
    ex, ey, ez = np.eye(3)
    pts, nrm = [], []

    def face(origin, eu, ev, nu, nv, n):
        i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
        pts.append(origin + (i.reshape(-1, 1) + 0.5) * step * eu + (j.reshape(-1, 1) + 0.5) * step * ev)
        nrm.append(np.tile(np.asarray(n, np.float64), (nu * nv, 1)))

    nx, ny, nz = int(2 * X / step), int(2 * Y / step), int((Z1 - Z0) / step)
    face(np.array([-X, -Y, Z0]), ex, ey, nx, ny, ez)            # floor
    face(np.array([-X, -Y, Z0]), ex, ez, nx, nz, ey)            # wall y = -Y
    face(np.array([-X, Y, Z0]), ex, ez, nx, nz, -ey)
    face(np.array([-X, -Y, Z0]), ey, ez, ny, nz, ex)
    face(np.array([X, -Y, Z0]), ey, ez, ny, nz, -ex)
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    N = len(pts)
    h2 = np.where(np.abs(nrm[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    t0 = np.cross(nrm, h2)
    t0 /= np.linalg.norm(t0, axis=1, keepdims=True)
    t1 = np.cross(nrm, t0)
    q = synth._quat_from_R(np.stack([t0, t1, nrm], 2))
    raw = {"xyz": pts, "scaling": np.log(np.full((N, 2), sigma)), "rotation": q,
           "opacity": np.full((N, 1), np.log(opacity / (1.0 - opacity)))}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in raw.items()}


def _negated(engine):
    """test-local: the same engine with the sign of the pose gradient flipped"""
    class Negated:
        def pose_step(self, camera):
            st = engine.pose_step(camera)
            self.pose_grad = -engine.pose_grad
            return st
    return Negated()


def run_refinement(device, H=32, W=256, iterations=40, iterations_negated=15, step=0.15):
    """Model-frozen refinement on the box room (box_room above): targets = what the model renders from the true
    pose, start 3.0 cm / 0.236 degrees off, Adam (0.9, 0.999, 1e-15) on the twist with steps 2e-3 m / 2e-4 rad."""
    from splat_loam_amd import pose, synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from splat_loam_amd.scene import Camera, SurfelModel
    raw = box_room(step=step)
    K = synth.spherical_K(H, W)
    view_true, proj = synth.camera_matrices(K, None)
    model = SurfelModel(raw["xyz"], raw["scaling"], raw["rotation"], raw["opacity"], device=str(device))
    with torch.no_grad():
        settings = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view_true, device=device), torch.tensor(proj, device=device))
        _, am = GaussianRasterizer(raster_settings=settings)(
            means3D=model.get_xyz, means2D=model.get_xyz, opacities=model.get_opacity, scales=model.get_scaling,
            rotations=model.get_rotation)
    alpha = am[1]
    valid = (alpha > 0.5)
    gt = torch.where(valid, am[0] / alpha.clamp_min(1e-9), torch.zeros_like(alpha))
    xi0 = np.array([0.02, -0.02, 0.01, 0.002, -0.002, 0.003])
    T_true = np.asarray(view_true, np.float64).T
    T_start = pose.se3_exp(xi0) @ T_true
    out = {"surfels": int(raw["xyz"].shape[0]), "valid_fraction": float(valid.float().mean()),
           "start_error": pose.pose_error(T_true, T_start)}
    for tag, its, wrap in (("refined", iterations, lambda e: e), ("negated", iterations_negated, _negated)):
        cam = Camera(K, gt[None].cpu().numpy(), None, valid[None].to(torch.uint8).cpu().numpy(), np.linalg.inv(T_start),
                     data_device=str(device))
        eng = MappingEngine(model, MappingConfig())
        eng.deterministic = 1
        res = pose.refine_pose(wrap(eng), cam, its, lr_t=2e-3, lr_r=2e-4)
        out[tag] = {"loss_start": res["loss"][0], "loss_end": res["final_loss"], "loss": res["loss"],
                    "error": pose.pose_error(T_true, res["world_view_transform"].T), "stats": dict(eng.stats)}
        assert np.abs(np.linalg.inv(res["world_view_transform"].T) - res["model_T_frame"]).max() <= 1e-12
    return out
