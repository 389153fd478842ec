"""Sensor poses as optimisation variables.

The rasterizer's backward returns g = dL/dxi at xi = 0 for the LEFT perturbation of the view transform,

    T_vw(xi) = Exp(xi) T_vw,        xi = (v, w) in R^6,        p_view -> p_view + w x p_view + v  (first order),

the convention of the frame-to-keyframe aligner (csrc/sls_aligner.hip).  The sensor's pose in the model is the inverse:
model_T_frame(xi) = model_T_frame Exp(-xi).  This module holds the host side of that: the exponential, the two
retractions, a pose distance, and the model-frozen refinement loop on MappingEngine.pose_step.  Everything here is
float64 on the host — six numbers per iteration; the kernels are in libsls_hip.so.
"""
from __future__ import annotations

import math

import numpy as np


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=np.float64)


def se3_exp(xi) -> np.ndarray:
    """Exp of the twist xi = (v, w): the 4x4 [[R, V v], [0, 1]] with R = exp(hat(w)) (Rodrigues) and
    V = I + B hat(w) + C hat(w)^2, B = (1 - cos t) / t^2, C = (t - sin t) / t^3, t = |w|; below t = 0.2 the
    coefficients come from their series (the closed forms cancel there)."""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    v, w = xi[:3], xi[3:]
    t2 = float(w @ w)
    t = math.sqrt(t2)
    if t < 0.2:
        # (six terms: the next one is below 1e-18 here, while the closed forms lose eps / t^2)
        A = 1.0 + t2 * (-1.0 / 6 + t2 * (1.0 / 120 + t2 * (-1.0 / 5040 + t2 * (1.0 / 362880 - t2 / 39916800))))
        B = 0.5 + t2 * (-1.0 / 24 + t2 * (1.0 / 720 + t2 * (-1.0 / 40320 + t2 * (1.0 / 3628800 - t2 / 479001600))))
        Cc = 1.0 / 6 + t2 * (-1.0 / 120 + t2 * (1.0 / 5040 + t2 * (-1.0 / 362880 + t2 * (1.0 / 39916800 - t2 / 6227020800))))
    else:
        A = math.sin(t) / t
        B = (1.0 - math.cos(t)) / t2
        Cc = (t - math.sin(t)) / (t2 * t)
    K = _hat(w)
    K2 = K @ K
    T = np.eye(4, dtype=np.float64)
    T[:3, :3] = np.eye(3) + A * K + B * K2
    T[:3, 3] = (np.eye(3) + B * K + Cc * K2) @ v
    return T


def _np64(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64).reshape(4, 4)


def retract_view(world_view_transform, xi) -> np.ndarray:
    """The view matrix in the layout of Camera.world_view_transform / GaussianRasterizationSettings.viewmatrix (the
    TRANSPOSE of T_vw: [:3,:3] = R^T, [3,:3] = t) after the step xi: (Exp(xi) T_vw)^T, float64."""
    return (se3_exp(xi) @ _np64(world_view_transform).T).T


def retract_pose(model_T_frame, xi) -> np.ndarray:
    """The sensor's pose in the model after the same step: model_T_frame Exp(-xi) = inv(Exp(xi) T_vw), float64."""
    return _np64(model_T_frame) @ se3_exp(-np.asarray(xi, dtype=np.float64))


def pose_error(A, B):
    """(metres, radians) between two rigid transforms given as 4x4 matrices with the translation in the last COLUMN
    (poses, or T_vw = world_view_transform^T): translation norm and rotation angle of inv(A) B."""
    D = np.linalg.inv(_np64(A)) @ _np64(B)
    c = min(1.0, max(-1.0, 0.5 * (float(np.trace(D[:3, :3])) - 1.0)))
    # (the angle from the skew part where the cosine is flat)
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.linalg.norm(D[:3, 3])), float(math.atan2(s, c))


class TwistAdam:
    """Adam on the six twist coordinates, on the host in float64: step size lr_t on v (metres), lr_r on w (radians).
    The twist is re-centred at every iteration (the gradient is always taken at xi = 0 of the current pose), so the
    moments live in the moving view frame — exact for the small steps a refinement takes."""

    def __init__(self, lr_t: float, lr_r: float, betas=(0.9, 0.999), eps: float = 1e-15):
        self.lr = np.array([lr_t] * 3 + [lr_r] * 3, dtype=np.float64)
        self.b1, self.b2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        self.m, self.v, self.t = np.zeros(6), np.zeros(6), 0

    def step(self, g) -> np.ndarray:
        """The twist to retract by for the gradient g = dL/dxi."""
        g = np.asarray(g, dtype=np.float64).reshape(6)
        self.t += 1
        self.m = self.b1 * self.m + (1.0 - self.b1) * g
        self.v = self.b2 * self.v + (1.0 - self.b2) * g * g
        mh = self.m / (1.0 - self.b1 ** self.t)
        vh = self.v / (1.0 - self.b2 ** self.t)
        return -self.lr * mh / (np.sqrt(vh) + self.eps)


def set_camera_view(camera, world_view_transform64) -> None:
    """Writes a float64 view matrix into camera.world_view_transform IN PLACE: the camera object — and with it the
    keyframe's cached depth order, launch order and measurement tables — stays; the tensor's version changes, so the
    rasterizer rebuilds its SlsCamera (R, t by value) while the ray tables, which depend on K only, come from their cache.
    Only that tensor is rewritten: whatever a caller derived from the old pose (a frame's model_T_frame, a cached inverse
    of the old view matrix) is the caller's to update — retract_pose gives the matching pose."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(world_view_transform64, dtype=np.float32))
    camera.world_view_transform.copy_(t.to(camera.world_view_transform.device))


def refine_pose(engine, camera, iterations: int, lr_t: float = 2e-3, lr_r: float = 2e-4, betas=(0.9, 0.999),
                eps: float = 1e-15):
    """Model-frozen refinement of `camera`'s pose against the engine's model by descending the mapper's own pixel loss:
    per iteration one MappingEngine.pose_step (forward, loss, backward; no parameter changes), the six floats read
    beside the status, one Adam step on the twist, the retraction, the camera's view matrix rewritten in place.
    A pose update of a few centimetres keeps the keyframe's depth order repairable; where it does not, the iteration
    is void and repeated from a fresh sort by pose_step itself.
    Returns {"world_view_transform": float64 (4,4) in the camera's layout, "model_T_frame": its inverse-transpose,
    "loss": the loss at the start of every iteration, "final_loss": the loss at the refined pose}."""
    view = _np64(camera.world_view_transform)
    opt = TwistAdam(lr_t, lr_r, betas, eps)
    trace = []
    for _ in range(int(iterations)):
        st = engine.pose_step(camera)
        trace.append(st["loss"])
        g = engine.pose_grad.cpu().numpy().astype(np.float64)
        view = retract_view(view, opt.step(g))
        set_camera_view(camera, view)
    final = engine.pose_step(camera)["loss"]
    return {"world_view_transform": view, "model_T_frame": np.linalg.inv(view.T), "loss": trace, "final_loss": final}
