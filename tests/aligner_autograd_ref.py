"""An independent float64 statement of the registration's normal equations, for the tests only.

`oracle/aligner_ref.py` follows the kernel formula by formula, so a slip in a Jacobian would be shared.  Here
nothing analytic is written down: with the associations `j` and the Huber weights frozen at the checker's, both
residuals are functions of a LEFT twist xi = (v, w), the moved point being p(xi) = matrix_exp(hat(xi)) T p:

    e_g(xi) = n_j . (p(xi) - q_j)
    e_r(xi) = |p(xi)| - (D_j + gu_j (u(p(xi)) - u(p(0))) + gv_j (v(p(xi)) - v(p(0))))

with u = fx atan2(y, x) + cx, v = fy atan2(z, hypot(x, y)) + cy, and the image gradient (gu, gv) recomputed
here from the reference range image by the stated rule (central difference; zero at a border, columns wrapping
only on a wrapping camera; zero beside a depth <= depth_min).  J comes from torch's forward-mode autograd,
H = J^T W J, b = J^T W e, chi2 = sum w e^2.
"""
import numpy as np
import torch


def range_gradient(depth_img, depth_min, wrap, r, c):
    """(gu, gv) at the pixels (r[i], c[i]), one pixel at a time."""
    H, W = depth_img.shape
    gu, gv = np.zeros(len(r)), np.zeros(len(r))
    for i, (ri, ci) in enumerate(zip(r, c)):
        left, right = ci - 1, ci + 1
        if wrap:
            left, right = left % W, right % W
        if 0 <= left and right < W:
            a, b = float(depth_img[ri, left]), float(depth_img[ri, right])
            if a > depth_min and b > depth_min:
                gu[i] = (b - a) / 2.0
        if 0 < ri < H - 1:
            a, b = float(depth_img[ri - 1, ci]), float(depth_img[ri + 1, ci])
            if a > depth_min and b > depth_min:
                gv[i] = (b - a) / 2.0
    return gu, gv


def _hat(xi):
    z = xi.new_zeros(())
    return torch.stack([torch.stack([z, -xi[5], xi[4], xi[0]]),
                        torch.stack([xi[5], z, -xi[3], xi[1]]),
                        torch.stack([-xi[4], xi[3], z, xi[2]]),
                        torch.stack([z, z, z, z])])


def _weights(e, delta):
    a = np.abs(e)
    return np.where(a <= delta, 1.0, delta / np.maximum(a, 1e-300))


def system(cam, prm, ref_depth, ref_points, ref_normals, q_points, T, det):
    """-> dict(H (6,6), b (6,), chi2, inliers, S (6,) = sum_i |w J_ik e_i|, gu, gv) for the inliers and the
    weights of the checker's details `det`."""
    Hh, Ww = cam["H"], cam["W"]
    ok = det["ok"]
    j = det["j"][ok]
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    q = t(np.asarray(q_points).reshape(-1, 3)[ok])
    tgt = t(np.asarray(ref_points).reshape(-1, 3)[j])
    nrm = t(np.asarray(ref_normals).reshape(-1, 3)[j])
    depth_img = np.asarray(ref_depth, np.float64).reshape(Hh, Ww)
    D = t(depth_img.reshape(-1)[j])
    gu_np, gv_np = range_gradient(depth_img, prm.depth_min, cam["wrap"], j // Ww, j % Ww)
    gu, gv = t(gu_np), t(gv_np)
    Tt = t(T)
    with_range = prm.range_weight > 0.0

    def moved(xi):
        M = torch.linalg.matrix_exp(_hat(xi)) @ Tt
        return q @ M[:3, :3].T + M[:3, 3]

    def uv(p):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        return cam["fx"] * torch.atan2(y, x) + cam["cx"], cam["fy"] * torch.atan2(z, torch.hypot(x, y)) + cam["cy"]

    xi0 = torch.zeros(6, dtype=torch.float64)
    u0, v0 = uv(moved(xi0))

    def residuals(xi):
        p = moved(xi)
        e_g = (nrm * (p - tgt)).sum(1)
        if not with_range:
            return e_g
        u, v = uv(p)
        e_r = torch.linalg.vector_norm(p, dim=1) - (D + gu * (u - u0) + gv * (v - v0))
        return torch.cat([e_g, e_r])

    e = residuals(xi0).numpy()
    J = torch.autograd.functional.jacobian(residuals, xi0, vectorize=True, strategy="forward-mode").numpy()
    n = int(ok.sum())
    w = _weights(det["e_g"][ok], prm.huber_delta)
    if with_range:
        w = np.concatenate([w, prm.range_weight * _weights(det["e_r"][ok], prm.range_huber)])
    WJ = J * w[:, None]
    return dict(H=J.T @ WJ, b=WJ.T @ e, chi2=float((w * e * e).sum()), inliers=n,
                S=np.abs(WJ * e[:, None]).sum(0), gu=gu_np, gv=gv_np, e=e)
