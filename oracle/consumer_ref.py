"""float64 restatement of the allmap CONSUMER: render()'s post-processing, the
spherical back-projection with central-difference normals, and the pixel terms
of the mapper's loss.  TEST INFRASTRUCTURE (see sls_oracle.c's header): imported
by tests/ only; the product's consumer is csrc/sls_consumer.hip.

Why a float64 version exists beside splat_loam_amd/renderer.py (float32 torch,
pinned to the reference by G1/G2/G5): the normal-consistency term differentiates
the back-projected range image with a 2-pixel stencil, so a relative
perturbation eps of `allmap` is amplified by ~1/(2*pixel pitch) ~ 1/0.006 before
it reaches dL/dallmap.  Two float32 evaluations of the same formulas differ by
~1e-4 there; the float64 evaluation is the common truth both are compared with.

Follows, line by line:
  gaussian_renderer/__init__.py:51-82   alpha mask, normal / depth division, surf_depth, surf_normal *= alpha
  utils/graphic_utils.py:26-66          depth_to_points, pixel (c, r) at image coordinate (c - 0.5, r - 0.5)
  utils/graphic_utils.py:69-88          depth_to_normal: normalize(cross(P[r+1]-P[r-1], P[c+1]-P[c-1])), 0 on the border
  slam/mapper.py:158-187                geom_l1 (mean over ALL pixels), normal loss and BCE (means over valid pixels)
"""
from __future__ import annotations

import torch


def pixel_rays64(K: torch.Tensor, H: int, W: int, dtype=torch.float64) -> torch.Tensor:
    """(H, W, 3) unit rays of the sensor frame (float64 unless `dtype` says otherwise), pixel (c, r) at (c - 0.5, r - 0.5)."""
    Kinv = torch.linalg.inv(K.to(dtype))
    xs = torch.arange(W, dtype=dtype) - 0.5
    ys = torch.arange(H, dtype=dtype) - 0.5
    gx, gy = xs[None, :].expand(H, W), ys[:, None].expand(H, W)
    az = Kinv[0, 0] * gx + Kinv[0, 1] * gy + Kinv[0, 2]
    el = Kinv[1, 0] * gx + Kinv[1, 1] * gy + Kinv[1, 2]
    ce = torch.cos(el)
    return torch.stack([torch.cos(az) * ce, torch.sin(az) * ce, torch.sin(el)], dim=-1)


def pixel_loss64(allmap: torch.Tensor, K, gt_depth, valid, depth_ratio=0.0, lambda_normal=0.5, lambda_alpha=0.4,
                 dtype=torch.float64, bce="clamped-log"):
    """allmap (7,H,W) float64 (requires_grad allowed) -> (total, geom_l1, normal_loss, alpha_loss) with the lambdas
    applied.  `valid` is the (H,W) bool mask `image_valid[0] == 1`, `gt_depth` (H,W).  The loss is invariant to
    the sensor pose (both normals are rotated by the same matrix), so everything stays in the sensor frame.
    `dtype`: the same text in another precision (float32: what float32 arithmetic itself costs on an image).
    `bce`: "clamped-log" writes the alpha term as -clamp(log a), the value of torch's BCE at target 1; "torch" calls
    F.binary_cross_entropy as slam/mapper.py:182-187 does — the same value, and torch's backward at the two ends of
    [0, 1]: (a - 1) / max((1 - a) a, 1e-12), i.e. -1e12 at a == 0 and 0 at a == 1, where the clamped log has NaN and -1."""
    assert allmap.dtype == dtype and bce in ("clamped-log", "torch")
    _, H, W = allmap.shape
    K = torch.as_tensor(K).to(dtype).reshape(3, 3)
    gt = torch.as_tensor(gt_depth).to(dtype).reshape(H, W)
    valid = torch.as_tensor(valid).reshape(H, W).bool()
    alpha = allmap[1]
    hit = alpha > 0.0
    safe = torch.where(hit, alpha, torch.ones_like(alpha))
    n_hat = torch.where(hit[None], allmap[2:5] / safe[None], allmap[2:5])
    d_exp = torch.where(hit, allmap[0] / safe, allmap[0])
    surf_depth = d_exp * (1.0 - depth_ratio) + allmap[5] * depth_ratio
    pts = (surf_depth[..., None] * pixel_rays64(K, H, W, dtype)).permute(2, 0, 1)           # (3,H,W)
    d_row = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    d_col = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    n_surf = torch.zeros((3, H, W), dtype=dtype)
    n_surf[:, 1:-1, 1:-1] = torch.nn.functional.normalize(torch.cross(d_row, d_col, dim=0), dim=0)
    n_surf = n_surf * alpha[None]
    geom = torch.abs(valid * (surf_depth - gt)).mean()
    normal = (1.0 - (n_hat[:, valid] * n_surf[:, valid]).sum(dim=0)).mean() * lambda_normal
    a = alpha[valid]
    if bce == "torch":
        bce = torch.nn.functional.binary_cross_entropy(a, torch.ones_like(a), reduction="mean") * lambda_alpha
    else:
        bce = -(torch.clamp(torch.log(a), min=-100.0)).mean() * lambda_alpha           # target 1: torch's BCE clamps the log
    return geom + normal + bce, geom, normal, bce
