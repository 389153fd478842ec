"""Hand-built `allmap`s for the loss stage (csrc/sls_consumer.hip, sls_consumer_dev.hpp) and its float64 reference.

A rendered image never holds the values at which the stage branches, so these are built by hand: a smooth base (the
inside of a sphere seen from the origin) with the branch values planted into it.  The map is built in float64 and
rounded to float32 ONCE: the kernels, the product's torch path and the reference (in either precision) all read the
same float32 numbers.

Reference: oracle/consumer_ref.pixel_loss64 with the alpha term through F.binary_cross_entropy — the expression of
slam/mapper.py:182-187, whose backward the kernel copies at alpha == 0 and alpha == 1 — under autograd, in float64;
the same text in float32 says what float32 arithmetic itself costs on a case (`d32`).

Norm for dL/dallmap (`plane_errors`): per plane max |g - g64| / max |g64|.  One exception, the alpha plane: a valid
pixel with alpha == 0 carries lambda_a 1e12 / n_valid and would set that plane's scale to 1e7..1e9, blinding the check
everywhere else; so scale and error of the alpha plane are taken over the pixels with alpha > 0, and the alpha == 0
pixels are compared element by element (`ALPHA0_RTOL`).  No pixel is left out.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass, field

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAMBDA_N, LAMBDA_A = 0.5, 0.4          # MappingConfig's defaults (configs/kitti/kitti-00-odom.yaml:18-21)
RATIOS = (0.0, 0.3, 1.0)
# shape -> (hfov, vfov) in degrees
SHAPES = {
    (1, 1): (120.0, 30.0), (2, 5): (120.0, 30.0),       # no interior
    (3, 3): (120.0, 30.0),                              # one interior pixel
    (5, 65): (120.0, 30.0),                             # one live column in the second block, one live row in the second block row
    (9, 131): (360.0, 30.0),                            # ragged, wraps
    (40, 200): (120.0, 30.0),
    (32, 256): (360.0, 27.0),
    (132, 513): (360.0, 90.0),                          # 33 x 9 = 297 blocks: kernel C's reduction makes a second trip
}
CASES = [(H, W, ratio) for (H, W) in SHAPES for ratio in RATIOS]
CASE_IDS = [f"{H}x{W}-ratio{ratio:g}" for (H, W, ratio) in CASES]

GRAD_FLOOR = 1e-5       # the project's bar; a case whose float32 reference is further from float64 gets 3 x that distance
GRAD_CAP = 1e-3         # ... and no case may need more than this
LOSS_RTOL = 2e-6        # the float32 reference's loss is within ~1e-7 of float64; the kernel sums up to 297 partials in another order
ALPHA0_RTOL = 1e-6      # the kernel's value at a valid alpha == 0 pixel is two float32 operations
MARGIN = 1e-5           # |s - gt| > MARGIN gt at every valid pixel but the deliberate tie: no sign decided by rounding


@dataclass
class Case:
    H: int
    W: int
    ratio: float
    K: np.ndarray                  # (3, 3) float32
    allmap: np.ndarray             # (7, H, W) float32
    gt: np.ndarray                 # (H, W) float32
    valid: np.ndarray              # (H, W) bool
    planted: dict = field(default_factory=dict)     # name -> (r, c)

    @property
    def n_valid(self):
        return int(self.valid.sum())

    @property
    def name(self):
        return f"{self.H}x{self.W}-ratio{self.ratio:g}"


def _surf_depth64(am, ratio):
    al = am[1].astype(np.float64)
    d = np.where(al > 0, am[0].astype(np.float64) / np.where(al > 0, al, 1.0), am[0].astype(np.float64))
    return d * (1.0 - ratio) + am[5].astype(np.float64) * ratio


@functools.lru_cache(maxsize=None)
def make_case(H: int, W: int, ratio: float) -> Case:
    from oracle.consumer_ref import pixel_rays64
    from splat_loam_amd import synth
    hfov, vfov = SHAPES[(H, W)]
    K = synth.spherical_K(H, W, -vfov / 2, vfov / 2, hfov)
    rng = np.random.default_rng(1000 * H + W)          # (the same base map at the three ratios)
    rays = pixel_rays64(torch.tensor(K), H, W).numpy()                                   # (H, W, 3)
    centre, radius = np.array([1.0, -0.7, 0.3]), 6.0
    b = rays @ centre
    s = b + np.sqrt(b * b - centre @ centre + radius * radius)                          # range to the sphere, from inside
    n = (centre - s[..., None] * rays) / radius                                         # unit, towards the centre
    if H >= 3 and W >= 3:                                                               # ... signed as the stencil's normal
        P = s[..., None] * rays
        cr = np.cross(P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2])
        if (cr * n[1:-1, 1:-1]).sum() < 0:
            n = -n
    alpha = rng.uniform(0.05, 0.98, (H, W))
    sign = np.where(rng.random((H, W)) < 0.5, -1.0, 1.0)
    noise = rng.uniform(0.005, 0.04, (H, W))
    valid = rng.random((H, W)) < 0.9
    am = np.zeros((7, H, W), np.float64)
    am[0] = s * alpha
    am[1] = alpha
    am[2:5] = (alpha[..., None] * n).transpose(2, 0, 1)
    am[5] = s * (1.0 + 1e-3 * np.sin(0.1 * np.arange(W)))[None, :]
    am[6] = rng.uniform(0.0, 0.1, (H, W))              # (the distortion plane: read by nobody, its gradient is 0)
    # valid pixels in the four corners and on each border
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        valid[r, c] = True
    planted = {}
    tie_alpha = 0.5
    if H >= 5 and W >= 65:
        r0 = H // 2                                     # interior, and so are its neighbours

        def pixel(c, al, ok):
            am[0, r0, c] = s[r0, c] * al
            am[1, r0, c] = al
            am[2:5, r0, c] = al * n[r0, c]
            valid[r0, c] = ok

        planted["alpha0_valid"] = (r0, 3)               # a measurement the model does not reach: all seven planes 0
        am[:, r0, 3] = 0.0
        valid[r0, 3] = True
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):     # ... inside four valid neighbours' stencils
            valid[r0 + dr, 3 + dc] = True
        planted["alpha0_invalid"] = (r0, 8)
        am[:, r0, 8] = 0.0
        valid[r0, 8] = False
        planted["alpha1"] = (r0, 13)
        pixel(13, 1.0, True)
        planted["alpha_tiny"] = (r0, 18)
        pixel(18, 2.0 ** -20, True)
        if ratio in (0.0, 1.0):                         # (at any other ratio s is rounded differently in the two precisions)
            planted["tie"] = (r0, 23)
            pixel(23, tie_alpha, True)
        planted["zero_stencil"] = (r0, 29)              # a 3 x 3 patch at the origin: its centre's cross product is exactly 0
        am[0, r0 - 1:r0 + 2, 28:31] = 0.0
        am[5, r0 - 1:r0 + 2, 28:31] = 0.0
        valid[r0 - 1:r0 + 2, 28:31] = True
        # (the four pixels next to the centre have a zero-length stencil too, with ONE difference zero: valid, their adjoint
        #  (g / 1e-12) x u is ~1e4 and would be the whole scale of the depth plane, blinding it everywhere else — invalid)
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            valid[r0 + dr, 29 + dc] = False
        planted["valid_alone"] = (r0, 36)
        valid[r0, 36] = True
        planted["invalid_alone"] = (r0, 42)
        valid[r0 - 1:r0 + 2, 41:44] = True
        valid[r0, 42] = False
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            valid[r0 + dr, 36 + dc] = False
    am32 = am.astype(np.float32)                        # rounded ONCE
    s32 = _surf_depth64(am32, ratio)                    # the surface depth of the rounded map
    base = np.where(s32 > 0, s32, s)                    # (the pixels planted at the origin: a target at the base surface)
    gt = (base * (1.0 + sign * noise)).astype(np.float32)
    if "tie" in planted:
        r, c = planted["tie"]
        # D = s alpha with alpha a power of two: D / alpha is exact in both precisions; at ratio 1 s is the median itself
        gt[r, c] = am32[0, r, c] / np.float32(tie_alpha) if ratio == 0.0 else am32[5, r, c]
    return Case(H, W, ratio, K, am32, gt, valid, planted)


@functools.lru_cache(maxsize=None)
def reference(H: int, W: int, ratio: float, dtype=torch.float64):
    """The reference on a case: {"loss", "parts" (geom, normal, alpha, lambdas applied), "grad" (7, H, W) float64 array,
    "part_grads" (3, 7, H, W): the gradient of each term alone}.  Computed once per case and precision; read-only."""
    from oracle.consumer_ref import pixel_loss64
    case = make_case(H, W, ratio)
    am = torch.tensor(case.allmap).to(dtype).requires_grad_(True)
    total, geom, normal, bce = pixel_loss64(am, case.K, case.gt, case.valid, ratio, LAMBDA_N, LAMBDA_A, dtype=dtype, bce="torch")
    part_grads = [torch.autograd.grad(t, am, retain_graph=True, allow_unused=True)[0] for t in (geom, normal, bce)]
    part_grads = [torch.zeros_like(am) if g is None else g for g in part_grads]
    (grad,) = torch.autograd.grad(total, am)
    out = {"loss": float(total.detach()), "parts": tuple(float(t.detach()) for t in (geom, normal, bce)),
           "grad": grad.double().numpy(), "part_grads": torch.stack(part_grads).double().numpy()}
    for v in (out["grad"], out["part_grads"]):
        v.setflags(write=False)
    return out


def plane_errors(g, g64, alpha, without=None):
    """Per plane max |g - g64| / max |g64|; the alpha plane over the pixels with alpha > 0 (see the module's header).
    A plane the reference leaves at zero everywhere is compared at a scale of 1 (it has to be zero: checked bit for
    bit where the kernel says so).  `without`: a second, sharper look with these pixels out of scale AND error."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    errs = []
    for c in range(7):
        sel = (alpha > 0) if c == 1 else np.ones(alpha.shape, bool)
        if without is not None:
            sel = sel & ~without
        if not sel.any():
            errs.append(0.0)
            continue
        scale = np.abs(g64[c][sel]).max()
        errs.append(float(np.abs(g[c][sel] - g64[c][sel]).max() / (scale if scale > 0 else 1.0)))
    return errs


def alpha0_errors(g, g64, alpha):
    """Element-wise relative error of the alpha plane at the pixels with alpha == 0 (0 where the reference is 0 too)."""
    sel = alpha == 0
    a, b = np.asarray(g, np.float64)[1][sel], np.asarray(g64, np.float64)[1][sel]
    return np.where(b != 0, np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0), np.abs(a))


def stiff_pixels(case: Case):
    """The planted pixel with alpha = 2^-20: the divisions by alpha make its depth and normal gradients 1e6 times its
    neighbours', so it IS those planes' scale in the norm above.  The sharper look takes it out of scale and error: the
    rest of the image is then judged at its own scale (the pixel itself stays in the first look)."""
    m = np.zeros((case.H, case.W), bool)
    if "alpha_tiny" in case.planted:
        m[case.planted["alpha_tiny"]] = True
    return m


@functools.lru_cache(maxsize=None)
def d32(H: int, W: int, ratio: float, sharp: bool = False) -> float:
    """What float32 arithmetic itself costs on the case: the reference's float32 run against its float64 run, worst
    plane, under the norm of `plane_errors`.  From the reference alone, never from the code under test."""
    case = make_case(H, W, ratio)
    return max(plane_errors(reference(H, W, ratio, torch.float32)["grad"], reference(H, W, ratio)["grad"], case.allmap[1],
                            without=stiff_pixels(case) if sharp else None))


def grad_bar(H: int, W: int, ratio: float, sharp: bool = False) -> float:
    """max(1e-5, 3 d32): the rule of tests/test_aligner_parity.py.  The stencil amplifies float32 rounding by about
    1 / (2 pixel pitch); the margin of 3 covers another, equally valid order of the same float32 operations."""
    bar = max(GRAD_FLOOR, 3.0 * d32(H, W, ratio, sharp))
    assert bar <= GRAD_CAP, f"{H}x{W} ratio {ratio}: a bar of {bar:.2e} is no check"
    return bar


def torch_path(case: Case, device="cpu"):
    """The product's torch path in float32, mapping_loss(postprocess(cam, allmap, ratio)) with the regulariser off —
    pinned to the reference project by goldens G2 and G5: (loss, dL/dallmap as a float64 array)."""
    from splat_loam_amd.mapping import MappingConfig, mapping_loss
    from splat_loam_amd.renderer import postprocess
    from splat_loam_amd.scene import Camera, SurfelModel
    cam = Camera(case.K, case.gt[None], None, case.valid[None].astype(np.uint8), None, data_device=str(device))
    cfg = MappingConfig(opt_lambda_alpha=LAMBDA_A, opt_lambda_normal=LAMBDA_N, depth_ratio=case.ratio, opt_scaling_max_penalty=0.0)
    model = SurfelModel.from_activated(np.zeros((1, 3), np.float32), np.full((1, 2), 0.01, np.float32),
                                       np.array([[1.0, 0, 0, 0]], np.float32), np.array([0.5], np.float32), device=str(device))
    am = torch.tensor(case.allmap, device=device).requires_grad_(True)
    loss = mapping_loss(postprocess(cam, am, case.ratio), cam, model, cfg)
    (grad,) = torch.autograd.grad(loss, am)
    return float(loss.detach()), grad.double().cpu().numpy()
