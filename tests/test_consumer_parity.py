"""The loss stage's kernels (`sls_consumer_fwd_bwd`: consumer_b_kernel + consumer_c_kernel) against the float64
reference of tests/consumer_cases.py, pixel by pixel, on maps that hold the values at which the kernels branch
(alpha == 0 / 1 / 2^-20, s == gt, a zero-length stencil, lone valid and invalid pixels, images without an interior)
and at sizes from one pixel to 297 consumer blocks (kernel C's reduction over the partials makes a second trip).
The norm, the bars and where they come from: consumer_cases' header; the reference itself is checked on the CPU by
tests/test_consumer_math.py."""
import numpy as np
import pytest
import torch

import consumer_cases as cc

pytestmark = pytest.mark.gpu


def _tables(case, device):
    from splat_loam_amd.fused import camera_aux
    from splat_loam_amd.scene import Camera
    cam = Camera(case.K, case.gt[None], None, case.valid[None].astype(np.uint8), None, data_device=str(device))
    return cam, camera_aux(cam)


def _run(case, device, valid=None):
    """One sls_consumer_fwd_bwd on the case: (sums (4,) and dL/dallmap (7, H, W) as float32 arrays).  Both outputs are
    filled with NaN first: what comes back was written by the kernels."""
    from splat_loam_amd import _abi
    lib = _abi.lib()
    cam, aux = _tables(case, device)
    H, W = case.H, case.W
    am = torch.tensor(case.allmap, device=device)
    v = aux.valid if valid is None else torch.tensor(valid.astype(np.uint8), device=device)
    n_valid = int(v.sum().item())
    sums = torch.full((4,), float("nan"), dtype=torch.float32, device=device)
    grad = torch.full((7, H, W), float("nan"), dtype=torch.float32, device=device)
    nbytes = int(lib.sls_consumer_scratch_bytes(H, W))
    assert nbytes >= 48 * H * W + 12 * ((W + 63) // 64) * ((H + 3) // 4)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    _abi.check(lib.sls_consumer_fwd_bwd(H, W, am.data_ptr(), aux.gt.data_ptr(), v.data_ptr(), aux.col_h.data_ptr(),
                                        aux.row_h.data_ptr(), float(case.ratio), cc.LAMBDA_N, cc.LAMBDA_A, n_valid,
                                        sums.data_ptr(), grad.data_ptr(), scratch.data_ptr(), nbytes,
                                        torch.cuda.current_stream(device).cuda_stream), "sls_consumer_fwd_bwd")
    torch.cuda.synchronize(device)
    return sums.cpu().numpy(), grad.cpu().numpy()


def _all_zero_bits(x):
    return not (x.view(np.uint32) & np.uint32(0x7FFFFFFF)).any()


def _check_grad(name, what, g, g_ref, case):
    """dL/dallmap `g` against `g_ref` by the norm of consumer_cases: the issue's look (no pixel out), the sharper look
    (the 2^-20 pixel out of scale and error) and the alpha == 0 pixels element by element."""
    H, W, ratio, alpha = case.H, case.W, case.ratio, case.allmap[1]
    errs = cc.plane_errors(g, g_ref, alpha)
    sharp = cc.plane_errors(g, g_ref, alpha, without=cc.stiff_pixels(case))
    a0 = cc.alpha0_errors(g, g_ref, alpha)
    bar, bar_sharp = cc.grad_bar(H, W, ratio), cc.grad_bar(H, W, ratio, sharp=True)
    print(f"\n[{name}] {what}: d32 {cc.d32(H, W, ratio):.2e} bar {bar:.2e}, planes {['%.1e' % e for e in errs]}; without the 2^-20 pixel: "
          f"d32 {cc.d32(H, W, ratio, True):.2e} bar {bar_sharp:.2e}, planes {['%.1e' % e for e in sharp]}; "
          f"alpha == 0 pixels {a0.max() if a0.size else 0.0:.1e}")
    assert np.isfinite(g).all()
    assert max(errs) <= bar, f"{name}: {what}: planes {errs} against a bar of {bar:.2e}"
    assert max(sharp) <= bar_sharp, f"{name}: {what}: planes {sharp} (the 2^-20 pixel left out) against a bar of {bar_sharp:.2e}"
    assert (a0 <= cc.ALPHA0_RTOL).all(), f"{name}: {what}: alpha == 0 pixels off by {a0.max():.2e}"


@pytest.mark.parametrize("H,W,ratio", cc.CASES, ids=cc.CASE_IDS)
def test_consumer_kernels_match_float64(device, H, W, ratio):
    case = cc.make_case(H, W, ratio)
    ref = cc.reference(H, W, ratio)
    sums, g = _run(case, device)
    sums2, g2 = _run(case, device)
    # kernel B writes partials, kernel C sums them in a fixed order: no same-address float atomics, the same bits every run
    assert np.array_equal(sums.view(np.uint32), sums2.view(np.uint32)) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))
    # the loss and its three sums, with their weights
    nv = case.n_valid
    got = (sums[0] / (H * W), cc.LAMBDA_N / nv * sums[1], cc.LAMBDA_A / nv * sums[2])
    print(f"\n[{case.name}] loss {sums[3]:.7f} vs {ref['loss']:.7f} ({abs(sums[3] - ref['loss']) / ref['loss']:.1e}); terms "
          + ", ".join(f"{abs(a - b) / abs(b):.1e}" for a, b in zip(got, ref["parts"])))
    assert abs(float(sums[3]) - ref["loss"]) <= cc.LOSS_RTOL * abs(ref["loss"])
    for a, b, what in zip(got, ref["parts"], ("geom", "normal", "alpha")):
        assert abs(float(a) - b) <= cc.LOSS_RTOL * abs(b), (what, float(a), b)
    # dL/dallmap, all seven planes
    _check_grad(case.name, "kernels vs float64", g, ref["grad"], case)
    # exact zeros, not small numbers: every bit but the sign clear (0 x ds carries the sign of ds, and IEEE's -0 is a zero)
    assert _all_zero_bits(g[6]), "plane 6 (distortion): 0 bit for bit"
    if ratio == 0.0:
        assert _all_zero_bits(g[5]), "plane 5 (median) at ratio 0: 0 bit for bit"
    if ratio == 1.0:
        assert _all_zero_bits(g[0]), "plane 0 (depth) at ratio 1: 0 bit for bit"
    # through autograd, as the mapper calls it, with an upstream gradient of 3
    from splat_loam_amd.fused import fused_pixel_loss
    from splat_loam_amd.mapping import MappingConfig
    cam, _ = _tables(case, device)
    am = torch.tensor(case.allmap, device=device).requires_grad_(True)
    loss = fused_pixel_loss(am, cam, MappingConfig(opt_lambda_alpha=cc.LAMBDA_A, opt_lambda_normal=cc.LAMBDA_N, depth_ratio=ratio))
    (3.0 * loss).backward()
    assert float(loss.detach()) == float(sums[3])
    assert np.array_equal(am.grad.cpu().numpy().view(np.uint32), (g * np.float32(3.0)).view(np.uint32))
    # the planted pixels, one by one
    if case.planted:
        p = case.planted
        r, c = p["alpha0_valid"]
        want = np.float32(cc.LAMBDA_A) * (np.float32(1.0) / np.float32(nv)) * np.float32(-1.0) / np.float32(1e-12)
        assert abs(float(g[1, r, c]) - float(want)) <= cc.ALPHA0_RTOL * abs(float(want))
        assert not g[2:5, r, c].any()
        r, c = p["alpha0_invalid"]
        assert not g[1:5, r, c].any()


def test_bce_backward_on_both_sides_of_its_clamp(device):
    """torch's BCE backward divides by max((1 - a) a, 1e-12).  alpha == 0 and alpha == 1 do not tell a maximum from a sum
    (0 + 1e-12 and max(0, 1e-12) are the same number), and at alpha = 2^-20 the 1e-12 is 1e-6 of the denominator.  So:
    pixels at alpha = 2^-39 (1.8e-12: the clamp is off), 2^-40 and 2^-41 (9.1e-13, 4.5e-13: it is on), every other plane
    0 there — no blended normal, no depth, so their alpha gradient is the BCE term alone, five float32 operations:
    element-wise at 1e-6, the bar of the alpha == 0 pixels.  On a copy of the 5x65 map (these values would be the whole
    scale of the alpha plane in the shared cases)."""
    from oracle.consumer_ref import pixel_loss64
    H, W, ratio = 5, 65, 0.0
    base = cc.make_case(H, W, ratio)
    am = base.allmap.copy()
    spots = {(2, 48): 2.0 ** -39, (2, 52): 2.0 ** -40, (2, 56): 2.0 ** -41}
    valid = base.valid.copy()
    for (r, c), a in spots.items():
        am[:, r, c] = 0.0
        am[1, r, c] = a
        valid[r, c] = True
    case = cc.Case(H, W, ratio, base.K, am, base.gt, valid)
    am64 = torch.tensor(am).double().requires_grad_(True)
    pixel_loss64(am64, case.K, case.gt, valid, ratio, cc.LAMBDA_N, cc.LAMBDA_A, bce="torch")[0].backward()
    g64 = am64.grad.numpy()
    _, g = _run(case, device)
    for (r, c), a in spots.items():
        want = cc.LAMBDA_A / case.n_valid * (a - 1.0) / max((1.0 - a) * a, float(np.float32(1e-12)))
        assert abs(g64[1, r, c] - want) <= 1e-12 * abs(want), "the reference: torch's backward, its 1e-12 a float32 constant"
        assert abs(float(g[1, r, c]) - g64[1, r, c]) <= cc.ALPHA0_RTOL * abs(g64[1, r, c]), (a, float(g[1, r, c]), g64[1, r, c])
    assert np.isfinite(g).all()


@pytest.mark.parametrize("H,W", [(3, 3), (40, 200)], ids=["3x3", "40x200"])
@pytest.mark.parametrize("ratio", cc.RATIOS, ids=[f"ratio{r:g}" for r in cc.RATIOS])
def test_no_valid_pixel(device, H, W, ratio):
    """n_valid == 0: torch's means over no pixel are NaN, so there is no reference; what launch_consumer documents for
    inv_nv = 0 is asserted — no normal term, no alpha term, no loss, and a gradient of zeros, bit for bit."""
    case = cc.make_case(H, W, ratio)
    sums, g = _run(case, device, valid=np.zeros((H, W), bool))
    assert sums[1] == 0.0 and sums[2] == 0.0, sums
    assert sums[3] == 0.0 and sums[0] == 0.0, sums
    assert _all_zero_bits(g), "dL/dallmap: all zeros, bit for bit"


@pytest.mark.parametrize("H,W", [(40, 200), (32, 256)], ids=["40x200", "32x256"])
@pytest.mark.parametrize("ratio", cc.RATIOS, ids=[f"ratio{r:g}" for r in cc.RATIOS])
def test_consumer_kernels_match_the_torch_path(device, H, W, ratio):
    """fused_pixel_loss against the product's float32 torch path on the device, mapping_loss(postprocess(...)) — pinned to
    the reference project by goldens G2 and G5 — under the same norm and bar."""
    case = cc.make_case(H, W, ratio)
    loss_t, g_t = cc.torch_path(case, device)
    sums, g = _run(case, device)
    assert abs(float(sums[3]) - loss_t) <= cc.LOSS_RTOL * abs(loss_t)
    _check_grad(case.name, "kernels vs the float32 torch path", g, g_t, case)
