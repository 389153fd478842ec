"""The loss stage's float64 reference, checked on the CPU before any kernel is compared with it
(tests/test_consumer_parity.py): it agrees with the product's torch path — which goldens G2 and G5 pin to the
reference project — it is finite on every hand-built map, it takes the documented value at every planted pixel, and
the bar it gives each case is a check."""
import numpy as np
import pytest
import torch

import consumer_cases as cc

CASES = pytest.mark.parametrize("H,W,ratio", cc.CASES, ids=cc.CASE_IDS)
PLANTED = pytest.mark.parametrize("H,W,ratio", [c for c in cc.CASES if c[0] >= 5 and c[1] >= 65],
                                  ids=[i for c, i in zip(cc.CASES, cc.CASE_IDS) if c[0] >= 5 and c[1] >= 65])


@CASES
def test_cases_hold_what_they_claim(H, W, ratio):
    """The margins of the builder: no |s - gt| near zero by accident (a sign decided by rounding moves the depth plane by
    its whole scale), the planted values are there after the rounding to float32, and the shapes reach what they are for."""
    case = cc.make_case(H, W, ratio)
    am, valid = case.allmap, case.valid
    assert am.dtype == np.float32 and case.gt.dtype == np.float32 and case.n_valid > 0 and (case.gt > 0).all()
    s64 = cc._surf_depth64(am, ratio)
    tie = np.zeros((H, W), bool)
    if "tie" in case.planted:
        tie[case.planted["tie"]] = True
        assert s64[tie][0] == float(case.gt[tie][0]) and valid[tie][0], "the tie: s == gt bit for bit"
    m = np.abs(s64 - case.gt.astype(np.float64))
    assert (m > cc.MARGIN * case.gt)[valid & ~tie].all(), f"a valid pixel within {cc.MARGIN} of its target"
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        assert valid[r, c]
    if H >= 5 and W >= 65:
        p = case.planted
        for name, (r, c) in p.items():
            assert 2 <= r < H - 2 and 2 <= c < W - 2, f"{name}: interior, and so are its neighbours"
        four = lambda r, c: [(r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)]
        r, c = p["alpha0_valid"]
        assert not am[:, r, c].any() and valid[r, c] and all(valid[q] for q in four(r, c))
        r, c = p["alpha0_invalid"]
        assert not am[:, r, c].any() and not valid[r, c]
        assert am[1][p["alpha1"]] == 1.0 and valid[p["alpha1"]]
        assert am[1][p["alpha_tiny"]] == 2.0 ** -20 and valid[p["alpha_tiny"]]
        r, c = p["zero_stencil"]
        assert not am[0, r - 1:r + 2, c - 1:c + 2].any() and not am[5, r - 1:r + 2, c - 1:c + 2].any()
        assert valid[r, c] and am[1, r, c] > 0 and am[2:5, r, c].any() and not any(valid[q] for q in four(r, c))
        r, c = p["valid_alone"]
        assert valid[r, c] and not any(valid[q] for q in four(r, c))
        r, c = p["invalid_alone"]
        assert not valid[r, c] and all(valid[q] for q in four(r, c))
        assert ("tie" in p) == (ratio in (0.0, 1.0))
    else:
        assert not case.planted
    blocks = ((W + 63) // 64) * ((H + 3) // 4)
    if (H, W) == (132, 513):
        assert blocks == 297 > 256, "kernel C's reduction over the partials makes a second trip"
    if (H, W) == (5, 65):
        assert (W - 1) // 64 == 1 and W % 64 == 1 and (H - 1) // 4 == 1 and H % 4 == 1


@CASES
def test_reference_matches_the_torch_path(H, W, ratio):
    """The float64 reference against mapping_loss(postprocess(...)) in float32, by the rule the kernels are judged by;
    and the reference's own float32 run reproduces that deviation to its order: the torch path's distance from float64
    is what float32 costs, not a difference of formulas."""
    case = cc.make_case(H, W, ratio)
    ref = cc.reference(H, W, ratio)
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all() and np.isfinite(ref["part_grads"]).all()
    loss, grad = cc.torch_path(case)
    assert np.isfinite(grad).all()
    d32, bar = cc.d32(H, W, ratio), cc.grad_bar(H, W, ratio)
    assert 3.0 * d32 <= cc.GRAD_CAP
    errs = cc.plane_errors(grad, ref["grad"], case.allmap[1])
    a0 = cc.alpha0_errors(grad, ref["grad"], case.allmap[1])
    print(f"\n[{case.name}] d32 {d32:.2e} bar {bar:.2e}; torch path: planes {['%.1e' % e for e in errs]}, "
          f"alpha == 0 pixels {a0.max() if a0.size else 0.0:.1e}, loss {abs(loss - ref['loss']) / abs(ref['loss']):.1e}")
    assert abs(loss - ref["loss"]) <= cc.LOSS_RTOL * abs(ref["loss"])
    assert max(errs) <= bar, (errs, bar)
    assert (a0 <= cc.ALPHA0_RTOL).all()
    # (below 1e-6 both are a handful of float32 roundings of a single pixel: no order to compare)
    floor = 1e-6
    assert 0.1 <= max(max(errs), floor) / max(d32, floor) <= 10.0, (max(errs), d32)
    assert not ref["grad"][6].any(), "nobody reads the distortion plane"
    if ratio == 0.0:
        assert not ref["grad"][5].any()
    if ratio == 1.0:
        assert not ref["grad"][0].any()


@PLANTED
def test_reference_at_the_planted_pixels(H, W, ratio):
    case = cc.make_case(H, W, ratio)
    ref, p = cc.reference(H, W, ratio), case.planted
    g, (g_geom, g_normal, g_bce) = ref["grad"], ref["part_grads"]
    # alpha == 0 at a valid pixel: torch's BCE backward, (a - 1) / max((1 - a) a, 1e-12); the normal term adds
    # k <n_hat, n_surf> = 0, the blended normal being 0 there; nothing comes back through the divisions (alpha > 0 is false)
    # (torch holds that 1e-12 as a float32 constant in either precision, 4e-9 below 1e-12 — and so does the kernel)
    want = -cc.LAMBDA_A / float(np.float32(1e-12)) / case.n_valid
    assert abs(want + cc.LAMBDA_A * 1e12 / case.n_valid) <= 1e-8 * abs(want)
    assert abs(g[1][p["alpha0_valid"]] - want) <= 1e-12 * abs(want)
    assert g_normal[1][p["alpha0_valid"]] == 0.0
    # (its depths do: the neighbours' stencils read its point)
    assert not g[1:5, p["alpha0_invalid"][0], p["alpha0_invalid"][1]].any(), "an invalid pixel's alpha and normals carry no gradient"
    assert g_bce[1][p["alpha1"]] == 0.0, "alpha == 1: the BCE part is 0, not the -1 of a clamped log"
    a = 2.0 ** -20
    want = cc.LAMBDA_A / case.n_valid * (a - 1.0) / ((1.0 - a) * a)
    assert abs(g_bce[1][p["alpha_tiny"]] - want) <= 1e-12 * abs(want)
    if "tie" in p:
        r, c = p["tie"]
        assert not g_geom[:, r, c].any(), "s == gt: sign 0, the geometric term contributes nothing"
    # the zero-length stencil: n_surf is 0 there, so the pixel's normal term is exactly 1 / n_valid of lambda_n ...
    r, c = p["zero_stencil"]
    from oracle.consumer_ref import pixel_loss64, pixel_rays64
    P = cc._surf_depth64(case.allmap, ratio)[..., None] * pixel_rays64(torch.tensor(case.K), H, W).numpy()
    assert not np.cross(P[r + 1, c] - P[r - 1, c], P[r, c + 1] - P[r, c - 1]).any()
    assert not g_normal[2:5, r, c].any() and g_normal[1, r, c] == 0.0, "d/dN and d/dalpha of alpha <N / alpha, 0>"
    # ... and its adjoint takes normalize's `g / eps` branch: v x (g / eps) with v = 0, zero, not NaN.  Against a central
    # difference of the float64 loss in the eight neighbouring depths; the branch holds at any step (moving one neighbour
    # leaves the other difference at exactly 0).  Step 1e-3 on depths of ~6: truncation ~(h / s)^2 = 3e-8 of the
    # derivative, rounding ~1e-16 / h of a loss of ~1 against gradients of >= 1e-5: 1e-8.  Bar 1e-6 of the largest.
    h = 1e-3
    planes = ([0] if ratio < 1.0 else []) + ([5] if ratio > 0.0 else [])

    def loss_at(plane, rr, cc_, step):
        am = torch.tensor(case.allmap).double()
        am[plane, rr, cc_] += step
        return float(pixel_loss64(am, case.K, case.gt, case.valid, ratio, cc.LAMBDA_N, cc.LAMBDA_A, bce="torch")[0])

    fd, ad = [], []
    for plane in planes:
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr == 0 and dc == 0:
                    continue
                fd.append((loss_at(plane, r + dr, c + dc, h) - loss_at(plane, r + dr, c + dc, -h)) / (2 * h))
                ad.append(g[plane, r + dr, c + dc])
    fd, ad = np.array(fd), np.array(ad)
    assert np.abs(ad).max() > 0
    assert np.abs(fd - ad).max() <= 1e-6 * np.abs(ad).max(), (fd, ad)


def test_existing_callers_of_the_reference_see_no_change():
    """pixel_loss64's defaults are what they were: float64, the alpha term as the clamped log — same value as torch's
    BCE, to the last bits, on a map with alpha inside (0, 1)."""
    from oracle.consumer_ref import pixel_loss64
    case = cc.make_case(3, 3, 0.3)
    am = torch.tensor(case.allmap).double()
    a = pixel_loss64(am, case.K, case.gt, case.valid, 0.3, cc.LAMBDA_N, cc.LAMBDA_A)
    b = pixel_loss64(am, case.K, case.gt, case.valid, 0.3, cc.LAMBDA_N, cc.LAMBDA_A, dtype=torch.float64, bce="torch")
    assert all(x.dtype == torch.float64 for x in a)
    assert all(abs(float(x) - float(y)) <= 1e-15 * abs(float(y)) for x, y in zip(a, b))
    with pytest.raises(AssertionError):
        pixel_loss64(am.float(), case.K, case.gt, case.valid)
