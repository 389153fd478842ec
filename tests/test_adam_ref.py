"""The float64 Adam reference of tests/adam_ref.py against torch.optim.Adam in float64, its bounds against a NumPy float32
restatement of adam_one (the evidence that a correct float32 implementation reaches them with room to spare), and the
reference of sls_grad_compact's rows on an example written by hand.  No GPU."""
import numpy as np
import pytest
import torch

import adam_ref
from adam_ref import BETAS, EPSS, LRS, STEPS

CONFIGS = [(b, e) for b in BETAS for e in EPSS]


@pytest.mark.parametrize("betas,eps", CONFIGS)
def test_adam_step64_is_torch_adam_in_float64(betas, eps):
    """Four tensors, one per learning rate, through steps 1-4 and step 1000 from the step-4 state; both sides free-running
    in float64 from the same float32 inputs.  1e-12 relative — to the operands: |p| + |step| for p (a step may cancel the
    parameter), |m| + |g| for m (as the float32 bound), the result for v (positive terms).  Float64 leaves 1e-16 per
    operation and the two sides differ in the order of a handful of them."""
    rng = np.random.default_rng(11)
    n = 4001
    p0 = [adam_ref.make_params(rng, n) for _ in LRS]
    tp = [torch.tensor(p.astype(np.float64), requires_grad=True) for p in p0]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(tp, LRS)], lr=0.0, betas=betas, eps=eps, foreach=False)
    state = [(p.astype(np.float64), np.zeros(n), np.zeros(n)) for p in p0]
    worst = 0.0
    for t in STEPS:
        if t == 1000:
            for p in tp:
                opt.state[p]["step"].fill_(999.0)
        for k, (p, lr) in enumerate(zip(tp, LRS)):
            g = adam_ref.make_grads(rng, n)
            p.grad = torch.tensor(g.astype(np.float64))
            before = state[k]
            state[k] = adam_ref.adam_step64(before[0], g, before[1], before[2], lr, betas[0], betas[1], eps, t)
            state[k] = state[k] + (np.abs(before[0]) + np.abs(state[k][0] - before[0]), np.abs(before[1]) + np.abs(g))
        opt.step()
        for k, p in enumerate(tp):
            st = opt.state[p]
            assert int(st["step"]) == t
            p1, m1, v1, scale_p, scale_m = state[k]
            for got, ref, scale in ((p.detach().numpy(), p1, scale_p), (st["exp_avg"].numpy(), m1, scale_m),
                                    (st["exp_avg_sq"].numpy(), v1, v1)):
                bad = np.abs(got - ref) > 1e-12 * scale
                assert not bad.any(), (t, k, int(bad.sum()), got[bad][:3], ref[bad][:3])
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(scale > 0, np.abs(got - ref) / scale, 0.0))))
            state[k] = (p1, m1, v1)
    print(f"\n[adam_step64 vs torch float64] betas {betas} eps {eps}: worst relative difference {worst:.2e}")


@pytest.mark.parametrize("betas,eps", CONFIGS)
def test_float32_restatement_stays_inside_half_the_bounds(betas, eps):
    """adam_one restated in NumPy float32, chained from its own float32 state as the device tests chain from the device's:
    2 M elements, every step setting, the four learning rates side by side.  Worst error / tolerance <= 0.5.

    Measured (the same at both eps to two digits):   betas (0.9, 0.999)  p 0.250  m 0.494  v 0.455
                                                     betas (0.5, 0.9)    p 0.250  m 0.375  v 0.358
                                                     betas (0.0, 0.99)   p 0.250  m 0.000  v 0.388
    With m + (g - m) * w1 at every beta1 (adam_one's form before this test) the last line read p 0.470, m 1.000: at
    beta1 = 0 float64 gives m' = g exactly, while g - m rounds in the binade above g's and the sum lands one ulp of g
    beside it.  adam_one and this restatement now take torch's other lerp form, g - (g - m) * beta1, from 1 - beta1 = 0.5
    on; below it (beta1 = 0.9, what the project runs) the operations and the bits are the ones they were."""
    rng = np.random.default_rng(5)
    n = 2_000_000
    lr = np.resize(np.asarray(LRS, np.float64), n)
    state = (adam_ref.make_params(rng, n), np.zeros(n, np.float32), np.zeros(n, np.float32))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for t in STEPS:
        g = adam_ref.make_grads(rng, n)
        after = adam_ref.adam_one32(state[0], g, state[1], state[2], lr, betas[0], betas[1], eps, t)
        for key, (r, _) in adam_ref.adam_ratios(state, g, after, lr, betas[0], betas[1], eps, t).items():
            worst[key] = max(worst[key], r)
        state = after
    print(f"\n[adam error / tolerance] NumPy float32 adam_one, betas {betas} eps {eps}: {worst}")
    assert max(worst.values()) <= 0.5, worst


def test_bounds_notice_a_wrong_learning_rate_and_a_wrong_moment():
    """What the bounds are for: one element in 100 k stepped with its neighbour group's learning rate, or one moment
    decayed with the other beta, lies outside them."""
    rng = np.random.default_rng(2)
    n = 100_000
    b1, b2, eps, t = 0.9, 0.999, 1e-15, 3
    before = (adam_ref.make_params(rng, n), adam_ref.make_grads(rng, n) * np.float32(0.1), adam_ref.make_grads(rng, n) ** 2)
    g = adam_ref.make_grads(rng, n)
    g[77] = 3.0
    good = adam_ref.adam_one32(*((before[0], g) + before[1:]), 5e-3, b1, b2, eps, t)
    assert all(r <= 0.5 for r, _ in adam_ref.adam_ratios(before, g, good, 5e-3, b1, b2, eps, t).values())
    other_lr = adam_ref.adam_one32(*((before[0], g) + before[1:]), 1e-3, b1, b2, eps, t)
    p = good[0].copy(); p[77] = other_lr[0][77]
    r, i = adam_ref.adam_ratios(before, g, (p, good[1], good[2]), 5e-3, b1, b2, eps, t)["p"]
    assert i == 77 and r > 100.0, (r, i)        # (four fifths of a step against 1e-5 of it and two ulps)
    m = good[1].copy(); m[77] = np.float32(b2 * before[1][77] + (1 - b2) * 3.0)
    r, i = adam_ref.adam_ratios(before, g, (good[0], m, good[2]), 5e-3, b1, b2, eps, t)["m"]
    assert i == 77 and r > 100.0, (r, i)


def test_compact_rows_on_a_hand_written_example():
    N = 3
    flat = np.arange(30, dtype=np.float32)      # xyz 0-8 | opacity 9-11 | scaling 12-17 | rotation 18-29
    rows = adam_ref.compact_rows(N, [True, False, True], flat)
    assert rows.dtype == np.float32
    assert rows.tolist() == [[0, 1, 2, 9, 12, 13, 18, 19, 20, 21],
                             [6, 7, 8, 11, 16, 17, 26, 27, 28, 29]]
    assert adam_ref.compact_rows(N, [False, True, False], flat).tolist() == [[3, 4, 5, 10, 14, 15, 22, 23, 24, 25]]
    assert adam_ref.compact_rows(N, [False] * 3, flat).shape == (0, 10)
    # the vectorised layout helpers of the GPU tests agree with it, both ways
    assert np.array_equal(adam_ref.surfel_rows(N, flat), adam_ref.compact_rows(N, [True] * 3, flat))
    assert np.array_equal(adam_ref.flat_from_rows(N, adam_ref.surfel_rows(N, flat)), flat)
    assert adam_ref.flat_lr(2).tolist() == [5e-4] * 6 + [5e-2] * 2 + [5e-3] * 4 + [1e-3] * 8
    assert adam_ref.pack_bitmap(70, [i in (0, 63, 64, 69) for i in range(70)], 4).tolist() == [1 | 1 << 63, 1 | 1 << 5, 0, 0]
