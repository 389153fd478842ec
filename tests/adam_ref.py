"""Float64 reference of the library's one Adam update rule (adam_one, sls_common.hpp) with DERIVED float32 bounds, the
inputs every Adam test shares, a NumPy float32 restatement of adam_one, and the reference of sls_grad_compact's rows.

The rule (torch.optim.Adam without weight decay or amsgrad), on float32 inputs widened to float64:

    m' = b1 m + (1 - b1) g
    v' = b2 v + (1 - b2) g^2
    p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

Tests chain ONE step at a time from the float32 state the code under test produced (as test_keyframe_parallel.py does):
a free-running reference turns one sign flip of a rounding-noise gradient into a whole learning-rate step.

The bounds.  adam_one computes, in float32 (u = 2^-24, the relative error of one rounding to nearest):

    m  = m + (g - m) * w1                       w1 = float(1 - b1), where w1 < 0.5
    m  = g + (g - m) * w1                       w1 = -float(b1), from float(1 - b1) = 0.5 on (torch's two-sided lerp)
    v  = v * b2 + (w2 * g) * g                  b2 = float(b2), w2 = float(1 - b2)
    d  = sqrt(v) * rcp(float(sqrt(1 - b2^t))) + eps
    p  = p - (lr * rcp(float(1 - b1^t))) * (m * rcp(d))

First moment, |m - m'| <= 2^-23 (|m_prev| + |g|) = 2 u S.  Three roundings (the difference, the product, the sum) and the
rounding of the factor w: |error| <= u (3 |w| |g - m| + |m'|) to first order, with |g - m| <= S and |m'| <= S.  For the
settings used here: w = 0.1 gives 1.3 u S; w = -0.5 (b1 = 0.5: factor and product exact) 1.5 u S; w = -0 (b1 = 0) gives g
itself, as float64 does.  (The first form alone would not: g - m rounds in the binade above g's and the sum lands one ulp
beside g, the whole bound when m is small; adam_one was that form until these tests showed it.)  The bound is relative to
the OPERANDS: 0.9 m + 0.1 g can cancel, and a bound relative to m' would then ask for more than float32 has.

Second moment, |v - v'| <= 2^-21 v' + 2^-125.  Every term is positive, so the bound is relative to the result: v b2 carries
the roundings of b2 and of the product (2 u), (w2 g) g those of w2 and of two products (3 u), the sum one more: <= 4 u v'
= 2^-22 v' to first order; 2^-21 leaves room for the second-order terms.  The floor covers a g^2 flushed to zero (2^-126 is
the smallest normal float32).

Parameter, |p - p'| <= 2 ulp32(p') + 1e-5 |p' - p_prev| + lr / (1 - b1^t) * 2^-23 (|m_prev| + |g|) / (sqrt(v') / sqrt(1 - b2^t) + eps).
The first two terms are the project's own bound (test_keyframe_parallel.py): the final subtraction rounds p' (half an ulp; two
leave room for a step that crosses a binade), and the step itself — two hardware reciprocals and a hardware square root of
1 ulp each, the roundings of sqrt(v), of the bias corrections and of four products, about 12 u = 7e-7 relative — stays far
inside 1e-5 of its own size.  The third term carries the first-moment bound through the division: where g ~ -9 m the new
moment all but cancels, its ABSOLUTE float32 error is many times 1e-5 of what is left, and a correct float32 implementation
fails the first two terms alone (a NumPy float32 restatement did, 28 times in 40 M elements, by up to 3.6 x; with the third
term its worst error / bound over 80 M elements was 0.25 for p, 0.49 for m, 0.45 for v — test_adam_ref.py repeats that
measurement at 2 M elements and every beta setting and asserts <= 0.5, which is the room left for the 1-ulp hardware sqrt
and rcp).

These bounds are conditions on the code, not descriptions of it: a result beyond one is a finding."""
import numpy as np

LRS = (5e-4, 5e-2, 5e-3, 1e-3)                          # the project's: xyz, opacity, scaling, rotation
STEPS = (1, 2, 3, 4, 1000)                              # step 1000 starts from the step-4 state
BETAS = ((0.9, 0.999), (0.5, 0.9), (0.0, 0.99))
EPSS = (1e-15, 1e-8)                                    # the reference's, and torch's default
WIDTHS = (3, 1, 2, 4)                                   # floats per surfel of the four model tensors
STARTS = (0, 3, 4, 6)                                   # ... and where their blocks start in the flat buckets, in units of N


def make_params(rng, n):
    """randn * 10^U(-3, 2): a small parameter next to a large one."""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 2.0, n)).astype(np.float32)


def make_grads(rng, n):
    """randn * 10^U(-8, 3), 20 % exact zeros."""
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8.0, 3.0, n)).astype(np.float32)
    g[rng.random(n) < 0.2] = 0.0
    return g


def adam_step64(p, g, m, v, lr, beta1, beta2, eps, t):
    """One float64 Adam step of float32 (or float64) inputs; lr a scalar or one value per element.  Returns p', m', v'."""
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    lr = np.asarray(lr, np.float64)
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    p1 = p - lr / (1.0 - beta1 ** t) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - beta2 ** t) + eps)
    return p1, m1, v1


def adam_tolerances(p_prev, g, m_prev, p_ref, v_ref, lr, beta1, beta2, eps, t):
    """The three bounds of the module docstring, per element, for one step whose float64 result is p_ref, (m_ref,) v_ref."""
    p_prev, g, m_prev = (np.asarray(x).astype(np.float64) for x in (p_prev, g, m_prev))
    lr = np.asarray(lr, np.float64)
    tol_m = 2.0 ** -23 * (np.abs(m_prev) + np.abs(g))
    tol_v = 2.0 ** -21 * v_ref + 2.0 ** -125
    ulp = np.spacing(np.abs(p_ref).astype(np.float32)).astype(np.float64)
    tol_p = (2.0 * ulp + 1e-5 * np.abs(p_ref - p_prev) +
             lr / (1.0 - beta1 ** t) * tol_m / (np.sqrt(v_ref) / np.sqrt(1.0 - beta2 ** t) + eps))
    return tol_p, tol_m, tol_v


def _worst(err, tol):
    err, tol = np.ravel(err), np.ravel(tol)
    if err.size == 0:
        return 0.0, -1
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err == 0.0, 0.0, np.inf))
    r = np.where(np.isfinite(err), r, np.inf)           # a NaN or an infinity is never inside a bound
    i = int(np.argmax(r))
    return float(r[i]), i


def adam_ratios(before, g, after, lr, beta1, beta2, eps, t):
    """before, after: (p, m, v) float32 arrays around ONE step with gradient g.  Returns {"p" | "m" | "v": (worst error /
    tolerance, its element)} against adam_step64 of `before` — 1.0 means exactly on the bound."""
    p0, m0, v0 = before
    p_ref, m_ref, v_ref = adam_step64(p0, g, m0, v0, lr, beta1, beta2, eps, t)
    tol_p, tol_m, tol_v = adam_tolerances(p0, g, m0, p_ref, v_ref, lr, beta1, beta2, eps, t)
    out = {}
    for key, got, ref, tol in (("p", after[0], p_ref, tol_p), ("m", after[1], m_ref, tol_m), ("v", after[2], v_ref, tol_v)):
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == ref.shape, (key, got.dtype, got.shape, ref.shape)
        out[key] = _worst(np.abs(got.astype(np.float64) - ref), tol)
    return out


class Worst:
    """Running worst ratios of one entry point, and the assertion that each stays inside its bound."""

    def __init__(self, name):
        self.name, self.r, self.n = name, {"p": 0.0, "m": 0.0, "v": 0.0}, 0

    def check(self, what, before, g, after, lr, beta1, beta2, eps, t, limit=1.0):
        ratios = adam_ratios(before, g, after, lr, beta1, beta2, eps, t)
        self.n += int(np.size(g))
        for key, (r, i) in ratios.items():
            self.r[key] = max(self.r[key], r)
            if not r <= limit:
                ref = adam_step64(before[0], g, before[1], before[2], lr, beta1, beta2, eps, t)["pmv".index(key)]
                raise AssertionError(
                    f"{self.name} {what}, betas ({beta1}, {beta2}) eps {eps} step {t}: {key}[{i}] = {np.ravel(after['pmv'.index(key)])[i]!r} "
                    f"vs float64 {np.ravel(ref)[i]!r}: {r:.3f} x its bound (from p {np.ravel(before[0])[i]!r} m {np.ravel(before[1])[i]!r} "
                    f"v {np.ravel(before[2])[i]!r}, gradient {np.ravel(g)[i]!r})")

    def __str__(self):
        return (f"[adam error / tolerance] {self.name}: p {self.r['p']:.3f}  m {self.r['m']:.3f}  v {self.r['v']:.3f}  "
                f"({self.n} element-steps)")


def adam_one32(p, g, m, v, lr, beta1, beta2, eps, t):
    """adam_one and make_adam_coef restated in NumPy float32: the same operations in the same order, each rounded to
    nearest once (no fused multiply-add), square root and 1 / x correctly rounded.  Returns p', m', v' (float32)."""
    f = np.float32
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    b2, w2, e = f(beta2), f(1.0 - beta2), f(eps)
    from_g = f(1.0 - beta1) >= f(0.5)
    w1 = -f(beta1) if from_g else f(1.0 - beta1)
    bc1, bc2_sqrt = f(1.0 - beta1 ** t), f(np.sqrt(1.0 - beta2 ** t))
    step_size = np.asarray(lr, f) * (f(1.0) / bc1)
    m1 = (g if from_g else m) + (g - m) * w1
    v1 = v * b2 + (w2 * g) * g
    denom = np.sqrt(v1) * (f(1.0) / bc2_sqrt) + e
    p1 = p - step_size * (m1 * (f(1.0) / denom))
    assert p1.dtype == m1.dtype == v1.dtype == f
    return p1, m1, v1


def flat_lr(N, lrs=LRS):
    """The learning rate of every element of a flat [xyz 3N | opacity N | scaling 2N | rotation 4N] bucket."""
    return np.concatenate([np.full(w * N, lr, np.float64) for w, lr in zip(WIDTHS, lrs)])


def surfel_rows(N, flat):
    """flat bucket (10 N) -> rows (N, 10): row i = [3i, 3i+1, 3i+2, 3N+i, 4N+2i, 4N+2i+1, 6N+4i .. 6N+4i+3]."""
    flat = np.asarray(flat)
    assert flat.shape == (10 * N,)
    return np.concatenate([flat[s * N:(s + w) * N].reshape(N, w) for s, w in zip(STARTS, WIDTHS)], axis=1)


def flat_from_rows(N, rows):
    """The inverse of surfel_rows."""
    rows = np.asarray(rows)
    assert rows.shape == (N, 10)
    return np.concatenate([rows[:, a:a + w].reshape(-1) for a, w in zip((0, 3, 4, 6), WIDTHS)])


def compact_rows(N, bits, grads_flat):
    """sls_grad_compact's rows: for every surfel i with bits[i], in surfel order, row rank(i) (the number of set bits
    below i) holds the surfel's ten values of the flat bucket.  Returns (K, 10) of grads_flat's dtype."""
    bits = np.asarray(bits, bool)
    grads_flat = np.asarray(grads_flat)
    assert bits.shape == (N,) and grads_flat.shape == (10 * N,)
    out = np.empty((int(bits.sum()), 10), grads_flat.dtype)
    rank = 0
    for i in range(N):
        if not bits[i]:
            continue
        out[rank] = [grads_flat[3 * i], grads_flat[3 * i + 1], grads_flat[3 * i + 2], grads_flat[3 * N + i],
                     grads_flat[4 * N + 2 * i], grads_flat[4 * N + 2 * i + 1]] + [grads_flat[6 * N + 4 * i + k] for k in range(4)]
        rank += 1
    return out


def pack_bitmap(N, bits, nwords):
    """bits (N bools) -> nwords uint64, little-endian bit order, the two verdict words (the last) zero."""
    full = np.zeros((nwords - 2) * 64, bool)
    full[:N] = np.asarray(bits, bool)
    out = np.zeros(nwords, np.uint64)
    out[:nwords - 2] = np.packbits(full, bitorder="little").view(np.uint64)
    return out
