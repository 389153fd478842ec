"""Reference side of the seeded densify draw ("The densify draw"; include/sls_draw_math.h) —
shared by tests/test_densify_draw_math.py (CPU) and tests/test_densify_draw.py (GPU).  Not a test module.

A NumPy restatement, operation for operation: Philox4x32-10 in uint64 arithmetic masked to 32 bits, the uniform and
-ln(u) in float32 array operations (each +, -, *, / of two float32 arrays rounds once, as the header's do under
-ffp-contract=off), the race keys, the k smallest of (key bits, pixel) and the no-draw rules.  The drawn set is a pure
function of (weights, seed, draw index), so a device result is compared to it without tolerance.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit words (scalars or arrays that broadcast with the
    counter) -> the four output words (uint32 arrays)."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in counter]
    k = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in key]
    *c, k0, k1 = np.broadcast_arrays(*c, *k)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        n0 = (p1 >> _S32) ^ c[1] ^ k0
        n2 = (p0 >> _S32) ^ c[3] ^ k1
        c = [n0, p1 & _MASK, n2, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def draw_words(n_pixels, seed, draw_index):
    """The random word of every pixel 0 .. n_pixels - 1: counter (pixel, 0, draw_index, 0), key (seed lo, seed hi)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    pix = np.arange(n_pixels, dtype=np.uint64)
    zero = np.zeros_like(pix)
    return philox4x32_10((pix, zero, zero + np.uint64(int(draw_index) & 0xFFFFFFFF), zero),
                         (seed & 0xFFFFFFFF, seed >> 32))[0]


def uniform(r):
    """(2 (r >> 9) + 1) 2^-24 as float32 (exact)."""
    r = np.asarray(r, dtype=np.uint32)
    return (np.uint32(2) * (r >> np.uint32(9)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def neg_log(u):
    """sls_draw_neg_log in float32 array operations, in the header's order."""
    f = np.float32
    u = np.ascontiguousarray(u, dtype=np.float32)
    bits = u.view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - np.int32(127)
    frac = bits & np.uint32(0x007FFFFF)
    fold = frac > np.uint32(0x003504F3)
    mbits = np.where(fold, frac | np.uint32(0x3F000000), frac | np.uint32(0x3F800000)).astype(np.uint32)
    e = e + fold.astype(np.int32)
    m = mbits.view(np.float32)
    t = (m - f(1.0)) / (m + f(1.0))
    s = t * t
    p = s * f(0.111111111)
    p = (p + f(0.142857143)) * s
    p = (p + f(0.2)) * s
    p = (p + f(0.333333333)) * s
    p = p + f(1.0)
    lnm = (t + t) * p
    ne = (-e).astype(np.float32)
    return (ne * f(0.693145751953125) - lnm) + ne * f(1.42860682030941723e-06)


def keys(weights, seed, draw_index):
    """The race keys (float32) of a flat weight array: E / w at w > 0, +inf elsewhere."""
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    E = neg_log(uniform(draw_words(w.size, seed, draw_index)))
    out = np.full(w.shape, np.inf, dtype=np.float32)
    pos = w > 0
    out[pos] = E[pos] / w[pos]
    return out


def select(key_array, k):
    """Ascending pixel indices (int64) of the k smallest (key bits, pixel)."""
    bits = np.ascontiguousarray(key_array, dtype=np.float32).view(np.uint32).astype(np.uint64)
    composite = (bits << _S32) | np.arange(bits.size, dtype=np.uint64)
    chosen = np.partition(composite, k - 1)[:k] if k < bits.size else composite
    return np.sort((chosen & _MASK).astype(np.int64))


def draw(weights, percentage, seed, draw_index, n_cand=None, gmax=None, total=None):
    """The drawn pixels (ascending int64) or None where nothing is drawn.  n_cand / gmax / total: the three statistics
    the weights kernel reports (default: the count of non-zero weights, the largest weight above the 1e-30 floor and
    the float64 sum of those) — the no-draw rules of slam_rules.densify_sample."""
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    real = np.where(w > np.float32(1.0e-30), w, np.float32(0.0))
    if n_cand is None:
        n_cand = int((w > 0).sum())
    if gmax is None:
        gmax = float(real.max()) if real.size else 0.0
    if total is None:
        total = float(real.astype(np.float64).sum())
    k = int(float(percentage) * int(n_cand))
    if k < 2 or not gmax > 0.0 or float(total) / float(gmax) <= 1e-5:
        return None
    return select(keys(w, seed, draw_index), k)
