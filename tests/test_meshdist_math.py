"""include/sls_meshdist_math.h as plain C99 (gcc -std=c99 -ffp-contract=off), against the float64 brute force and the
float32 twin of tests/meshdist_ref.py: the float bar on random triangles and slivers, exactness on the lattice, zero-area
faces, the error colours.  No device."""
import numpy as np
import pytest

import meshdist_ref as R

f32 = np.float32


def test_header_against_float64_on_random_triangles_and_slivers():
    """400 000 seeded cases: coordinates up to 64 m, sizes 1 cm to 10 m, a quarter of them slivers of height 1e-4, the query
    from ON the triangle (a tenth of them exactly, where a sliver's plane is at its worst) to 10 sizes away.
    |d - d64| <= 1e-5 * scale, scale = the largest distance from the query to the three vertices; nothing non-finite."""
    q, a, b, c = R.random_cases(400000, seed=1)
    d2, closest = R.host().triangles(q, a, b, c)
    d64, closest64 = R.triangle64(q, a, b, c)
    scale = R.scale_of(q, a, b, c)
    assert np.isfinite(d2).all() and np.isfinite(closest).all() and (d2 >= 0).all()
    err = (np.sqrt(d2.astype(np.float64)) - np.sqrt(d64)) / scale
    print(f"header vs float64: max |d - d64| / scale = {np.abs(err).max():.3e}, lowest {err.min():.3e} (below the truth)")
    assert np.abs(err).max() <= R.BAR
    # the closest point lies ON the triangle and at the distance returned: both within the bar, plus the one rounding of
    # `query frame + q`, half an ulp of the map's coordinates (up to 64 m)
    slack = R.BAR * scale + np.abs(q).max(1) * 2.0 ** -23
    on = np.sqrt(R.triangle64(closest.astype(np.float64), a, b, c)[0])
    away = np.abs(np.linalg.norm(closest.astype(np.float64) - q, axis=1) - np.sqrt(d64))
    print(f"closest point: off the triangle by {(on / slack).max():.3f} of its slack, off the distance by {(away / slack).max():.3f}")
    assert (on <= slack).all() and (away <= slack).all()
    # the twin restates the header: within the bar on its own, and the same bits up to its emulated fma (see meshdist_ref)
    t2, tclosest = R.triangle32(q, a, b, c)
    same = (t2.view(np.uint32) == d2.view(np.uint32)).mean()
    print(f"twin: the header's bits in {same:.6f} of the cases")
    assert np.abs(np.sqrt(t2.astype(np.float64)) - np.sqrt(d64)).max() <= R.BAR * scale.max()
    assert (np.abs(np.sqrt(t2.astype(np.float64)) - np.sqrt(d64)) <= R.BAR * scale).all() and same >= 0.999


def _regions(q):
    """The region of the triangle (0,0,0), (4,0,0), (0,4,0) a query's projection falls into: 0 inside, 1-3 a vertex, 4-6 an edge"""
    x, y = q[:, 0].astype(np.float64), q[:, 1].astype(np.float64)
    r = np.full(len(q), -1)
    r[(x > 0) & (y > 0) & (x + y < 4)] = 0
    r[(x <= 0) & (y <= 0)] = 1
    r[(x >= 4) & (y - x <= -4)] = 2
    r[(y >= 4) & (y - x >= 4)] = 3
    r[(y <= 0) & (x > 0) & (x < 4)] = 4
    r[(x <= 0) & (y > 0) & (y < 4)] = 5
    r[(x + y >= 4) & (np.abs(y - x) < 4)] = 6
    return r


def test_exact_on_the_lattice():
    """Triangle (0,0,0), (4,0,0), (0,4,0), queries on the 1/16 lattice above, in and below the plane: the three e . e are 16,
    16 and 32 and s = |n|^2 = 256, so every division is by a power of two, every intermediate a short dyadic number, and
    d2 and the closest point EQUAL the float64 values."""
    g = np.arange(-32, 97) / 16.0
    x, y, z = np.meshgrid(g, g, np.array([-1.5, -1 / 16, 0.0, 1 / 16, 1.0]), indexing="ij")
    q = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
    a, b, c = (np.broadcast_to(np.array(v, f32), q.shape) for v in ((0, 0, 0), (4, 0, 0), (0, 4, 0)))
    region = _regions(q)
    assert set(np.unique(region)) == set(range(7)) and min(np.bincount(region)) >= 100      # all seven regions
    d2, closest = R.host().triangles(q, a, b, c)
    d64, closest64 = R.triangle64(q, a, b, c)
    assert np.array_equal(d2.astype(np.float64), d64)
    assert np.array_equal(closest.astype(np.float64), closest64)
    t2, tclosest = R.triangle32(q, a, b, c)
    assert np.array_equal(t2, d2) and np.array_equal(tclosest, closest)
    # by hand: beyond the hypotenuse, above a vertex, inside below the plane, on the triangle
    hand = np.array([[4, 4, 0], [-3, -4, 0], [1, 1, -2], [1, 2, 0], [5, -1, 0.5]], f32)
    d2, closest = R.host().triangles(hand, a[:5], b[:5], c[:5])
    assert d2.tolist() == [8.0, 25.0, 4.0, 0.0, 2.25]
    assert closest.tolist() == [[2, 2, 0], [0, 0, 0], [1, 1, 0], [1, 2, 0], [4, 0, 0]]
    # the same triangle with its vertices rotated and its orientation flipped: the same distances
    for order in ((1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0)):
        tri = [a, b, c]
        d2o, _ = R.host().triangles(q, *(tri[k] for k in order))
        assert np.array_equal(d2o.astype(np.float64), d64), order


def test_zero_area_faces():
    """Collinear vertices give the distance to the segment they span, three coincident ones the distance to the point —
    by themselves: no branch asks for the area, and nothing divides by zero."""
    rng = np.random.default_rng(6)
    n = 20000
    base, step = rng.integers(-200, 201, (n, 3)) / 8.0, rng.integers(-8, 9, (n, 3)) / 8.0
    step[(step == 0).all(1)] = 1.0
    q = (base + rng.normal(0, 3, (n, 3))).astype(f32)
    k1, k2 = rng.integers(0, 6, (n, 1)), rng.integers(0, 6, (n, 1))            # (equal: two coincident vertices too)
    a, b, c = base.astype(f32), (base + k1 * step).astype(f32), (base + k2 * step).astype(f32)       # exactly collinear
    far = np.where(k1 >= k2, b, c)                                              # the segment they span: a .. the farther one
    for tri in ((a, b, c), (b, c, a), (c, a, b), (b, a, c)):
        d2, closest = R.host().triangles(q, *tri)
        assert np.isfinite(d2).all() and np.isfinite(closest).all()
        want, _ = R._segment64(a.astype(np.float64) - q, far.astype(np.float64) - a)
        scale = R.scale_of(q, a, b, c)
        assert (np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(want)) <= R.BAR * scale).all()
    d2, closest = R.host().triangles(q, a, a, a)
    want = ((a.astype(np.float64) - q) ** 2).sum(1)
    assert (np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(want)) <= R.BAR * np.sqrt(want)).all()
    assert np.array_equal(closest, (a - q) + q)                                 # the point itself, through the query frame
    d2, closest = R.host().triangles(a, a, a, a)                                # ... and a query on it
    assert not d2.any() and np.array_equal(closest, a)


def test_error_colours():
    h = R.host()
    T = f32(0.5)
    d = lambda k: f32((k / 256.0 * 0.5) ** 2)                                   # L = k exactly: the root and the quotient are exact
    hand = {0.0: (0, 255, 0), d(1): (2, 255, 0), d(127): (254, 255, 0), d(128): (255, 254, 0), d(255): (255, 0, 0),
            d(256): (255, 0, 0), f32(0.0625): (255, 254, 0), f32(1.0): (255, 0, 0), f32(np.inf): (255, 0, 0),
            f32(np.nan): (0, 0, 255), f32(-1.0): (0, 0, 255)}
    # green at 0, yellow at half the truncation (0.0625 = 0.25^2), red at and beyond it, blue for a NaN
    keys = np.array(list(hand), f32)
    assert h.colors(keys, T).tolist() == [list(v) for v in hand.values()]
    assert R.error_colors(keys, T).tolist() == [list(v) for v in hand.values()]
    rng = np.random.default_rng(2)
    for trunc in (0.5, 0.40625, 1.0, 3.3, 1e-3):
        d2 = np.concatenate([rng.uniform(0, 1.5 * trunc, 50000) ** 2, [0, np.nan, np.inf, -0.0, -2.0, 1e-45, 3e38],
                             (np.arange(0, 300) / 256.0 * trunc) ** 2]).astype(f32)
        got = h.colors(d2, trunc)
        assert np.array_equal(got, R.error_colors(d2, trunc))                   # the header against the restatement, bit for bit
        assert len(np.unique(got, axis=0)) > 200
