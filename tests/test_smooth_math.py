"""include/sls_smooth_math.h compiled for the host against the NumPy restatement of tests/smooth_ref.py (no device needed):
offsets, neighbours, boundary flags, status words and positions equal bit for bit on every case and setting (NumPy float32
and float64 round every operation once, as the header does); and the properties of the rule, on the restatement."""
import numpy as np
import pytest

import smooth_ref as ref
from mesh_ref import bits

CASES = ref.cases()
SETTINGS = ref.settings()


@pytest.fixture(scope="module")
def host():
    return ref.host()


def test_the_settings_hold_both_parities():
    steps = {len(ref.factors(m, n)) % 2 for m, _, _, n in SETTINGS if n}
    assert steps == {0, 1} and len(SETTINGS) == 35
    assert {m for m, _, _, _ in SETTINGS} == {0, 1, 2} and {n for m, _, _, n in SETTINGS if m == ref.TAUBIN} == {0, 1, 2}


@pytest.mark.parametrize("case", sorted(CASES))
def test_adjacency_header_equals_restatement(host, case):
    v, f = CASES[case]
    offsets, nbr, boundary, stats = ref.adjacency(f, len(v))
    got_o, got_n, got_b, status = host.adjacency(f, len(v))
    assert status == ref.status_words(stats), case
    assert np.array_equal(got_o, offsets) and np.array_equal(got_n, nbr) and np.array_equal(got_b, boundary)
    # the properties of every adjacency: rows ascending and distinct, symmetric, no loops, 2 E entries
    assert offsets[0] == 0 and offsets[-1] == len(nbr) == 2 * stats["edges"] and (np.diff(offsets) >= 0).all()
    rows = np.repeat(np.arange(len(v)), np.diff(offsets))
    pairs = set(zip(rows.tolist(), nbr.tolist()))
    assert len(pairs) == len(nbr) and all((b, a) in pairs and a != b for a, b in pairs)
    for i in range(len(v)):
        assert (np.diff(nbr[offsets[i]:offsets[i + 1]]) > 0).all()


def test_hand_case_counts():
    """what every hand case is there for, from the restatement"""
    want = {"tetrahedron": dict(live=4, edges=6, boundary=0, max_row=3), "triangle": dict(live=3, edges=3, boundary=3, max_row=2),
            "sheet": dict(live=25, edges=56, boundary=16, max_row=6), "fan_64": dict(live=65, edges=128, boundary=64, max_row=64),
            "fan_65": dict(max_row=65), "fan_100": dict(max_row=100, boundary=100),
            "three_on_edge": dict(live=5, edges=7, boundary=5, max_row=4),          # the shared edge has three owners: not a boundary edge
            "repeated": dict(live=4, edges=5, boundary=3, degenerate=0),            # (0,2), (1,2) have three owners, (0,1) four; (0,3), (1,3) one
            "bad_indices": dict(live=4, edges=5, degenerate=6, out_of_range=4),
            "unreferenced": dict(live=5, edges=7, degenerate=1, nonfinite=0), "coincident": dict(live=5, edges=8),
            "nan_live": dict(live=4, nonfinite=1), "no_vertices": dict(live=0, edges=0, max_row=0), "no_faces": dict(live=0, edges=0, boundary=0)}
    for case, words in want.items():
        v, f = CASES[case]
        stats = ref.smooth(v, f, 0)[1]
        assert {k: stats[k] for k in words} == words, (case, stats)
    assert ref.adjacency(CASES["repeated"][1], 5)[2].tolist() == [1, 1, 0, 1, 0]
    assert ref.adjacency(CASES["three_on_edge"][1], 5)[2].tolist() == [1, 1, 1, 1, 1]


@pytest.mark.parametrize("case", sorted(CASES))
def test_header_equals_restatement(host, case):
    v, f = CASES[case]
    for method, weights, fix, n in SETTINGS:
        want, stats = ref.smooth(v, f, n, method, weights, fix_boundary=fix)
        got, status = host.smooth(v, f, n, method, weights, fix_boundary=fix)
        assert status == ref.status_words(stats), (case, method, weights, fix, n)
        if case not in ref.UNSPECIFIED:
            assert np.array_equal(bits(got), bits(want)), (case, method, weights, fix, n)
        if n == 0:
            assert np.array_equal(bits(got), bits(v))
    offsets = ref.adjacency(f, len(v))[0]                           # a vertex that is not live is copied bit for bit, always
    dead = np.diff(offsets) == 0
    got = host.smooth(v, f, 5, ref.LAPLACIAN)[0]
    assert np.array_equal(bits(got[dead]), bits(v[dead]))
    if case == "unreferenced":
        assert dead[3] and bits(got[3]).tolist() == [0x80000000] * 3


def test_long_rows_follow_the_butterfly():
    """the hub of fan_65: 64 lanes and the butterfly, not one sum after the other (the two orders differ in the last bits
    here, so a host or a device that took the short path would be caught)"""
    v, f = CASES["fan_65"]
    offsets, nbr, _, _ = ref.adjacency(f, len(v))
    items = ref._items(v, np.zeros((65,), np.int64), nbr[:65], ref.INVERSE_DISTANCE)
    serial = np.zeros((4,))
    for row in items:
        serial = serial + row
    assert not np.array_equal(serial, ref.segment_sum(items))


def test_planar_sheet_stays_in_its_plane():
    """the float64 sums carry a relative error of at most N 2^-53, far below a float32 ulp (3e-8 at z = 0.3): the rounding
    returns the plane's z or, at worst, its neighbour"""
    v, f = CASES["sheet"]
    border = ref.sheet_border()
    inner = np.setdiff1d(np.arange(len(v)), border)
    for method, weights, fix, n in SETTINGS:
        out = ref.smooth(v, f, n, method, weights, fix_boundary=fix)[0]
        assert np.abs(out[:, 2].astype(np.float64) - np.float32(ref.SHEET_Z)).max() <= 6e-8
        if fix:
            assert np.array_equal(bits(out[border]), bits(v[border]))
            if n:
                assert (bits(out[inner]) != bits(v[inner])).any()
    assert ref.adjacency(f, len(v))[2].nonzero()[0].tolist() == border.tolist()


def test_factor_zero_is_the_identity():
    for case in ("sheet_noisy", "fan_100", "sphere_noisy", "coincident"):
        v, f = CASES[case]
        out = ref.smooth(v, f, 3, ref.LAPLACIAN, ref.UNIFORM, lam=0.0)[0]
        assert np.array_equal(bits(out), bits(v)), case


def test_lattice_translation_is_exact():
    """rows of 2 and 4 neighbours (a triangle, an octahedron), coordinates on the lattice of 1/16 and factors 0.5 / -0.5: every
    sum, mean and step is exact in float32, so a translation by a lattice vector goes through exactly"""
    octa_v = np.array([(1, 0, 0), (-1, 0.125, 0), (0, 1.25, 0.0625), (0.5, -1, 0), (0, 0.25, 1), (0.0625, 0, -1.5)], np.float32)
    octa_f = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int32)
    tri_v, tri_f = np.array([(0, 0, 0), (1, 0.25, 0), (0.25, 1, 0.5)], np.float32), np.array([(0, 1, 2)], np.int32)
    shift = np.array([3.0, -2.5, 7.0625], np.float32)
    for v, f in ((octa_v, octa_f), (tri_v, tri_f)):
        assert set(np.diff(ref.adjacency(f, len(v))[0]).tolist()) <= {2, 4}
        for method, n, mu in ((ref.LAPLACIAN, 2, 0.0), (ref.TAUBIN, 1, -0.5)):
            a = ref.smooth(v, f, n, method, ref.UNIFORM, lam=0.5, mu=mu)[0]
            b = ref.smooth(v + shift, f, n, method, ref.UNIFORM, lam=0.5, mu=mu)[0]
            assert np.array_equal(bits(a + shift), bits(b)) and not np.array_equal(bits(a), bits(v))


SPHERE_ITERATIONS = 5


def test_sphere_noise_falls_and_taubin_keeps_the_radius():
    """The welded unit sphere with uniform radial noise of 0.02 (seed 7), 5 iterations, inverse-distance weights, from the
    restatement alone.  rms deviation of the radius from its mean: input 1.1595e-2, Laplacian 4.2502e-3, Taubin 6.3370e-3 (both
    fall); mean radius: input 0.998942, Laplacian 0.994340 (it shrinks), Taubin 0.999083 (closer to the input's)."""
    v, f = ref.sphere(ref.SPHERE_NOISE)
    r0 = ref.radii(v)
    lap = ref.radii(ref.smooth(v, f, SPHERE_ITERATIONS, ref.LAPLACIAN)[0])
    tau = ref.radii(ref.smooth(v, f, SPHERE_ITERATIONS, ref.TAUBIN)[0])
    rms = lambda r: float(np.sqrt(((r - r.mean()) ** 2).mean()))     # noqa: E731
    print(f"rms: input {rms(r0):.4e}, laplacian {rms(lap):.4e}, taubin {rms(tau):.4e}; mean radius: input {r0.mean():.6f}, "
          f"laplacian {lap.mean():.6f}, taubin {tau.mean():.6f}")
    assert rms(lap) < rms(r0) and rms(tau) < rms(r0)
    assert abs(tau.mean() - r0.mean()) < abs(lap.mean() - r0.mean())
