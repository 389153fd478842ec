"""include/sls_signdist_math.h as plain C99 (gcc -std=c99 -ffp-contract=off; tests/signdist_ref.py): the feature
classification against sls_meshdist_triangle and the lattice's regions, the header's own arctangent and corner angle
against libm, the sign on the blade against the analytic inside test, the status words of a mesh with one of each defect.
No device."""
import numpy as np

import meshdist_ref
import signdist_ref as R
from test_meshdist_math import _regions

f32 = np.float32


def test_triangle_gives_the_bits_of_the_unsigned_header():
    q, a, b, c = meshdist_ref.random_cases(400000, seed=1)
    d2, closest = meshdist_ref.host().triangles(q, a, b, c)
    s2, rel, feature = R.host().triangles(q, a, b, c)
    assert np.array_equal(s2.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal((rel + q).view(np.uint32), closest.view(np.uint32))
    assert set(np.unique(feature)) == set(range(7))


def test_all_seven_features_on_the_lattice():
    """Triangle (0,0,0), (4,0,0), (0,4,0) and the 1/16 lattice of test_meshdist_math: every decision is exact there, so the
    feature IS the region the query's projection falls into (regions: 1-3 the vertices, 4 edge AB, 5 edge CA, 6 edge BC)."""
    g = np.arange(-32, 97) / 16.0
    x, y, z = np.meshgrid(g, g, np.array([-1.5, -1 / 16, 0.0, 1 / 16, 1.0]), indexing="ij")
    q = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
    a, b, c = (np.broadcast_to(np.array(v, f32), q.shape) for v in ((0, 0, 0), (4, 0, 0), (0, 4, 0)))
    region = _regions(q)
    _, _, feature = R.host().triangles(q, a, b, c)
    want = np.array([0, 4, 5, 6, 1, 3, 2])[region]
    assert set(np.unique(feature)) == set(range(7))
    assert np.array_equal(feature, want)
    # a zero-length edge is its start vertex: the triangle (a, a, c) from beyond a
    _, _, ft = R.host().triangles(np.array([[-1, -1, 0]], f32), a[:1], a[:1], c[:1])
    assert ft.tolist() == [4]


def test_atan_against_libm():
    rng = np.random.default_rng(11)
    x = np.concatenate([[0.0, 1.0, np.tan(np.pi / 16), 1e300, np.inf], 10.0 ** rng.uniform(-300, 300, 500000), rng.uniform(0, 4, 500000)])
    got = R.host().atan(x)
    err = np.abs(got - np.arctan(x))
    print(f"atan: max |header - libm| = {err.max():.3e} rad")
    assert err.max() <= 1e-13
    assert got[0] == 0.0 and np.isnan(R.host().atan(np.array([np.nan]))[0])


def test_corner_angle_against_atan2():
    rng = np.random.default_rng(12)
    u = rng.normal(0, 1, (1000000, 3)) * 10.0 ** rng.uniform(-3, 3, (1000000, 1))
    w = rng.normal(0, 1, (1000000, 3)) * 10.0 ** rng.uniform(-3, 3, (1000000, 1))
    # 2 000 corners within 1e-9 rad of parallel and of opposite: w = +-(u turned by a tiny angle about a random axis)
    base = rng.normal(0, 1, (2000, 3))
    side = np.cross(base, rng.normal(0, 1, (2000, 3)))
    side *= (np.linalg.norm(base, axis=1) / np.linalg.norm(side, axis=1))[:, None]
    eps = rng.uniform(0, 1e-9, (2000, 1))
    near = (base + eps * side) * np.where(np.arange(2000) % 2 == 0, 1.0, -1.0)[:, None]
    u, w = np.concatenate([u, base]), np.concatenate([w, near])
    want = np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(1))
    # near parallel and opposite atan2 of the cancelling cross product is itself only good to eps64 * |u||w| / |u x w|; the
    # truth there is eps (or pi - eps) to first order, which the construction knows
    want[-2000:] = np.where(np.arange(2000) % 2 == 0, np.arctan(eps[:, 0]), np.pi - np.arctan(eps[:, 0]))
    got = R.host().angles(u, w)
    err = np.abs(got - want)
    print(f"corner angle: max |header - atan2| = {err[:-2000].max():.3e} rad; near 0 and pi {err[-2000:].max():.3e}")
    assert err.max() <= 1e-13
    assert R.host().angles([[1.0, 0, 0]], [[-1.0, 0, 0]])[0] == np.pi and R.host().angles([[0.0, 0, 0]], [[1.0, 0, 0]])[0] == 0.0


def test_the_blade():
    """200 000 uniform queries around the thin tetrahedron: the header's sign equals the analytic inside test for every query
    at least 1e-3 m from the surface; at most 0.5 % are nearer; and the face normal alone is wrong for more than 5 %."""
    v, f = R.blade()
    q = R.blade_queries(200000, seed=3)
    tables = R.host().tables(v, f)
    assert tables[3].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]               # closed, manifold, consistently oriented
    sd, face, closest, feature = R.host().query(v, f, tables, q)
    inside = R.inside_convex(q, v, f)
    d64 = np.sqrt(meshdist_ref.mesh64(q, v, f)[0])
    far = d64 >= 1e-3
    wrong = ((sd < 0) != inside) & far
    # the face-normal sign, float64, for the same (query, face)
    fn = tables[0].astype(np.float64)[face]
    naive_wrong = ((((q.astype(np.float64) - closest) * fn).sum(1) < 0) != inside) & far
    print(f"blade: {int((~far).sum())} of {len(q)} excluded, pseudo-normal sign wrong for {int(wrong.sum())}, "
          f"face-normal sign wrong for {int(naive_wrong.sum())} ({naive_wrong.mean():.3%}); features {np.bincount(feature, minlength=7).tolist()}")
    assert (~far).mean() <= 0.005
    assert not wrong.any()
    assert naive_wrong.mean() > 0.05
    # the float64 restatement agrees, sign and magnitude
    s64, _ = R.signed64(q[:20000], v, f)
    assert np.array_equal((s64 < 0)[far[:20000]], (sd[:20000] < 0)[far[:20000]])
    assert np.abs(np.abs(s64) - np.abs(sd[:20000])).max() <= 1e-5 * 8


def test_tables_against_the_float64_restatement():
    for v, f in (R.blade(), R.cube(), R.l_prism(), R.folded_sheet(), R.icosphere(2)):
        fn, en, vn, status = R.host().tables(v, f)
        fn64, en64, vn64 = R.tables64(v, f)
        assert np.abs(fn - fn64).max() <= 1e-6 and np.abs(en - en64).max() <= 1e-6 and np.abs(vn - vn64).max() <= 1e-6
        assert status[:4].tolist() == [0, 0, 0, 0] and status[7] == 1
    # a closed surface: the corner angles at a vertex of the cube sum to 3 pi / 2 whatever its triangulation, and the
    # pseudo-normal points along the diagonal
    v, f = R.cube()
    _, _, vn, _ = R.host().tables(v, f)
    corner = np.sign(v - v.mean(0))
    assert np.abs(vn - corner * (np.pi / 2)).max() <= 1e-6
    assert R.host().tables(*R.folded_sheet())[3].tolist() == [0, 0, 0, 0, 10, 0, 0, 1]     # an open sheet: 10 boundary edges


def test_status_words_of_the_defect_mesh():
    v, f = R.defects()
    fn, en, vn, status = R.host().tables(v, f)
    print("defect mesh status:", status.tolist())
    # one index-degenerate face (inside the range), one zero-area face whose three edges are boundary edges; the fin's two
    # new edges are boundary edges too and its third has three owners, as have the three edges of the repeated triangle;
    # the flipped triangle runs the same way as its neighbour across each of its edges that has exactly two owners
    assert status[0] == 1 and status[1] == 0 and status[2] == 0 and status[3] == 1 and status[7] == 1
    assert status[4] == 3 + 2 and status[5] >= 3 and status[6] >= 1
    assert not fn[-1].any() and not fn[-2].any() and not en[-1].any() and not vn[9:].any()
    # restated: group sizes by undirected edge over the faces that are not index-degenerate
    live = f[:-1].astype(np.int64)
    lo, hi = np.minimum(live, np.roll(live, -1, 1)).reshape(-1), np.maximum(live, np.roll(live, -1, 1)).reshape(-1)
    key, inverse, counts = np.unique(lo * 100 + hi, return_inverse=True, return_counts=True)
    start = live.reshape(-1)
    same = sum(1 for g in np.flatnonzero(counts == 2) if len(set(start[inverse == g])) == 1)
    assert status[4:7].tolist() == [int((counts == 1).sum()), int((counts >= 3).sum()), same]
    # an out-of-range index and a non-finite vertex are counted, not dereferenced
    f2 = np.concatenate([f, [[0, 1, 99], [-1, 2, 3]]]).astype(np.int32)
    v2 = np.array(v)
    v2[8, 0] = np.inf
    s2 = R.host().tables(v2, f2)[3]
    assert s2[0] == 3 and s2[1] == 2 and s2[2] == 1


def test_signed_colours():
    h = R.host()
    T = 0.5
    sd = np.array([0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 3.0, -3.0, np.inf, -np.inf, np.nan, 0.5 / 256, -0.5 / 256], f32)
    assert h.colors(sd, T).tolist() == [[255, 255, 255], [255, 255, 255], [255, 127, 127], [127, 127, 255], [255, 0, 0], [0, 0, 255],
                                        [255, 0, 0], [0, 0, 255], [255, 0, 0], [0, 0, 255], [0, 0, 0], [255, 254, 254], [254, 254, 255]]
