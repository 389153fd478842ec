"""include/sls_raycast_math.h on the host (no device): the watertight ray / triangle test is exact on a lattice, lets no
ray through a closed lattice mesh, agrees with float64 wherever float64 is clear, and the box test never rejects the box
of a face the triangle test reports."""
import numpy as np
import pytest

from raycast_ref import BAR, cube, edges_of, host, moller_trumbore64, octahedron, random_cases, rays_at, scale_of, shape_of

TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
# directions whose largest |component| is 1 or 2: the shear's divisions are exact
DIRS = np.array([[0, 0, -1], [0, 0, 1], [1, 0, -1], [1, 1, 2], [-1, 0, 2], [0, 1, -2], [1, -1, -1], [2, 1, -1], [-2, 1, 1],
                 [1, 2, 1], [0.5, -2, 1], [0, -1, 0.5], [2, 2, -2]], np.float64)
TS = np.array([0.5, 1.0, 2.0, 3.0])


def _lattice(points, dirs=DIRS, ts=TS):
    """Rays that meet the plane z = 0 at `points` after t: every (point, direction, t)."""
    p, d, t = (x.reshape(-1, x.shape[-1]) for x in np.broadcast_arrays(np.asarray(points, np.float64)[:, None, None, :],
                                                                         dirs[None, :, None, :], ts[None, None, :, None]))
    return p - t[:, :1] * d, d, t[:, 0], p


@pytest.mark.parametrize("name,points", [
    ("interior", [[1, 1, 0], [0.5, 2, 0], [2.5, 1.25, 0]]),
    ("edges", [[2, 0, 0], [2, 2, 0], [0, 2, 0], [1, 3, 0], [0.5, 0, 0]]),
    ("vertices", [[0, 0, 0], [4, 0, 0], [0, 4, 0]]),
])
def test_lattice_hits_equal_float64(name, points):
    o, d, t, p = _lattice(points)
    hit, t32, u32, v32 = host().triangles(o, d, TRI[None, 0], TRI[None, 1], TRI[None, 2])
    hit64, t64, u64, v64, _ = moller_trumbore64(o, d, TRI[0], TRI[1], TRI[2])
    assert hit64.all() and hit.all(), (name, np.flatnonzero(~hit))
    assert np.array_equal(t32.astype(np.float64), t64) and np.array_equal(t64, t)
    assert np.array_equal(u32.astype(np.float64), u64) and np.array_equal(u64, p[:, 0] / 4)
    assert np.array_equal(v32.astype(np.float64), v64) and np.array_equal(v64, p[:, 1] / 4)


def test_lattice_misses():
    h = host()
    a, b, c = TRI[None, 0], TRI[None, 1], TRI[None, 2]
    # outside the triangle, in its plane's reach
    o, d, _, _ = _lattice([[3, 3, 0], [-1, 1, 0], [5, 0, 0], [1, -0.5, 0], [4.5, -0.5, 0]])
    assert not h.triangles(o, d, a, b, c)[0].any()
    # pointing away: the plane lies behind the origin
    o, d, _, _ = _lattice([[1, 1, 0], [2, 0, 0], [0, 0, 0]])
    hit = h.triangles(o, -d, a, b, c)[0]
    assert not hit.any()
    # parallel to the plane, above it; and IN the plane: through the interior, along an edge, through a vertex
    par_d = np.array([[1, 0, 0], [1, 1, 0], [-1, 2, 0], [0, -1, 0], [2, 1, 0]], np.float64)
    for origin in ([1, 1, 1], [-1, 1, 0.5], [-1, 1, 0], [-2, 0, 0], [-1, -1, 0], [5, -1, 0], [0, -3, 0], [1, 1, 0]):
        o = np.broadcast_to(np.array(origin, np.float64), par_d.shape)
        for sgn in (1.0, -1.0):
            assert not h.triangles(o, sgn * par_d, a, b, c)[0].any(), origin


def test_both_sides_hit_and_t_range():
    h = host()
    a, b, c = TRI[None, 0], TRI[None, 1], TRI[None, 2]
    o = np.array([[1, 1, 2], [1, 1, -2]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, 1]], np.float32)
    hit, t, u, v = h.triangles(o, d, a, b, c)
    assert hit.all() and t.tolist() == [2.0, 2.0] and u.tolist() == [0.25, 0.25] and v.tolist() == [0.25, 0.25]
    # the ends of [t_min, t_max] are inside, the next floats are not; a direction of length 4 quarters t
    assert h.triangles(o, d, a, b, c, t_min=2.0, t_max=2.0)[0].all()
    assert not h.triangles(o, d, a, b, c, t_min=np.nextafter(np.float32(2), np.float32(3)))[0].any()
    assert not h.triangles(o, d, a, b, c, t_max=np.nextafter(np.float32(2), np.float32(0)))[0].any()
    assert h.triangles(o, 4 * d, a, b, c)[1].tolist() == [0.5, 0.5]
    # -0 comes back as +0: a ray that starts on the face
    hit, t, _, _ = h.triangles(np.array([[1, 1, 0]], np.float32), np.array([[0, 0, -1]], np.float32), a, b, c)
    assert hit.all() and t.view(np.uint32).tolist() == [0]


def test_refused_rays():
    h = host()
    o = np.zeros((6, 3), np.float32)
    d = np.array([[0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-31, -1e-31, 0], [0, 0, 1], [0, -1e-30, 0]], np.float32)
    assert h.valid(o, d).tolist() == [False, False, False, False, True, True]
    o2 = o.copy()
    o2[4, 1] = np.inf
    assert not h.valid(o2, d)[4]


# ---- watertightness --------------------------------------------------------------------------------------------------------
MESHES = {"octahedron": (octahedron, [[0, 0, 0], [1, 1, -1], [0.5, -1.5, 1.25], [-1, 2, 0.5]]),
          "cube12": (lambda: cube(1), [[0, 0, 0], [1, 2, -1], [0.5, -1.5, 2.25], [-3, 3, 3]]),
          "cube8x8": (lambda: cube(8, seed=3), [[0, 0, 0], [1, 2, -1], [0.5, -1.5, 2.25], [-3, 3, 3]])}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_no_ray_passes_between_faces(name):
    make, origins = MESHES[name]
    v, f = make()
    edges = edges_of(f)
    targets = np.concatenate([v.astype(np.float64), 0.5 * (v[edges[:, 0]].astype(np.float64) + v[edges[:, 1]])])
    # the faces that share each target: a vertex's faces, an edge's two faces
    share = [set(np.flatnonzero((f == i).any(1))) for i in range(len(v))]
    share += [share[a] & share[b] for a, b in edges]
    assert all(len(s) >= 2 for s in share)
    n_exact = 0
    for origin in origins:
        o, d = rays_at(targets, origin)
        assert np.array_equal(o.astype(np.float64) + d.astype(np.float64), targets), "the targets must be representable"
        t, face, _ = host().cast(v, f, o, d)
        assert (face >= 0).all(), f"{name} from {origin}: {int((face < 0).sum())} rays passed through"     # the condition
        assert all(int(face[i]) in share[i] for i in range(len(targets)))
        assert np.all(np.abs(t - 1.0) <= BAR)
        # where the shear is exact (the largest |component| of d is a power of two) the ray meets the vertex or the edge
        # EXACTLY: every face that shares it is hit at t = 1 and the lowest index wins
        m = np.abs(d).max(1)
        exact = np.frexp(m)[0] == 0.5
        n_exact += int(exact.sum())
        lowest = np.array([min(s) for s in share])
        assert np.array_equal(face[exact], lowest[exact]) and np.all(t[exact] == 1.0)
    assert n_exact >= len(targets)          # from the centre every ray is exact


# ---- against float64 -----------------------------------------------------------------------------------------------------
# A case is CLEAR when each part of its float64 margin (raycast_ref.moller_trumbore64) reaches its threshold:
#   * |cos| between ray and normal >= 0.05 (3 degrees off the plane);
#   * t at least 1e-3 |t| away from both ends of [t_min, t_max];
#   * the smallest |barycentric weight| >= 1e-3 + 16 ulps of the scale expressed as a weight: the sheared vertices are
#     differences of coordinates as large as the scale, so the ray's position against an edge is known to a few 2^-24 scale
#     and no better; as a weight that is 2^-24 scale / (the face's height seen along the ray = height |cos|).
# None of it looks at what the header returns.
EPS32 = 2.0 ** -24


def _clear(o, d, a, b, c):
    hit64, t64, u64, v64, _ = moller_trumbore64(o, d, a, b, c)
    o64, d64, a64, b64, c64 = (np.asarray(x, np.float64) for x in (o, d, a, b, c))
    n = np.cross(b64 - a64, c64 - a64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = np.abs((n * d64).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d64, axis=1))
        wmin = np.abs(np.minimum(np.minimum(u64, v64), 1.0 - u64 - v64))
        tdist = np.abs(t64) / np.maximum(np.abs(t64), 1e-300)        # t_min = 0, t_max = inf: the distance from 0
        longest, height = shape_of(a, b, c)
        scale = scale_of(o, a, b, c)
        w_noise = 16 * EPS32 * np.maximum(scale, longest) / (height * cos)
        clear = (cos >= 0.05) & (tdist >= 1e-3) & (wmin >= 1e-3 + w_noise)
    return np.where(np.isfinite(w_noise), clear, False), hit64, t64


def test_random_cases_against_float64():
    n = 200_000
    o, d, a, b, c = random_cases(n, seed=11)
    longest, height = shape_of(a, b, c)
    assert 0.2 < (height < 1e-3 * longest).mean() < 0.3        # a quarter are slivers
    hit, t, u, v = host().triangles(o, d, a, b, c)
    clear, hit64, t64 = _clear(o, d, a, b, c)
    share = 1.0 - clear.mean()
    print(f"unclear cases: {share:.4%} of {n}; hits among the clear: {hit64[clear].mean():.3f}")
    assert share <= 0.05
    assert 0.2 < hit64[clear].mean() < 0.8                  # both decisions are exercised
    wrong = clear & (hit != hit64)
    print(f"wrong decisions among the clear: {int(wrong.sum())}")
    assert not wrong.any()
    both = clear & hit64
    # t is a ray parameter: |d| t is a length, compared with the scale
    err = np.abs(t[both].astype(np.float64) - t64[both]) * np.linalg.norm(d[both].astype(np.float64), axis=1)
    scale = scale_of(o[both], a[both], b[both], c[both])
    sl = (height < 1e-3 * longest)[both]
    print(f"max |t - t64| |d| / scale = {np.max(err / scale):.3e} (slivers {np.max((err / scale)[sl]):.3e}, others "
          f"{np.max((err / scale)[~sl]):.3e})")
    assert np.all(err <= BAR * scale)


def test_slivers_in_general_orientation():
    """Slivers as meshdist_ref makes them, any orientation: the decisions still agree wherever they are clear, and t is
    off by no more than the weight noise times the face's length.  Each edge function is wrong by at most 3 roundings of
    products up to (2 L)^2 and by the sheared vertices' own error, 3 2^-24 scale each, times 2 L; det is at least
    L height cos; the three weights' errors each move t by at most the spread sqrt(3) L of the vertices along the
    dominant axis: 64 2^-24 (L + scale) L / (height cos) covers it.  Measured: the printed figure."""
    n = 100_000
    o, d, a, b, c = random_cases(n, seed=12, sliver_share=1.0, aligned_slivers=False)
    hit, t, _, _ = host().triangles(o, d, a, b, c)
    clear, hit64, t64 = _clear(o, d, a, b, c)
    assert clear.mean() > 0.5 and not (clear & (hit != hit64)).any()
    both = clear & hit64
    d64 = d[both].astype(np.float64)
    n64 = np.cross(b[both].astype(np.float64) - a[both], c[both].astype(np.float64) - a[both])
    cos = np.abs((n64 * d64).sum(1)) / (np.linalg.norm(n64, axis=1) * np.linalg.norm(d64, axis=1))
    longest, height = (x[both] for x in shape_of(a, b, c))
    scale = scale_of(o[both], a[both], b[both], c[both])
    err = np.abs(t[both].astype(np.float64) - t64[both]) * np.linalg.norm(d64, axis=1)
    print(f"slivers, any orientation: max |t - t64| |d| = {np.max(err / scale):.3e} of the scale, {np.max(err / longest):.3e} of "
          f"the face's length; {np.mean(err > BAR * scale):.2%} of the clear hits beyond 1e-5 of the scale")
    assert np.all(err <= BAR * scale + 64 * EPS32 * (longest + scale) * longest / (height * cos))


# ---- the box test -----------------------------------------------------------------------------------------------------------
def _box_cases(seed, n):
    """(o, d, a, b, c): random cases, a quarter each left alone, with the origin moved onto a face of the triangle's own
    box, with one direction component zeroed, and with both (the same axis)."""
    o, d, a, b, c = (x.copy() for x in random_cases(n, seed))
    rng = np.random.default_rng(seed + 1)
    mn, mx = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    rows, k, kind = np.arange(n), rng.integers(0, 3, n), rng.integers(0, 4, n)
    face = np.where(rng.random(n) < 0.5, mn[rows, k], mx[rows, k])
    on_face, zero = (kind == 1) | (kind == 3), kind >= 2
    o[rows[on_face], k[on_face]] = face[on_face]
    d[rows[zero], k[zero]] = 0.0
    return o, d, a, b, c


def test_box_never_rejects_a_reported_hit():
    h = host()
    want, got, seed = 100_000, [], 100
    total = 0
    while total < want:
        o, d, a, b, c = _box_cases(seed, 150_000)
        seed += 7
        ok = h.valid(o, d)
        hit, t, _, _ = h.triangles(o, d, a, b, c)
        keep = hit & ok
        mn, mx = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        passed = h.boxes(o[keep], d[keep], mn[keep], mx[keep], t[keep])
        got.append((passed, o[keep], d[keep]))
        total += int(keep.sum())
    passed = np.concatenate([g[0] for g in got])
    o, d = np.concatenate([g[1] for g in got]), np.concatenate([g[2] for g in got])
    print(f"{len(passed)} reported hits, {(d == 0).any(1).sum()} with a zero direction component")
    assert (d == 0).any(1).sum() > 1000
    assert passed.all(), f"{int((~passed).sum())} boxes of reported hits rejected"


def test_box_zero_components_and_origins_on_faces():
    h = host()
    mn, mx = np.array([[1, 1, 1]], np.float32), np.array([[2, 3, 4]], np.float32)
    cases = [  # origin, direction, passes
        ([1, 0, 2], [0, 1, 0], True),          # slides along the face x = 1
        ([2, 0, 4], [0, 1, 0], True),          # along the edge x = 2, z = 4
        ([1, 1, 0], [0, 0, 1], True),          # along the edge x = 1, y = 1
        ([1, 1, 1], [0, 0, -1], True),         # starts on a corner, leaves
        ([1, 2, 2], [1, 0, 0], True),          # starts on a face, goes in
        ([0.5, 0, 2], [0, 1, 0], False),       # parallel, outside the slab
        ([2.5, 2, 5], [0, 0, -1], False),
        ([0, 2, 2], [-1, 0, 0], False),        # points away
        ([1.5, 2, 2], [0, 0, 1], True),        # from inside
        ([1.5, 2, 2], [-0.0, 0, 1], True),     # a negative zero
    ]
    o = np.array([x[0] for x in cases], np.float32)
    d = np.array([x[1] for x in cases], np.float32)
    assert h.boxes(o, d, mn, mx, np.inf).tolist() == [x[2] for x in cases]
    # the bound: the box is entered at t = 1 along +y from y = 0
    o1, d1 = np.array([[1.5, 0, 2]], np.float32), np.array([[0, 1, 0]], np.float32)
    assert h.boxes(o1, d1, mn, mx, 1.0).all() and not h.boxes(o1, d1, mn, mx, 0.99).any()
    assert not h.boxes(o1, d1, mn, mx, np.inf, t_lo=3.01).any() and h.boxes(o1, d1, mn, mx, np.inf, t_lo=3.0).all()
