"""include/sls_tsdf_math.h compiled as plain C (tsdf_ref.host()) against the NumPy restatements of tests/tsdf_ref.py, and
the geometry of the marching-tetrahedra rule: block keys and extraction bit for bit, integration within 1e-5 of trunc of
float64, the six tetrahedra and their 16 cases, a sphere that must come out closed, and missing data.  No device."""
import itertools

import numpy as np
import pytest

import tsdf_ref as ref
from tsdf_ref import CENTRE, ORIGIN, TRUNC, VS, bits as _bits


# ---- block keys ------------------------------------------------------------------------------------------------------
def test_block_keys_bit_for_bit():
    h = ref.host()
    pts = ref.key_points()
    for origin in ((0.0, 0.0, 0.0), ORIGIN):
        want, n_nf, n_rng = ref.blocks_of_points(pts, VS, TRUNC, origin)
        got, g_nf, g_rng = h.blocks_of_points(pts, VS, TRUNC, origin)
        print(f"origin {origin}: {len(want)} blocks, {n_nf} non-finite, {n_rng} out of range")
        assert (g_nf, g_rng) == (n_nf, n_rng) == (2, 3)
        assert np.array_equal(got, want)
        assert np.all(np.diff(ref.block_key(want)) > 0)
    # a point on a block face names two blocks per axis below the largest margin and three with it (the box ends on the
    # next face); one in the middle of a block names three per axis from 2 m > 8 voxels on — its own block among them,
    # which the corners of the box alone would miss
    keys, ok = h.point_keys(np.zeros((1, 3), np.float32), VS, 6 * VS)
    assert ok.all() and len(np.unique(keys)) == 8
    assert len(np.unique(h.point_keys(np.zeros((1, 3), np.float32), VS, 7 * VS)[0])) == 27
    mid = np.full((1, 3), 4 * VS, np.float32)
    keys, ok = h.point_keys(mid, VS, TRUNC)
    assert ok.all() and len(np.unique(keys)) == 27 and int(ref.block_key(np.array([0, 0, 0]))) in keys.tolist()[0]
    assert len(np.unique(h.point_keys(mid, VS, 2 * VS)[0])) == 1
    # {lo, mid, hi} is the whole range lo .. hi: an exhaustive walk over the boxes of a cloud finds the same blocks
    cloud = ref.key_points()[:300].astype(np.float64)
    walk = set()
    for p in cloud:
        lo, hi = np.floor((p - TRUNC - VS) / (8 * VS)).astype(int), np.floor((p + TRUNC + VS) / (8 * VS)).astype(int)
        walk.update(itertools.product(*(range(lo[a], hi[a] + 1) for a in range(3))))
    assert walk == set(map(tuple, ref.blocks_of_points(cloud, VS, TRUNC)[0].tolist()))
    wall = np.stack([np.full(50, 4 * VS), np.linspace(-3, 3, 50), np.linspace(-2, 2, 50)], 1).astype(np.float32)
    assert (ref.blocks_of_points(wall, VS, TRUNC)[0][:, 0] == 0).any()
    # key <-> block, the ends of the range
    for b in ((0, 0, 0), (-1, 2, -3), (-(1 << 20) + 1, (1 << 20) - 1, 0)):
        k = h.lib.ref_key(*b)
        out = np.zeros(3, np.int32)
        h.lib.ref_key_block(k, out.ctypes.data)
        assert out.tolist() == list(b) and k == int(ref.block_key(np.array(b))) and k != 0
    pts2 = np.array([[8 * VS * ((1 << 20) - 1) - 1.0, 0, 0], [8 * VS * (1 << 20) + 1.0, 0, 0]], np.float32)
    assert h.point_keys(pts2, VS, TRUNC)[1].tolist() == [True, False]


# ---- the tetrahedra --------------------------------------------------------------------------------------------------
def _corner(i):
    return np.array([(i >> k) & 1 for k in range(3)], dtype=np.float64)


def test_six_tetrahedra_tile_the_cube():
    h = ref.host()
    volume, faces = 0.0, {}
    for t in range(6):
        v = np.zeros(4, np.int32)
        positive = h.lib.ref_tet_corners(t, v.ctypes.data)
        want, orient = ref.tet_corners(t)
        assert tuple(v.tolist()) == want and bool(positive) == (orient > 0)
        p = np.array([_corner(i) for i in v])
        det = np.linalg.det(p[1:] - p[0])
        assert abs(abs(det) - 1.0) < 1e-12 and (det > 0) == bool(positive)
        volume += abs(det) / 6.0
        for tri in itertools.combinations(v.tolist(), 3):
            faces.setdefault(tuple(sorted(tri)), []).append(t)
    assert abs(volume - 1.0) < 1e-12
    for tri, users in faces.items():
        p = np.array([_corner(i) for i in tri])
        on_boundary = any((p[:, k] == p[0, k]).all() for k in range(3))     # the three corners share a coordinate: a cube face
        assert len(users) == (1 if on_boundary else 2), (tri, users)
    # the split of every cube face is the same on the opposite face: neighbouring cubes agree on the diagonal
    for k in range(3):
        lo = {tuple(sorted(i for i in tri)) for tri in faces if all(not (i >> k) & 1 for i in tri)}
        hi = {tuple(sorted(i & ~(1 << k) for i in tri)) for tri in faces if all((i >> k) & 1 for i in tri)}
        assert lo == hi and len(lo) == 2


def test_sixteen_cases_point_to_the_positive_side():
    h = ref.host()
    rng = np.random.default_rng(0)
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=np.float64)      # positively oriented
    assert np.linalg.det(P[1:] - P[0]) > 0
    for mask in range(16):
        code = int(h.lib.ref_tet_case(mask))
        want = ref.tet_case(mask)
        ntri = code & 3
        got = [[((code >> (4 + 4 * (3 * n + k))) & 3, (code >> (6 + 4 * (3 * n + k))) & 3) for k in range(3)] for n in range(ntri)]
        assert got == [[tuple(e) for e in tri] for tri in want], mask
        assert ntri == (0, 1, 2, 1, 0)[bin(mask).count("1")]
        for trial in range(20):
            f = np.where([(mask >> i) & 1 for i in range(4)], -1.0, 1.0) * rng.uniform(0.05, 1.0, 4)
            grad = np.linalg.solve(P[1:] - P[0], f[1:] - f[0])              # of the linear interpolant
            for tri in got:
                pts = []
                for i, j in tri:
                    assert (f[i] < 0) != (f[j] < 0)                         # every vertex lies on a crossing edge
                    s = f[i] / (f[i] - f[j])
                    pts.append(P[i] + s * (P[j] - P[i]))
                n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                assert np.dot(n, grad) > 0, (mask, tri)
            if ntri == 2:                                                   # the two triangles share the diagonal, opposite ways
                assert got[0][0] == got[1][0] and got[0][2] == got[1][1]


# ---- extraction ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    blocks, tsdf, weight = ref.sphere_volume(CENTRE, 1.0, VS, TRUNC, ORIGIN)
    tris, counts = ref.host().extract(blocks, tsdf, weight, VS, ORIGIN)
    for a in (blocks, tsdf, weight, tris, counts):
        a.setflags(write=False)
    return blocks, tsdf, weight, tris, counts


def test_extraction_bit_for_bit(sphere):
    blocks, tsdf, weight, tris, counts = sphere
    want, wcounts = ref.extract(blocks, tsdf, weight, VS, ORIGIN)
    print(f"sphere: {len(blocks)} blocks, {len(tris)} triangles")
    assert len(tris) == len(want) > 1000 and np.array_equal(counts, wcounts)
    assert np.array_equal(_bits(tris), _bits(want))
    # a random volume: every case of every tetrahedron, values of either sign next to zeros
    rng = np.random.default_rng(3)
    b2 = np.array(sorted(itertools.product((0, 1), (-1, 0), (2, 3)), key=lambda b: int(ref.block_key(np.array(b)))), np.int32)
    t2 = rng.uniform(-1, 1, (len(b2), 512)).astype(np.float32)
    t2[rng.uniform(size=t2.shape) < 0.05] = 0.0
    w2 = (rng.uniform(size=t2.shape) < 0.97).astype(np.float32)
    got, gc = ref.host().extract(b2, t2, w2, 0.3, (1.0, 2.0, 3.0))
    want, wc = ref.extract(b2, t2, w2, 0.3, (1.0, 2.0, 3.0))
    assert len(got) == len(want) > 5000 and np.array_equal(gc, wc) and np.array_equal(_bits(got), _bits(want))


def test_sphere_is_closed_oriented_and_round(sphere):
    ref.check_sphere_mesh(sphere[3])


def test_missing_block_and_zero_weight(sphere):
    blocks, tsdf, weight, tris, counts = sphere
    k = ref.drop_cases(blocks, counts)
    keep = np.arange(len(blocks)) != k
    part, _ = ref.host().extract(blocks[keep], tsdf[keep], weight[keep], VS, ORIGIN)
    ref.check_missing(tris, part, blocks, k, VS, ORIGIN)
    w0 = weight.copy()
    w0[k] = 0.0
    part2, c2 = ref.host().extract(blocks, tsdf, w0, VS, ORIGIN)
    assert c2[k] == 0 and np.array_equal(_bits(part2), _bits(part))
    want, _ = ref.extract(blocks, tsdf, w0, VS, ORIGIN)
    assert np.array_equal(_bits(part2), _bits(want))
    # one block alone: nothing crosses into an absent neighbour — only the 7^3 inner cubes can give triangles
    one, c1 = ref.host().extract(blocks[k:k + 1], tsdf[k:k + 1], weight[k:k + 1], VS, ORIGIN)
    g = np.floor((one.astype(np.float64).min(1) - np.asarray(ORIGIN)) / VS - 0.5 + 1e-6).astype(np.int64) - 8 * blocks[k]
    assert len(one) > 0 and (g >= 0).all() and (g <= 6).all()
    # a min_weight above every weight: nothing
    assert len(ref.host().extract(blocks, tsdf, weight, VS, ORIGIN, min_weight=2.0)[0]) == 0


# ---- integration -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_ratio", [0.0, 1.0])
@pytest.mark.parametrize("hfov,vfov", [(360.0, 60.0), (120.0, 60.0)])
def test_integration_against_float64(hfov, vfov, depth_ratio):
    blocks, cams, maps = ref.integration_case(hfov, vfov)
    t, w = np.ones((len(blocks), 512), np.float32), np.zeros((len(blocks), 512), np.float32)
    for cam, am in zip(cams, maps):
        t, w, pixel = ref.host().integrate(blocks, t, w, am, cam, VS, TRUNC, ORIGIN, 0.5, 0.1, depth_ratio)
    assert set(np.unique(w).tolist()) <= {0.0, 1.0, 2.0} and np.abs(t).max() <= 1.0
    ref.compare_with_float64(blocks, cams, maps, depth_ratio, t, w, f"{hfov:.0f} deg, depth_ratio {depth_ratio}")
    if hfov < 360:
        assert (pixel < 0).mean() > 0.3                      # most of the shell lies outside a 120-degree image
