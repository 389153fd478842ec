"""include/sls_poisson_math.h on the host, as plain C99 — the very functions the kernels run — against the NumPy restatement
(poisson_ref.py) bit for bit: field, b, diag, every CG vector after k passes, iso, chi, density; the inner product's order;
the operator's symmetry and definiteness; the restatement against a float64 direct solve; the capped sphere.

MEASURED HERE (the restatement's own figures, what the two bars below are derived from):
  two blocks, 1 500 samples of a tilted plane (seed 0), screening 4, tol 1e-6: 49 passes,
      |chi - chi*|_inf / |chi*|_inf = 1.49e-6 against np.linalg.solve in float64           -> bar 2 x 1.49e-6 = 2.99e-6
      (seeds 1 and 2 gave 1.53e-6 and 1.75e-6; the factor 2 covers float32 storage at another seed)
  capped unit sphere, 18 077 samples, h = 0.1, margin 3 voxels, 64 blocks, screening 4, tol 1e-4: 101 passes, closed,
      V - E + F = 2, mean radial error of the vertices outside the cap 6.32 mm                 -> bar 1.5 x 6.32 mm = 9.48 mm
      (the largest radial error inside the extrapolated cap: 60 mm)"""
import shutil

import numpy as np
import pytest

import poisson_ref as ref
import tsdf_ref

DIRECT_SOLVE_MEASURED = 1.4929110651776022e-06
SPHERE_MEAN_ERROR_MEASURED = 0.00631701059279022


@pytest.fixture(scope="module")
def host():
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    return ref.host()


def three_block_cloud(M=2000, seed=11):
    """blocks at negative and positive coordinates, two of them face to face; points inside them and a few around"""
    rng = np.random.default_rng(seed)
    blocks = ref.sort_blocks([[-2, -1, 0], [-1, -1, 0], [1, 0, -3]])
    h, origin = 0.125, (0.03, -0.07, 0.011)
    k = rng.integers(0, 3, M)
    local = rng.uniform(-0.3, 8.3, (M, 3))                  # a few fall outside: dropped corners, dropped points
    pts = (np.asarray(origin) + (8 * blocks[k] + local) * h).astype(np.float32)
    nrm = rng.normal(size=(M, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return blocks, pts, nrm, h, origin


def test_constants(host):
    assert host.consts() == [ref.FLAG_CONVERGED, ref.FLAG_NOT_PD, ref.FLAG_EMPTY, ref.STATUS_WORDS, ref.REDUCE]


def test_worked_by_hand(host):
    blocks = ref.sort_blocks([[0, 0, 0]])
    h = 0.5                                                 # exact in binary: u is an integer or a half
    node = np.array([[(2 + 0.5) * h, (3 + 0.5) * h, (5 + 0.5) * h]], np.float32)        # on node (2, 3, 5): weight 1
    n = np.array([[0.25, -0.5, 1.0]], np.float32)
    field, status = host.splat(node, n, blocks, h)
    want = np.zeros((1, 512, 4), np.float32)
    want[0, 2 | 3 << 3 | 5 << 6] = [0.25, -0.5, 1.0, 1.0]
    ref.same_bits(field, want, "a point on a node")
    assert status.tolist() == [0, 0, 0, 1]
    centre = np.array([[3 * h, 4 * h, 6 * h]], np.float32)                              # the centre of cube (2, 3, 5): 8 x 0.125
    field, _ = host.splat(centre, n, blocks, h)
    want[:] = 0
    for c in range(8):
        want[0, (2 + (c & 1)) | (3 + ((c >> 1) & 1)) << 3 | (5 + (c >> 2)) << 6] = [0.03125, -0.0625, 0.125, 0.125]
    ref.same_bits(field, want, "a point at a cube centre")
    ref.same_bits(ref.splat(centre, n, blocks, h)[0], want, "... restated")
    # a point in the last cell of the block: four corners have no block, the point is counted once
    field, status = host.splat(np.array([[7.75 * h, 1 * h, 1 * h]], np.float32), n, blocks, h)
    assert status.tolist() == [0, 0, 1, 1] and np.isclose(field[..., 3].sum(), 0.75)
    # a point whose cell lies in no block is dropped whole; non-finite values and far points are counted, not splatted
    bad = np.array([[-0.2 * h, h, h], [np.nan, 0, 0], [1, 1, 1], [3e7, 0, 0]], np.float32)
    nb = np.array([[0, 0, 1], [0, 0, 1], [np.inf, 0, 0], [0, 0, 1]], np.float32)
    field, status = host.splat(bad, nb, blocks, h)
    assert status.tolist() == [2, 1, 1, 1] and not field.any()
    fr, sr = ref.splat(bad, nb, blocks, h)
    assert sr.tolist() == [2, 1, 1, 1] and not fr.any()


def test_splat_bit_for_bit(host):
    blocks, pts, nrm, h, origin = three_block_cloud()
    want, ws = ref.splat(pts, nrm, blocks, h, origin)
    got, gs = host.splat(pts, nrm, blocks, h, origin)
    ref.same_bits(got, want, "field")
    assert gs.tolist() == ws.tolist() and ws[2] > 50 and ws[0] == ws[1] == 0
    assert (want[..., 3] > 0).sum() > 1000
    # many points in one cell: the order inside the cell is the input order
    rng = np.random.default_rng(3)
    cell = (np.asarray(origin) + (8 * blocks[1] + [3, 4, 5] + rng.uniform(0.5, 1.5, (3000, 3))) * h).astype(np.float32)
    n2 = rng.normal(size=(3000, 3)).astype(np.float32) * 10.0 ** rng.integers(-6, 6, (3000, 1)).astype(np.float32)
    want, _ = ref.splat(cell, n2, blocks, h, origin)
    got, _ = host.splat(cell, n2, blocks, h, origin)
    ref.same_bits(got, want, "3000 points in one cell")
    assert (want[..., 3] > 0).sum() == 8 and np.isclose(want[..., 3].astype(np.float64).sum(), 3000.0)


def test_system_solve_and_density_bit_for_bit(host):
    blocks, pts, nrm, h, origin = three_block_cloud()
    field, _ = ref.splat(pts, nrm, blocks, h, origin)
    nb = host.neighbours(blocks)
    assert nb.tolist() == [[-1] * 6, [-1, 2, -1, -1, -1, -1], [1, -1, -1, -1, -1, -1]]
    for alpha in (4.0, 0.37):
        for k in (0, 1, 2, 7, 300):
            want, got = ref.solve(blocks, field, alpha, k, 1e-5), host.solve(blocks, field, alpha, k, 1e-5)
            for name in ("b", "diag", "x", "r", "z", "p", "q"):
                ref.same_bits(got["vectors"][name], want["vectors"][name], f"alpha {alpha}, {k} passes: {name}")
            ref.same_bits(got["chi"], want["chi"], f"alpha {alpha}, {k} passes: chi")
            assert got["status"].tolist() == want["status"].tolist(), (alpha, k)
        st = ref.status_dict(want["status"])
        assert st["flags"] == ref.FLAG_CONVERGED and 7 < st["iterations"] < 300 and st["rr"] <= 1e-10 * st["bb"]
    # an empty field: x = 0, CONVERGED | EMPTY, no pass
    for solver in (ref.solve, host.solve):
        out = solver(blocks, np.zeros_like(field), 4.0, 10, 1e-4)
        assert out["status"][:3].tolist() == [0, ref.FLAG_CONVERGED | ref.FLAG_EMPTY, 3] and not out["chi"].any()
    for sweeps in (0, 1, 2, 3):
        ref.same_bits(host.density(blocks, field, sweeps), ref.density(blocks, field, sweeps), f"density after {sweeps} sweeps")
    assert np.array_equal(ref.density(blocks, field, 0), field[..., 3])
    d2 = ref.density(blocks, field, 2)
    assert (d2 > 0).sum() > (field[..., 3] > 0).sum() and abs(d2.sum() / field[..., 3].sum() - 1) < 0.2


def test_the_inner_product_follows_the_stated_order(host):
    rng = np.random.default_rng(8)

    def block(x):                                           # 512 values -> the block's partial, in plain loops
        waves = []
        for w in range(8):
            lanes = [x[64 * w + l] for l in range(64)]
            for off in (32, 16, 8, 4, 2, 1):
                lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
            waves.append(lanes[0])
        s = waves[0]
        for w in range(1, 8):
            s = s + waves[w]
        return s

    def plain(a, b):
        prod = a.astype(np.float64) * b.astype(np.float64)
        threads = [0.0] * 512
        for k in range(len(prod)):
            threads[k % 512] = threads[k % 512] + block(prod[k])
        return block(threads)
    for B in (1, 2, 3):
        a = (rng.normal(size=(B, 512)) * 10.0 ** rng.integers(-6, 6, (B, 512))).astype(np.float32)
        b = (rng.normal(size=(B, 512)) * 10.0 ** rng.integers(-6, 6, (B, 512))).astype(np.float32)
        assert ref.bits64(ref.dot(a, b)) == ref.bits64(plain(a, b)) == ref.bits64(host.dot(a, b)), B
    # past one round of the final step (the 1 089 blocks of the GPU suite's slab): one value per block, so that the
    # plain loops stay short — the block's partial of a lone value in lane 0 is that value
    for B in (511, 512, 513, 1089):
        a = np.zeros((B, 512), np.float32)
        b = np.ones((B, 512), np.float32)
        a[:, 0] = (rng.normal(size=B) * 10.0 ** rng.integers(-6, 6, B)).astype(np.float32)
        threads = [0.0] * 512
        for k in range(B):
            threads[k % 512] = threads[k % 512] + float(a[k, 0])
        assert ref.bits64(ref.dot(a, b)) == ref.bits64(block(threads)) == ref.bits64(host.dot(a, b)), B
        full = (rng.normal(size=(B, 512)) * 10.0 ** rng.integers(-3, 3, (B, 512))).astype(np.float32)
        assert ref.bits64(ref.dot(full, full)) == ref.bits64(host.dot(full, full)), B


def test_the_operator_is_symmetric_positive_definite():
    """Assembled from unit vectors on a block with neighbours on three sides; at alpha = 0 the constant vector is null."""
    rng = np.random.default_rng(4)
    blocks = ref.sort_blocks([[0, 0, 0], [1, 0, 0], [0, -1, 0]])
    h = 0.1
    pts = rng.uniform([0.0, -0.8, 0.0], [1.6, 0.8, 0.8], (400, 3)).astype(np.float32)
    field, _ = ref.splat(pts, np.tile(np.float32([0, 0, 1]), (400, 1)), blocks, h)
    nbr = ref.neighbour_slots(blocks)
    n = 3 * 512
    for alpha in (4.0, 0.0):
        _, diag = ref.system(blocks, field, alpha, nbr)
        A = np.zeros((n, n))
        e = np.zeros((3, 512), np.float32)
        for j in range(n):
            e.reshape(-1)[j] = 1.0
            A[:, j] = ref.apply(nbr, diag, e).reshape(-1)
            e.reshape(-1)[j] = 0.0
        assert np.array_equal(A, A.T)
        lam = np.linalg.eigvalsh(A)
        if alpha > 0:
            assert lam[0] > 0, lam[:3]
        else:
            assert np.array_equal(ref.apply(nbr, diag, np.ones((3, 512), np.float32)), np.zeros((3, 512), np.float32))
            assert abs(lam[0]) < 1e-9 and lam[1] > 1e-6         # one component: one null vector
    # the matrix the float64 reference assembles is the same one where the float32 diagonal is exact
    A64, _ = ref.operator_matrix(blocks, field, 0.0)
    assert np.array_equal(A64, A)


def two_block_plane(seed):
    rng = np.random.default_rng(seed)
    blocks = ref.sort_blocks([[-1, 0, 0], [0, 0, 0]])
    xy = rng.uniform([-0.8, 0.0], [0.8, 0.8], (1500, 2))
    nrm = np.array([0.2, -0.1, 1.0])
    nrm /= np.linalg.norm(nrm)
    z = 0.4 - (nrm[0] * xy[:, 0] + nrm[1] * (xy[:, 1] - 0.4)) / nrm[2] + 0.005 * rng.normal(size=1500)
    return blocks, np.concatenate([xy, z[:, None]], 1).astype(np.float32), np.tile(nrm.astype(np.float32), (1500, 1)), 0.1


@pytest.mark.parametrize("seed", [0, 1])
def test_against_a_direct_solve_in_float64(seed):
    """1 024 unknowns: np.linalg.solve of the float64 system, the iso-level in float64; the restatement at tol = 1e-6."""
    blocks, pts, nrm, h = two_block_plane(seed)
    field, _ = ref.splat(pts, nrm, blocks, h)
    A, b = ref.operator_matrix(blocks, field, 4.0)
    x = np.linalg.solve(A, b)
    W = field.reshape(-1, 4)[:, 3].astype(np.float64)
    chi_star = x - (W @ x) / W.sum()
    out = ref.solve(blocks, field, 4.0, 1000, 1e-6)
    st = ref.status_dict(out["status"])
    err = np.abs(out["chi"].reshape(-1) - chi_star).max() / np.abs(chi_star).max()
    print(f"seed {seed}: {st['iterations']} passes, |chi - chi*| / |chi*| = {err:.3e} (bar {2 * DIRECT_SOLVE_MEASURED:.3e})")
    assert st["flags"] == ref.FLAG_CONVERGED
    assert err <= 2 * DIRECT_SOLVE_MEASURED
    # chi grows along the normals: the plane's upper side is outside
    up = out["chi"].reshape(2, 8, 8, 8)
    assert (up[:, 7] > 0).all() and (up[:, 0] < 0).all()


def test_the_capped_sphere_is_closed(host):
    pts, nrm = ref.capped_sphere()
    blocks = ref.blocks_around(pts)
    field, status = ref.splat(pts, nrm, blocks, ref.VS, ref.ORIGIN)
    assert status.tolist() == [0, 0, 0, 1]
    out = ref.solve(blocks, field, 4.0, 300, 1e-4)
    st = ref.status_dict(out["status"])
    tris, _ = tsdf_ref.extract(blocks, out["chi"], np.ones_like(out["chi"]), ref.VS, ref.ORIGIN, 1.0)
    rep = ref.sphere_report(tris)
    print(f"{len(pts)} samples, {len(blocks)} blocks, {st['iterations']} passes: {rep}")
    assert st["flags"] == ref.FLAG_CONVERGED
    assert rep["closed"] and rep["euler"] == 2 and rep["outward"] and rep["cap_vertices"] > 50
    assert rep["mean_error"] <= 1.5 * SPHERE_MEAN_ERROR_MEASURED
    assert rep["cap_error"] <= ref.VS                       # the cap is closed within a voxel of the sphere
    ref.same_bits(tsdf_ref.host().extract(blocks, host.solve(blocks, field, 4.0, 300, 1e-4)["chi"], np.ones_like(out["chi"]), ref.VS,
                                          ref.ORIGIN, 1.0)[0], tris, "the header's mesh")
