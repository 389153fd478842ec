"""include/sls_icp_math.h on the host, as plain C99 — the very functions the kernels run — against the NumPy restatement
(icp_ref.py) bit for bit: transform, terms, solve; the Cayley update is a rotation; cases worked by hand."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sls_icp_math.h"
/* transform: in T[12] doubles, M int32, M x 3 floats; out M x 3 floats
 * terms:     in method, M int32, M int32 (inlier), 3 arrays of M x 3 floats (moved, q, n); out M x 29 doubles
 * solve:     in S[29] doubles, T[12] doubles, damping, eps_rot, eps_trans doubles, min_inliers int32;
 *            out flags int32, T[12] doubles, xi[6] doubles
 * consts:    out TERMS, BLOCK, the three flags, sizeof(SlsIcpParams) as int32, the defaults */
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    if (!strcmp(argv[1], "transform")) {
        double T[12]; int M;
        if (fread(T, 8, 12, in) != 12 || fread(&M, 4, 1, in) != 1) return 2;
        float *p = malloc(12 * (size_t)M + 4), *q = malloc(12 * (size_t)M + 4);
        if (fread(p, 12, M, in) != (size_t)M) return 2;
        for (int i = 0; i < M; ++i) sls_icp_transform(T, p + 3 * i, q + 3 * i);
        fwrite(q, 12, M, out);
    } else if (!strcmp(argv[1], "terms")) {
        int h[2];
        if (fread(h, 4, 2, in) != 2) return 2;
        const size_t M = (size_t)h[1];
        int32_t *inl = malloc(4 * M + 4);
        float *mv = malloc(12 * M + 4), *q = malloc(12 * M + 4), *n = malloc(12 * M + 4);
        double *acc = malloc(8 * SLS_ICP_TERMS * M + 8);
        if (fread(inl, 4, M, in) != M || fread(mv, 12, M, in) != M || fread(q, 12, M, in) != M || fread(n, 12, M, in) != M) return 2;
        for (size_t i = 0; i < M; ++i) sls_icp_terms(h[0], inl[i], mv + 3 * i, q + 3 * i, n + 3 * i, acc + SLS_ICP_TERMS * i);
        fwrite(acc, 8 * SLS_ICP_TERMS, M, out);
    } else if (!strcmp(argv[1], "solve")) {
        double S[SLS_ICP_TERMS], T[12], par[3], xi[6]; int32_t mi;
        if (fread(S, 8, SLS_ICP_TERMS, in) != SLS_ICP_TERMS || fread(T, 8, 12, in) != 12 || fread(par, 8, 3, in) != 3 || fread(&mi, 4, 1, in) != 1) return 2;
        SlsIcpParams prm;
        sls_icp_defaults(&prm);
        prm.damping = par[0]; prm.eps_rot = par[1]; prm.eps_trans = par[2]; prm.min_inliers = mi;
        int32_t flags = sls_icp_solve(S, &prm, T, xi);
        fwrite(&flags, 4, 1, out); fwrite(T, 8, 12, out); fwrite(xi, 8, 6, out);
    } else if (!strcmp(argv[1], "consts")) {
        SlsIcpParams prm;
        sls_icp_defaults(&prm);
        int32_t c[9] = { SLS_ICP_TERMS, SLS_ICP_BLOCK, SLS_ICP_FLAG_CONVERGED, SLS_ICP_FLAG_FEW, SLS_ICP_FLAG_NOT_PD, (int32_t)sizeof(SlsIcpParams),
                         prm.method, prm.iterations, prm.min_inliers };
        double d[4] = { prm.damping, prm.eps_rot, prm.eps_trans, (double)prm.max_distance };
        fwrite(c, 4, 9, out); fwrite(d, 8, 4, out);
    } else return 3;
    fclose(in); fclose(out);
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("icp_math")
    (d / "icp_math.c").write_text(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           str(d / "icp_math.c"), "-o", str(d / "icp_math"), "-lm"])
    return str(d / "icp_math")


def run(exe, tmp_path, mode, blob):
    (tmp_path / "in.bin").write_bytes(blob)
    subprocess.check_call([exe, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return (tmp_path / "out.bin").read_bytes()


def host_solve(exe, tmp_path, S, T, damping=1e-9, eps_rot=1e-7, eps_trans=1e-7, min_inliers=6):
    raw = run(exe, tmp_path, "solve", np.asarray(S, np.float64).tobytes() + np.asarray(T, np.float64).tobytes()
              + np.array([damping, eps_rot, eps_trans], np.float64).tobytes() + np.array([min_inliers], np.int32).tobytes())
    return int(np.frombuffer(raw[:4], np.int32)[0]), np.frombuffer(raw[4:100], np.float64), np.frombuffer(raw[100:148], np.float64)


def host_terms(exe, tmp_path, method, inlier, moved, q, n):
    M = len(moved)
    raw = run(exe, tmp_path, "terms", np.array([method, M], np.int32).tobytes() + np.asarray(inlier, np.int32).tobytes()
              + np.ascontiguousarray(moved, np.float32).tobytes() + np.ascontiguousarray(q, np.float32).tobytes()
              + np.ascontiguousarray(n, np.float32).tobytes())
    return np.frombuffer(raw, np.float64).reshape(M, ref.TERMS)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def some_pose(rng):
    return ref.pose12(ref.rotation(rng.normal(size=3), rng.uniform(0.0, 3.0)), rng.normal(size=3) * 5)


def test_constants_and_defaults(exe, tmp_path):
    raw = run(exe, tmp_path, "consts", b"")
    c, d = np.frombuffer(raw[:36], np.int32), np.frombuffer(raw[36:], np.float64)
    assert list(c[:5]) == [ref.TERMS, ref.BLOCK, ref.FLAG_CONVERGED, ref.FLAG_FEW, ref.FLAG_NOT_PD]
    assert c[5] == 40 and c[6] == ref.PLANE and c[7] == 30 and c[8] == ref.DEFAULTS["min_inliers"]
    assert list(d[:3]) == [ref.DEFAULTS["damping"], ref.DEFAULTS["eps_rot"], ref.DEFAULTS["eps_trans"]] and d[3] == 1.0


def test_transform_bit_for_bit(exe, tmp_path):
    rng = np.random.default_rng(1)
    pts = (rng.normal(size=(4001, 3)) * 30).astype(np.float32)
    for _ in range(4):
        T = some_pose(rng)
        raw = run(exe, tmp_path, "transform", T.tobytes() + np.array([len(pts)], np.int32).tobytes() + pts.tobytes())
        same_bits(np.frombuffer(raw, np.float32).reshape(-1, 3), ref.transform(T, pts), "transform")


@pytest.mark.parametrize("method", [ref.PLANE, ref.POINT])
def test_terms_bit_for_bit(exe, tmp_path, method):
    rng = np.random.default_rng(2 + method)
    M = 3000
    moved = (rng.normal(size=(M, 3)) * 20).astype(np.float32)
    q = (moved + rng.normal(size=(M, 3)) * 0.1).astype(np.float32)
    n = rng.normal(size=(M, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    inlier = rng.random(M) < 0.8
    want = ref.terms(method, inlier, moved, q, n)
    same_bits(host_terms(exe, tmp_path, method, inlier, moved, q, n), want, "terms")
    assert np.all(want[~inlier] == 0.0) and np.all(want[inlier, 28] == 1.0)
    # J^T J against a plain matrix product, to round-off
    i = int(np.flatnonzero(inlier)[0])
    p, d = moved[i].astype(np.float64), moved[i].astype(np.float64) - q[i].astype(np.float64)
    if method == ref.PLANE:
        J = np.concatenate([n[i].astype(np.float64), np.cross(p, n[i].astype(np.float64))])[None]
        r = np.array([n[i].astype(np.float64) @ d])
    else:
        K = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        J, r = np.concatenate([np.eye(3), -K], 1), d
    H = J.T @ J
    assert np.allclose(want[i, :21], H[np.triu_indices(6)], rtol=1e-13, atol=1e-13)
    assert np.allclose(want[i, 21:27], J.T @ r, rtol=1e-13, atol=1e-13) and np.isclose(want[i, 27], r @ r, rtol=1e-13)


def random_system(rng, M=400, method=ref.PLANE, scale=0.01):
    moved = (rng.normal(size=(M, 3)) * 5).astype(np.float32)
    n = rng.normal(size=(M, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    q = (moved + rng.normal(size=(M, 3)) * scale).astype(np.float32)
    return ref.reduce_terms(ref.terms(method, np.ones(M, bool), moved, q, n))


def test_solve_bit_for_bit(exe, tmp_path):
    rng = np.random.default_rng(5)
    seen = set()
    for trial in range(40):
        S = random_system(rng, method=trial % 2, scale=10.0 ** -rng.integers(1, 9))
        T = some_pose(rng)
        kw = dict(damping=[1e-9, 0.0, 1e-3][trial % 3], eps_rot=[1e-7, 1e-2][trial % 2], eps_trans=[1e-7, 1e-1][trial % 2],
                  min_inliers=[6, 401][trial % 5 == 4])
        flags, T2, xi = host_solve(exe, tmp_path, S, T, **kw)
        wf, wT, wxi = ref.solve(S, T, **kw)
        assert flags == wf
        same_bits(T2, wT, "pose"); same_bits(xi, wxi, "xi")
        seen.add(flags)
    assert seen == {0, ref.FLAG_CONVERGED, ref.FLAG_FEW}


def test_the_cayley_update_is_a_rotation(exe, tmp_path):
    """R^T R - I of the updated pose at round-off, for steps from tiny to a radian; and the angle is 2 atan(|w| / 2)."""
    rng = np.random.default_rng(6)
    for mag in (1e-9, 1e-4, 1e-2, 0.3, 1.0):
        w = rng.normal(size=3)
        w *= mag / np.linalg.norm(w)
        xi = np.concatenate([rng.normal(size=3) * mag, w])
        # a system whose solution is exactly -H^-1 b = xi: H = I (damping 0), b = -xi
        S = np.zeros(ref.TERMS)
        S[[0, 6, 11, 15, 18, 20]] = 1.0
        S[21:27] = -xi
        S[28] = 100.0
        flags, T, got = host_solve(exe, tmp_path, S, ref.IDENTITY, damping=0.0)
        assert flags in (0, ref.FLAG_CONVERGED)
        same_bits(got, xi, "xi of the identity system")
        R = T.reshape(3, 4)[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 4 * np.finfo(np.float64).eps
        assert np.linalg.det(R) > 0
        angle = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        assert np.isclose(angle, 2 * np.arctan(mag / 2), rtol=1e-6, atol=1e-12) or mag < 1e-6
        assert np.allclose(R @ w, w, atol=1e-15 + 1e-15 * mag)                    # the axis is kept
        same_bits(T.reshape(3, 4)[:, 3].copy(), xi[:3].copy(), "t = dR 0 + v")


def test_worked_by_hand(exe, tmp_path):
    # one point on one plane: p' = (1, 2, 0.5), q = (1, 2, 0), n = e_z: r = 0.5, J = [0, 0, 1, 2, -1, 0]
    acc = host_terms(exe, tmp_path, ref.PLANE, [1], [[1, 2, 0.5]], [[1, 2, 0]], [[0, 0, 1]])[0]
    J, r = np.array([0, 0, 1.0, 2.0, -1.0, 0]), 0.5
    assert np.array_equal(acc[:21], np.outer(J, J)[np.triu_indices(6)])
    assert np.array_equal(acc[21:27], J * r) and acc[27] == 0.25 and acc[28] == 1.0
    same_bits(acc[None], ref.terms(ref.PLANE, [True], np.array([[1, 2, 0.5]], np.float32), np.array([[1, 2, 0]], np.float32),
                                   np.array([[0, 0, 1]], np.float32)), "one point")
    # the same pair, point-to-point: sum r^2 = 0.25, the translation block is the identity
    acc = host_terms(exe, tmp_path, ref.POINT, [1], [[1, 2, 0.5]], [[1, 2, 0]], [[0, 0, 0]])[0]
    assert acc[0] == acc[6] == acc[11] == 1.0 and acc[1] == acc[2] == acc[7] == 0.0 and acc[27] == 0.25 and acc[23] == 0.5
    # a pair beyond the gate contributes nothing
    assert np.all(host_terms(exe, tmp_path, ref.PLANE, [0], [[1, 2, 0.5]], [[1, 2, 0]], [[0, 0, 1]]) == 0.0)

    # a pure translation along the normals, recovered in ONE step: three lattice walls, the source shifted by
    # (1/8, -1/16, 1/32) (exact in float32), each point paired with its own counterpart, axis normals
    tgt, _ = ref.walls(5)
    nrm = np.repeat(np.eye(3, dtype=np.float32), 25, axis=0)
    shift = np.array([0.125, -0.0625, 0.03125], np.float32)
    S = ref.reduce_terms(ref.terms(ref.PLANE, np.ones(75, bool), tgt + shift, tgt, nrm))
    flags, T, xi = host_solve(exe, tmp_path, S, ref.IDENTITY, damping=0.0)
    assert flags == 0
    assert np.abs(xi[:3] + shift).max() < 1e-14 and np.abs(xi[3:]).max() < 1e-14
    # ... and at the solution the step is zero: converged
    S = ref.reduce_terms(ref.terms(ref.PLANE, np.ones(75, bool), tgt, tgt, nrm))
    flags, T, xi = host_solve(exe, tmp_path, S, ref.IDENTITY, damping=0.0)
    assert flags == ref.FLAG_CONVERGED and np.all(xi == 0.0) and np.array_equal(T, ref.IDENTITY)

    # one plane holds three freedoms only: without damping the system is not positive definite and the pose is kept
    one = tgt[50:], nrm[50:]
    S = ref.reduce_terms(ref.terms(ref.PLANE, np.ones(25, bool), one[0] + np.float32([0, 0, 0.125]), one[0], one[1]))
    T0 = ref.pose12(ref.rotation([1, 2, 3], 0.3), [1, 2, 3])
    flags, T, xi = host_solve(exe, tmp_path, S, T0, damping=0.0)
    assert flags == ref.FLAG_NOT_PD and np.all(xi == 0.0)
    same_bits(T, T0, "the pose is kept")
    assert ref.solve(S, T0, 0.0, 1e-7, 1e-7, 6)[0] == ref.FLAG_NOT_PD
    # too few inliers keeps it too
    flags, T, xi = host_solve(exe, tmp_path, S, T0, min_inliers=26)
    assert flags == ref.FLAG_FEW
    same_bits(T, T0, "the pose is kept")


def test_the_sum_follows_the_stated_order():
    """reduce_terms against the header's four steps written as plain loops, on sizes on both sides of every boundary."""
    rng = np.random.default_rng(8)
    for M in (1, 63, 64, 65, 256, 257, 700):
        rows = rng.normal(size=(M, ref.TERMS)) * 10.0 ** rng.integers(-8, 8, size=(M, 1))
        nblocks = (M + 255) // 256
        padded = np.zeros((nblocks * 256, ref.TERMS)); padded[:M] = rows

        def block(x):                                   # (256, 29) -> (29,)
            waves = []
            for w in range(4):
                lanes = [x[64 * w + l] for l in range(64)]
                for off in (32, 16, 8, 4, 2, 1):
                    lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
                waves.append(lanes[0])
            return ((waves[0] + waves[1]) + waves[2]) + waves[3]
        partials = [block(padded[256 * b:256 * b + 256]) for b in range(nblocks)]
        threads = np.zeros((256, ref.TERMS))
        for b, p in enumerate(partials):
            threads[b % 256] = threads[b % 256] + p
        same_bits(block(threads), ref.reduce_terms(rows), f"M={M}")
