"""include/sls_normals_math.h on the host, as plain C99 — the very functions the kernel runs — against the NumPy restatement
(normals_ref.py) bit for bit, the restatement's two forms against each other, cases worked by hand, and the Jacobi solve
against LAPACK (np.linalg.eigh) on the same float64 covariance."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import normals_ref as ref
import outlier_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "sls_normals_math.h"
/* in: [M, k] int32, radius, viewpoint[3] (floats), M x 3 floats, M x k floats (d2 rows), M x k int32 (index rows)
 * out: M x 3 floats (normals), M int32 (counts), M x 3 floats (eigenvalues) */
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int h[2];
    float par[4];
    if (argc != 3 || !in || !out || fread(h, 4, 2, in) != 2 || fread(par, 4, 4, in) != 4) return 2;
    const size_t M = (size_t)h[0], k = (size_t)h[1];
    if (h[1] < 1 || h[1] > SLS_NORMALS_NN_MAX || SLS_NORMALS_SWEEPS != %d) return 3;
    float *xyz = malloc(12 * M + 4), *d2 = malloc(4 * M * k + 4), *nrm = malloc(12 * M + 4), *eig = malloc(12 * M + 4);
    int32_t *idx = malloc(4 * M * k + 4), *cnt = malloc(4 * M + 4);
    if (fread(xyz, 12, M, in) != M || fread(d2, 4 * k, M, in) != M || fread(idx, 4 * k, M, in) != M) return 2;
    for (size_t i = 0; i < M; ++i)
        cnt[i] = sls_normals_point(xyz, (int)i, d2 + i * k, idx + i * k, (int)k, par[0], par + 1, nrm + 3 * i, eig + 3 * i);
    fwrite(nrm, 12, M, out); fwrite(cnt, 4, M, out); fwrite(eig, 12, M, out);
    fclose(in); fclose(out);
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("normals_math")
    (d / "normals_math.c").write_text(PROGRAM.replace("SLS_NORMALS_SWEEPS != %d", f"SLS_NORMALS_SWEEPS != {ref.SWEEPS}"))
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           str(d / "normals_math.c"), "-o", str(d / "normals_math"), "-lm"])
    return str(d / "normals_math")


def run_host(exe, tmp_path, points, d2, index, radius, viewpoint):
    M, k = index.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([M, k], np.int32).tobytes())
        f.write(np.array([np.inf if radius is None else radius, *viewpoint], np.float32).tobytes())
        f.write(np.ascontiguousarray(points, np.float32).tobytes() + np.ascontiguousarray(d2, np.float32).tobytes()
                + np.ascontiguousarray(index, np.int32).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    return {"normals": np.frombuffer(raw[:12 * M], np.float32).reshape(M, 3), "count": np.frombuffer(raw[12 * M:16 * M], np.int32),
            "eigenvalues": np.frombuffer(raw[16 * M:], np.float32).reshape(M, 3)}


def same(got, want, what):
    assert np.array_equal(got["count"], want["count"]), what
    for key in ("normals", "eigenvalues"):
        bad = np.flatnonzero((got[key].view(np.uint32) != want[key].view(np.uint32)).any(1))
        assert bad.size == 0, f"{what}: {key} differ in {bad.size} rows, first {bad[:3]}: {got[key][bad[:3]]} {want[key][bad[:3]]}"


@functools.lru_cache(maxsize=None)
def cloud(M):
    pts = outlier_ref.filter_cloud(M, 11 * M) if M > 10 else (np.arange(3 * M).reshape(M, 3) % 5 / 16.0).astype(np.float32)
    return pts, ref.lists(pts, 64)


@pytest.mark.parametrize("M", [1, 2, 3, 65, 257, 1500])
def test_header_equals_the_restatement_bit_for_bit(exe, tmp_path, M):
    pts, full = cloud(M)
    view = (0.5, -3.0, 20.0)
    for k in (1, 3, 4, 20, 33, 64):
        for radius in (0.25, 1.0, None):
            want = ref.normals(pts, k, radius, view, full=full)
            got = run_host(exe, tmp_path, pts, full[0][:, :k], full[1][:, :k], radius, view)
            same(got, want, f"M={M} k={k} radius={radius}")
            assert np.all(want["count"] >= 1) and np.all(want["count"] <= min(k, M))
            if radius is None:
                assert np.all(want["count"] == min(k, M))


def test_the_two_forms_of_the_restatement_agree():
    """The array form against the header written out with Python floats and math.sqrt, point by point."""
    pts, full = cloud(257)
    view = (1.0, 2.0, -30.0)
    for k, radius in ((20, 1.0), (64, None), (5, 0.25)):
        want = ref.normals(pts, k, radius, view, full=full)
        for i in range(0, 257, 3):
            nrm, n, eig = ref.normal_scalar(pts, full[0][i, :k], full[1][i, :k], i, radius, view)
            assert n == want["count"][i]
            assert np.array_equal(nrm.view(np.uint32), want["normals"][i].view(np.uint32)), (k, radius, i)
            assert np.array_equal(eig.view(np.uint32), want["eigenvalues"][i].view(np.uint32)), (k, radius, i)
    assert (ref.normals(pts, 5, 0.25, view, full=full)["count"] < 3).any()


def test_worked_by_hand(exe, tmp_path):
    def both(pts, k, radius, view):
        pts = np.asarray(pts, np.float32)
        d2, idx = ref.lists(pts, k)
        want = ref.normals(pts, k, radius, view)
        same(run_host(exe, tmp_path, pts, d2, idx, radius, view), want, "by hand")
        return want
    # the exact plane z = 0: (0, 0, +-1) by the viewpoint's side, the two in-plane eigenvalues above an exact 0
    g = np.array([[x, y, 0.0] for x in range(-3, 4) for y in range(-3, 4)], np.float32) / 4
    up, down = both(g, 9, None, (0, 0, 5)), both(g, 9, None, (0.25, 0, -5))
    assert np.all(up["normals"] == (0, 0, 1)) and np.all(down["normals"] == (0, 0, -1))
    assert np.all(up["eigenvalues"][:, 0] == 0) and np.all(up["eigenvalues"][:, 1] > 0)
    # every point the same: a zero matrix, every rotation skipped, index 0 -> (+-1, 0, 0) by the viewpoint's side
    same_pt = np.tile(np.array([[2.0, 1.0, -1.0]], np.float32), (12, 1))
    assert np.all(both(same_pt, 8, 0.5, (10, 0, 0))["normals"] == (1, 0, 0))
    res = both(same_pt, 8, 0.5, (-10, 50, 50))
    assert np.all(res["normals"] == (-1, 0, 0)) and np.all(res["eigenvalues"] == 0) and np.all(res["count"] == 8)
    assert np.all(both(same_pt, 8, 0.5, (2, 50, 0))["normals"] == (1, 0, 0))          # a dot product of 0 does not flip
    # n < 3: unit(viewpoint - p); the point at the viewpoint: (0, 0, 1); eigenvalues 0
    far = np.array([[0, 0, 0], [3, 4, 0], [3, 4, 0.125], [0, -8, 0], [50, 50, 50]], np.float32)
    res = both(far, 4, 0.25, (0, 0, 0))
    assert res["count"].tolist() == [1, 2, 2, 1, 1] and np.all(res["eigenvalues"] == 0)
    assert res["normals"][0].tolist() == [0, 0, 1] and res["normals"][3].tolist() == [0, 1, 0]
    assert np.array_equal(res["normals"][1], (np.array([-3, -4, 0], np.float64) / 5).astype(np.float32))
    want4 = (np.array([-50, -50, -50], np.float64) / np.sqrt(7500.0)).astype(np.float32)
    assert np.array_equal(res["normals"][4], want4)
    # ... which is the reference's default -unit(point) for a viewpoint at the origin
    assert np.allclose(res["normals"][1:], -far[1:] / np.linalg.norm(far[1:], axis=1, keepdims=True), atol=1e-7)
    # the boundary is inside: d2 == r2 counts
    pair = np.array([[0, 0, 0], [0.75, 0, 0], [0, 0.75, 0]], np.float32)
    assert both(pair, 3, 0.75, (0, 0, 9))["count"].tolist() == [3, 2, 2] and both(pair, 3, 0.7499, (0, 0, 9))["count"].tolist() == [1, 1, 1]
    assert both(pair, 3, 0.75, (0, 0, 9))["normals"][0].tolist() == [0, 0, 1]
    # three collinear points: two zero eigenvalues, still a unit vector, the same one on every run
    line = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6]], np.float32)
    a, b = both(line, 3, None, (5, 5, 5)), both(line, 3, None, (5, 5, 5))
    assert np.array_equal(a["normals"].view(np.uint32), b["normals"].view(np.uint32)) and np.all(a["count"] == 3)
    assert np.all(np.abs(np.linalg.norm(a["normals"].astype(np.float64), axis=1) - 1) < 1e-7)
    assert np.all(np.abs(a["normals"].astype(np.float64) @ np.array([1.0, 2.0, 3.0])) < 1e-6)     # orthogonal to the line
    assert np.all(np.abs(a["eigenvalues"][:, :2]) < 1e-6) and np.all(a["eigenvalues"][:, 2] > 1)


def sphere_cloud(M=4000, R=64.0, seed=5):
    """Points of the radius-R sphere snapped to the 1/16 lattice."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (M, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.unique((np.round(v * R * 16) / 16).astype(np.float32), axis=0)


def eigh_check(want, limit=1e-6, gap=1e-3):
    """|n x n_eigh| wherever (l1 - l0) >= gap * l2, and the share of points (n >= 3) the condition excludes."""
    use = want["count"] >= 3
    c = want["cov"][use]
    Cm = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)
    w, V = np.linalg.eigh(Cm)
    clear = (w[:, 1] - w[:, 0]) >= gap * w[:, 2]
    cross = np.linalg.norm(np.cross(want["normals"][use].astype(np.float64), V[:, :, 0]), axis=1)
    eig_err = np.abs(want["eigenvalues"][use].astype(np.float64) - w).max(1) / np.maximum(w[:, 2], 1e-300)
    return cross[clear].max(), 1.0 - clear.mean(), eig_err.max()


def test_jacobi_against_lapack():
    """The restatement's normals against np.linalg.eigh of the same float64 covariance: |n x n_eigh| <= 1e-6 wherever
    (l1 - l0) >= 1e-3 * l2 — the float32 rounding of the output is 6e-8 per component and an eigenvector's error is of
    order eps64 / relative gap, so 1e-6 is the rounding with a margin of ten — and no more than 5 % of the points excluded."""
    pts = sphere_cloud()
    for k, radius in ((20, None), (50, None), (30, 8.0)):
        want = ref.normals(pts, k, radius, (0, 0, 0))
        worst, excluded, eig_err = eigh_check(want)
        print(f"sphere M={len(pts)} k={k} radius={radius}: max |n x n_eigh| {worst:.3g}, excluded {excluded:.4f}, "
              f"eigenvalue error / l2 {eig_err:.3g}")
        assert excluded <= 0.05 and worst <= 1e-6 and eig_err <= 1e-6
    pts = outlier_ref.filter_cloud(3000, 3)
    want = ref.normals(pts, 20, None, (0, 0, 40))
    worst, excluded, eig_err = eigh_check(want)
    print(f"slab: max |n x n_eigh| {worst:.3g}, excluded {excluded:.4f}, eigenvalue error / l2 {eig_err:.3g}")
    assert worst <= 1e-6 and eig_err <= 1e-6


def test_the_sweeps_are_enough():
    """Two more sweeps than SLS_NORMALS_SWEEPS change no bit, and the solve meets eigh: random positive semi-definite
    matrices over twelve decades of conditioning, a tenth of them with three nearly equal eigenvalues."""
    rng = np.random.default_rng(8)
    A = rng.normal(0, 1, (20000, 3, 3))
    scale = 10.0 ** rng.uniform(-6, 0, (20000, 1, 3))
    A = np.einsum("mij,mkj->mik", A * scale, A * scale)
    A[:2000] += np.eye(3)[None] * 1e3
    cov = np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], 1)
    d, V = ref.jacobi(cov)
    d2, V2 = ref.jacobi(cov, ref.SWEEPS + 2)
    assert np.array_equal(d.view(np.uint64), d2.view(np.uint64)) and np.array_equal(V.view(np.uint64), V2.view(np.uint64))
    w = np.linalg.eigvalsh(A)
    assert np.all(np.abs(np.sort(d, 1) - w) <= 1e-13 * w[:, 2:3])
    R = np.einsum("mij,mjk->mik", A, V) - V * d[:, None, :]            # A V - V D
    assert np.all(np.abs(R).max(axis=(1, 2)) <= 1e-13 * w[:, 2])
    assert np.abs(np.einsum("mji,mjk->mik", V, V) - np.eye(3)).max() <= 1e-14
