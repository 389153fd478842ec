"""sls_nn_query / sls_nn_stats / splat_loam_amd.evaluation on the device against the NumPy restatement (nn_ref.py).

Lattice inputs (multiples of 1/16, magnitude <= 64) make the kernel's float32 expression exact, so there the
restatement's float64 values are its bits and everything is compared with array_equal."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nn_ref
from splat_loam_amd import _abi, evaluation, ply_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lattice(rng, n, half=64.0, step=16):
    return (rng.integers(-int(half * step), int(half * step) + 1, (n, 3)) / float(step)).astype(np.float32)


def run(device, target, query, return_index=True):
    d2, idx = evaluation.nearest(torch.tensor(target, device=device), torch.tensor(query, device=device), return_index)
    return d2.cpu().numpy(), (idx.cpu().numpy() if idx is not None else None)


def assert_bitwise(device, target, query, what):
    d2, idx = run(device, target, query)
    r2, ridx = nn_ref.nearest(target, query)
    r2 = r2.astype(np.float32)
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == idx.shape == (len(query),)
    bad = np.flatnonzero((d2.view(np.uint32) != r2.view(np.uint32)) | (idx != ridx))
    assert bad.size == 0, f"{what}: {bad.size} of {len(query)} differ, first {bad[:5]}: got {d2[bad[:5]]} {idx[bad[:5]]}, " \
                          f"want {r2[bad[:5]]} {ridx[bad[:5]]}"


# the granularities of 32-point runs, 64-lane waves, 256-point boxes and 64-box chunks
@pytest.mark.parametrize("Mt,Mq", [(1, 1), (1, 65), (2, 64), (31, 3), (32, 64), (33, 65), (63, 1), (64, 64), (65, 63),
                                   (255, 100), (256, 256), (257, 129), (513, 1000), (6000, 4000)])
def test_lattice_bit_for_bit(device, Mt, Mq):
    rng = np.random.default_rng(1000 * Mt + Mq)
    assert_bitwise(device, lattice(rng, Mt), lattice(rng, Mq), f"Mt={Mt} Mq={Mq}")


def test_ties_lowest_index(device):
    """Integer targets, half-integer queries: nearly every minimum is attained by several targets, often in different
    boxes — the lowest index must win, so no box whose gap EQUALS the bound may be pruned."""
    rng = np.random.default_rng(5)
    target = rng.integers(-8, 9, (4000, 3)).astype(np.float32)
    query = (rng.integers(-8, 8, (300, 3)) + 0.5).astype(np.float32)
    d = nn_ref.dist2_matrix(query, target)
    tied = ((d == d.min(1, keepdims=True)).sum(1) > 1).mean()
    print(f"queries with a tied minimum: {tied:.3f}")
    assert tied > 0.9
    assert_bitwise(device, target, query, "ties")


def lidar_cloud():
    """The cloud of test_knn_bitexact: two walls, a 2 cm cluster, 40 far returns and 300 copies of one point."""
    rng = np.random.default_rng(21)
    wall1 = np.stack([rng.uniform(-20, 20, 6000), np.full(6000, 8.0), rng.uniform(-2, 3, 6000)], 1)
    wall2 = np.stack([np.full(4000, -15.0), rng.uniform(-30, 30, 4000), rng.uniform(-2, 6, 4000)], 1)
    cluster = rng.normal(0, 0.02, (3000, 3)) + np.array([3.0, -2.0, 0.5])
    far = rng.uniform(-150, 150, (40, 3))
    same = np.tile(np.array([[1.25, 2.5, -0.75]]), (300, 1))
    pts = np.concatenate([wall1, wall2, cluster, far, same]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def test_lidar_like_cloud(device):
    target = lidar_cloud()
    assert len(target) == 13340
    rng = np.random.default_rng(22)
    query = np.concatenate([
        target[rng.integers(0, len(target), 5000)] + rng.normal(0, 0.05, (5000, 3)),
        rng.uniform(-400, 400, (2000, 3)),                          # most lie outside the target's cube
        target[rng.integers(0, len(target), 200)],                  # exact copies of targets
        np.tile(np.array([[1.25, 2.5, -0.75]]), (64, 1)),           # the duplicated point
    ]).astype(np.float32)
    assert len(query) == 7264
    d2, idx = run(device, target, query)
    assert idx.min() >= 0 and idx.max() < len(target)
    n_dup_ties = n_excused = 0
    step = 256
    for a in range(0, len(query), step):
        D = nn_ref.dist2_matrix(query[a:a + step], target)
        rows = np.arange(D.shape[0])
        m = D.min(1)
        got, gi = d2[a:a + step].astype(np.float64), idx[a:a + step]
        at = D[rows, gi]
        assert np.all(at <= (1 + 1e-6) * m), "not a nearest target"
        assert np.all(np.abs(got - at) <= 2.0 ** -21 * at), "dist2 off by more than four ulp"
        assert np.all(got[m == 0] == 0), "a query that equals a target must get exactly 0"
        band = D <= ((1 + 1e-6) * m)[:, None]
        first = band.argmax(1)                                      # lowest index inside the band
        identical = band.sum(1) == 1                                # every target of the band is the same point ...
        multi = np.flatnonzero(~identical)                          # ... decided row by row where the band holds several
        same = (target[None, :, :] == target[first[multi]][:, None, :]).all(-1)
        identical[multi] = (~band[multi] | same).all(1)
        assert np.array_equal(gi[identical], first[identical]), "lowest index among coordinate-identical targets"
        n_dup_ties += int((identical & (band.sum(1) > 1)).sum())
        n_excused += int((~identical).sum())
    print(f"duplicate ties {n_dup_ties}, excused {n_excused} of {len(query)}")
    assert n_dup_ties >= 64                                         # at least the 64 copies of the duplicated point
    assert n_excused <= 0.001 * len(query)


def test_degenerate_and_structural_cases(device):
    rng = np.random.default_rng(9)
    # all targets identical: a cube of extent 0
    target = np.tile(np.array([[2.5, -1.0, 0.25]], np.float32), (700, 1))
    query = np.concatenate([lattice(rng, 200, half=8.0), target[:3]])
    assert_bitwise(device, target, query, "identical targets")
    d2, idx = run(device, target, query)
    assert np.all(idx == 0) and np.all(d2[-3:] == 0)
    # collinear targets
    target = np.zeros((1000, 3), np.float32)
    target[:, 0] = rng.integers(-1024, 1025, 1000) / 16.0
    assert_bitwise(device, target, lattice(rng, 300, half=64.0), "collinear")
    # queries = the target set, with duplicates: every dist2 is 0 and the index the lowest duplicate
    target = lattice(rng, 1500, half=4.0, step=2)                   # 17^3 cells: many repeated rows
    d2, idx = run(device, target, target)
    _, ridx = nn_ref.nearest(target, target)
    assert np.all(d2 == 0) and np.array_equal(idx, ridx) and (ridx != np.arange(1500)).any()
    # shuffling the queries permutes the outputs; index=None gives the same dist2
    target, query = lattice(rng, 3000), lattice(rng, 2000)
    d2, idx = run(device, target, query)
    perm = rng.permutation(len(query))
    d2p, idxp = run(device, target, query[perm])
    assert np.array_equal(d2p.view(np.uint32), d2[perm].view(np.uint32)) and np.array_equal(idxp, idx[perm])
    d2n, none = run(device, target, query, return_index=False)
    assert none is None and np.array_equal(d2n.view(np.uint32), d2.view(np.uint32))
    # no query: empty tensors; no target: an error
    t = torch.tensor(target, device=device)
    e2, ei = evaluation.nearest(t, torch.zeros((0, 3), device=device))
    assert e2.shape == (0,) and e2.dtype == torch.float32 and ei.shape == (0,) and ei.dtype == torch.int32
    with pytest.raises(ValueError, match="empty"):
        evaluation.nearest(torch.zeros((0, 3), device=device), t)
    with pytest.raises(ValueError):
        evaluation.nearest(t, torch.zeros((5, 2), device=device))


def test_wide_key_path(device):
    """More than 200 000 targets: the codes are sorted on all 30 bits (three radix passes)."""
    rng = np.random.default_rng(14)
    assert_bitwise(device, lattice(rng, 200001), lattice(rng, 1024), "Mt=200001")


def nn_stats(device, d2, truncation, threshold, include_truncated):
    lib = _abi.lib()
    t = torch.tensor(d2, dtype=torch.float32, device=device)
    nbytes = 32768
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    out = torch.full((4,), -1, dtype=torch.int64, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    _abi.check(lib.sls_nn_stats(len(d2), t.data_ptr() if len(d2) else None, truncation, threshold, include_truncated,
                                out.data_ptr(), (scratch.data_ptr() + 255) & ~255, nbytes, st), "sls_nn_stats")
    w = out.cpu().numpy()
    return int(w[0]), int(w[1]), w[2:3].view(np.float64)[0], int(w[3]), w[2]


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 1000, 100003])
def test_nn_stats(device, M):
    rng = np.random.default_rng(M)
    trunc, thr = np.float32(0.5), np.float32(0.2)
    d2 = (rng.uniform(0, 0.6, M).astype(np.float32)) ** 2
    special = np.array([trunc * trunc, thr * thr, 0.0, np.inf, np.nextafter(trunc * trunc, np.float32(0)),
                        np.nextafter(thr * thr, np.float32(1)), 0.0], np.float32)
    k = min(M, len(special))
    d2[rng.permutation(M)[:k]] = special[:k] if M >= len(special) else special[rng.permutation(len(special))[:k]]
    for inc in (0, 1):
        n, below, s, m, bits = nn_stats(device, d2, float(trunc), float(thr), inc)
        rn, rbelow, rs, rm = nn_ref.stats(d2, trunc, thr, bool(inc))
        print(f"M={M} include_truncated={inc}: n {n} below {below} sum {s!r} (NumPy {rs!r})")
        assert (n, below, m) == (rn, rbelow, rm) and m == M
        assert abs(s - rs) <= 1e-12 * abs(rs)
        assert nn_stats(device, d2, float(trunc), float(thr), inc)[4] == bits      # the same bits on a second run


@pytest.mark.parametrize("M", nn_ref.STATS_ORDER_SIZES)
def test_nn_stats_sum_is_the_documented_order(device, M):
    """Word 2 bit for bit: the float64 sum is taken in the order nn_ref.device_sum restates, on terms spread over
    eighteen decades, seeded so that other orders give other bits (tests/test_nn_host.py shows that on this very data).  280 800 entries:
    1024 blocks whose first 18 656 threads take a second entry, and a final block whose threads read four partials each."""
    d2 = nn_ref.stats_order_dist2(M)
    for inc in (0, 1):
        n, below, s, m, bits = nn_stats(device, d2, 0.5, 0.2, inc)
        rn, rbelow, rs, rm = nn_ref.stats_device_order(d2, 0.5, 0.2, bool(inc))
        print(f"M={M} include_truncated={inc}: n {n} sum {s!r} (restated {rs!r}, NumPy's order {nn_ref.stats(d2, 0.5, 0.2, bool(inc))[2]!r})")
        assert (n, below, m) == (rn, rbelow, rm) and 0 < n <= M
        assert int(bits) == int(np.array([rs], np.float64).view(np.int64)[0])


@functools.lru_cache(maxsize=None)
def two_clouds():
    """Two lattice clouds of one surface region, each with points beyond both truncations."""
    rng = np.random.default_rng(31)
    reference = np.concatenate([lattice(rng, 2800, half=1.0), lattice(rng, 200, half=1.0) + np.float32(20.0)])
    estimate = np.concatenate([lattice(rng, 2300, half=1.0), lattice(rng, 200, half=1.0) - np.float32(30.0)])
    return reference[rng.permutation(3000)], estimate[rng.permutation(2500)]


SETTINGS = dict(threshold=0.09375, truncation_acc=0.15625, truncation_com=0.1875)


def check_metrics(got, want):
    assert set(got) == set(want)
    for k in ("n_accuracy", "n_completeness", "precision", "recall", "threshold", "truncation_acc", "truncation_com"):
        assert got[k] == want[k], k
    for k in ("accuracy_m", "completeness_m", "chamfer_l1_m", "fscore"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k


def test_cloud_metrics_and_crop(device):
    reference, estimate = two_clouds()
    r, e = torch.tensor(reference, device=device), torch.tensor(estimate, device=device)
    for kw in (SETTINGS, {}):
        want = nn_ref.cloud_metrics(reference, estimate, **kw)
        assert 0 < want["n_accuracy"] < 2500 and want["n_completeness"] == 3000 and 0 < want["recall"] < 1
        check_metrics(evaluation.cloud_metrics(r, e, **kw), want)
    for dist in (1.2, 0.25, 0.0625):
        mask = evaluation.crop_union_mask(r, e, dist)
        assert mask.dtype == torch.bool and mask.shape == (3000,)
        want = nn_ref.crop_union_mask(reference, estimate, dist)
        assert np.array_equal(mask.cpu().numpy(), want) and (dist > 1 or 0 < want.sum() < 3000)
    # an accuracy set that is empty: NaN, and an F-score of 0 where nothing is below the threshold
    far = evaluation.cloud_metrics(r, e + 500.0)
    assert np.isnan(far["accuracy_m"]) and np.isnan(far["precision"]) and far["n_accuracy"] == 0
    assert far["recall"] == 0.0 and far["completeness_m"] == 0.5
    none = evaluation.cloud_metrics(r, e, threshold=0.0)
    assert none["precision"] == 0.0 and none["recall"] == 0.0 and none["fscore"] == 0.0


def test_eval_cloud_tool(device, tmp_path):
    reference, estimate = two_clouds()
    ply_io.save_point_cloud(tmp_path / "reference.ply", reference, np.zeros_like(reference))
    ply_io.save_point_cloud(tmp_path / "estimate.ply", torch.tensor(estimate, device=device), torch.zeros((2500, 3)))
    assert np.array_equal(ply_io.load_point_cloud(tmp_path / "estimate.ply")[0], estimate)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_cloud.py"), str(tmp_path / "reference.ply"),
                          str(tmp_path / "estimate.ply"), "--threshold", "0.09375", "--truncation-acc", "0.15625",
                          "--truncation-com", "0.1875"], check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out.strip().splitlines()[-1])
    want = evaluation.cloud_metrics(torch.tensor(reference, device=device), torch.tensor(estimate, device=device), **SETTINGS)
    assert got == want                              # the same kernels on the same input: the same bits
    check_metrics(got, nn_ref.cloud_metrics(reference, estimate, **SETTINGS))
