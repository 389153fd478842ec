"""The references of the size tests (tests/scale_ref.py) on the host, no device needed: each fast reference against the plain
one it replaces (lexsort weld against np.unique, block-diagonal k-NN against the brute force and, where SciPy imports,
against a KD-tree at full size, the tetrahedra's closed form against the breadth-first walk, the tiled fan against the header
run on the whole mesh), the preconditions the device tests rest on (cluster separation, the statistical rule's margin), and
the constants of scale_ref against the sources as text: whoever retunes one is told which size test has lost its path."""
import math
import os
import time

import numpy as np
import pytest

import fill_ref
import mesh_ref
import nn_ref
import outlier_ref
import scale_ref as S
import smooth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1                        # the seed of the large clouds, here and in test_scale_paths.py


def fsum_mean(mean):
    """cloud_mean of outlier_ref.statistical with an exactly rounded sum"""
    return math.fsum(mean[mean > 0].tolist()) / len(mean)


def timed(what, fn):
    t = time.perf_counter()
    out = fn()
    print(f"{what}: {time.perf_counter() - t:.2f} s")
    return out


def test_constants_are_the_sources():
    """A plain text match, as test_nn_host.py matches SLS_NN_STATS_SCRATCH_BYTES.  (The 256 threads of the sorter's row scan
    and of the reductions and the 64 boxes of a sweep chunk are literals in the sources: their lines are matched whole.)"""
    text = {}
    for path, line, covers in S.SOURCES:
        if path not in text:
            text[path] = open(os.path.join(ROOT, path)).read()
        assert line in text[path], f"{path} no longer holds `{line}`: tests/scale_ref.py and the sizes of {covers} need another look"
    # the figures scale_ref derives from those lines
    assert S.SORT_WAVE_ITEMS == 64 * 16 and S.ROWSCAN_THREADS == 256 and S.ROWSCAN_KEEP == 8
    assert S.CLOUD_CHUNK == S.CLOUD_THREADS * 4 == 1024 and S.MESH_CHUNK == S.MESH_THREADS * 4 == 2048
    assert S.KNN_BOX == 256 and S.SWEEP_BOXES == 64 and S.REDUCE_MAX_BLOCKS == 32768 // 32 == 1024
    assert S.LONG_MAX_BLOCKS == 2048 and S.LONG_WAVES == 256 // 64 and S.LONG_ROW == 64


def test_threshold_arithmetic():
    """the sizes the issue names, through the helpers the device tests assert with"""
    assert [S.rowscan_p(n) for n in (262143, 262144, 262145, 2097152, 2097153, 2098177)] == [1, 1, 2, 8, 9, 9]
    assert S.rowscan_p(27 * 80022) == 9 and S.scan_p(27 * 80022, S.MESH_THREADS, S.MESH_CHUNK) == 3
    assert [S.scan_p(n, S.CLOUD_THREADS, S.CLOUD_CHUNK) for n in (262144, 262145)] == [1, 2]
    assert [S.scan_p(n, S.MESH_THREADS, S.MESH_CHUNK) for n in (1048576, 1048577)] == [1, 2]
    assert [S.sweep_chunks(n) for n in (5000, 16384, 16385, 50000)] == [1, 1, 2, 4]
    assert [S.reduce_blocks(n) for n in (65536, 65537, 70200, 262144, 280800)] == [256, 257, 275, 1024, 1024]
    V, T = 66 * S.FAN_COPIES, 65 * S.FAN_COPIES
    assert S.smooth_long_waves(V, T) == 8192 < S.FAN_COPIES and S.fill_long_waves(T) == 8192 < S.FAN_COPIES
    assert S.smooth_long_waves(66 * 100, 65 * 100) == 604 and S.fill_long_waves(65 * 100) == 104


@pytest.mark.parametrize("n", [0, 1, 2, 4097, 6000, 2098177])
def test_weld_lexsort_is_np_unique(n):
    rows = mesh_ref.sized_rows(n) if n else np.zeros((0, 3), np.float32)
    got_v, got_i = timed(f"weld_lexsort, {n} rows", lambda: S.weld_lexsort(rows))
    want_v, want_i = timed(f"mesh_ref.weld, {n} rows", lambda: mesh_ref.weld(rows))
    assert np.array_equal(mesh_ref.bits(got_v), mesh_ref.bits(want_v)) and np.array_equal(got_i, want_i)
    if n == 6000:                                                   # signed words, -0.0 apart from 0.0, NaN payloads
        for case, r in mesh_ref.weld_cases().items():
            gv, gi = S.weld_lexsort(r)
            wv, wi = mesh_ref.weld(r)
            assert np.array_equal(mesh_ref.bits(gv), mesh_ref.bits(wv)) and np.array_equal(gi, wi), case


def test_blockdiag_is_the_brute_force():
    pts, label = S.clustered_cloud(6, SEED)
    assert pts.shape == (3000, 3) and np.bincount(label).tolist() == [500] * 6
    want = outlier_ref.keys_k(pts, pts, 32)
    assert np.array_equal(S.keys_k_blockdiag(pts, label, 32), want)
    rng = np.random.default_rng(3)                                  # a second cloud: queries of three of the six parts only
    rows = np.flatnonzero(label % 2 == 0)[:700]
    query = pts[rows] + (rng.integers(-3, 4, (700, 3)) / 16.0).astype(np.float32)
    got = S.keys_k_blockdiag(pts, label, 5, query, label[rows])
    assert np.array_equal(got, outlier_ref.keys_k(pts, query, 5))
    # the filters' tails from the keys
    w, g = outlier_ref.statistical(pts, 20, 2.0), S.statistical_from_keys(want, 20, 2.0)
    assert all(np.array_equal(w[k], g[k]) for k in w)
    for nb, r in ((3, 0.25), (19, 0.75), (31, 1.5)):
        assert np.array_equal(S.radius_from_keys(want, nb, r), outlier_ref.radius(pts, nb, r))
    est, est_label = S.estimate_cloud(6, SEED)
    kw = dict(threshold=0.09375, truncation_acc=0.15625, truncation_com=0.1875)
    d_acc = outlier_ref.split(S.keys_k_blockdiag(pts, label, 1, est, est_label))[0][:, 0]
    d_com = outlier_ref.split(S.keys_k_blockdiag(est, est_label, 1, pts, label))[0][:, 0]
    assert S.metrics_from_dist2(d_acc, d_com, **kw) == nn_ref.cloud_metrics(pts, est, **kw)


def test_large_clouds_preconditions():
    """The separation asserted inside clustered_cloud / filter_keys, the sizes, and the statistical rule's margin: no mean
    within 1e-6 of the threshold, so the device's mask must equal the reference's (asserted again on the device)."""
    for n_clusters in (135, 540):
        pts, label, nrm = S.filter_cloud(n_clusters, SEED)
        keys = timed(f"filter_keys, {len(pts)} points", lambda: S.filter_keys(n_clusters, SEED))
        M = len(pts)
        assert M == n_clusters * 500 + n_clusters * 20 and nrm.shape == pts.shape and np.abs(pts).max() <= 64.0
        want = S.statistical_from_keys(keys, 20, 2.0)
        print(f"M={M}: margin {want['margin']:.3g}, kept {want['keep'].sum()}, cloud_mean {want['cloud_mean']!r}, std {want['std']!r}, "
              f"threshold {want['thr']!r}; bounds {S.sum_bound(M):.3g} {S.std_bound(M, want['cloud_mean'], want['std']):.3g} "
              f"{S.thr_bound(M, want['cloud_mean'], want['std']):.3g}")
        assert want["margin"] > 1e-6 and 0 < want["keep"].sum() < M
        assert abs(fsum_mean(want["mean"]) - want["cloud_mean"]) <= S.sum_bound(M) * want["cloud_mean"]
        d2, idx = outlier_ref.split(keys)
        assert (d2[:, 0] == 0).all() and (label[idx] == label[:, None]).all()     # itself (or a copy) first; neighbours of its own part
    assert S.reduce_blocks(70200) > 256 and 270000 > S.CLOUD_THREADS * S.CLOUD_CHUNK


def test_blockdiag_agrees_with_kdtree_at_full_size():
    spatial = pytest.importorskip("scipy.spatial")
    pts, label = S.clustered_cloud(540, SEED)
    keys = timed("keys_k_blockdiag, 270000 points, k = 32", lambda: S.keys_k_blockdiag(pts, label, 32))
    d2, idx = outlier_ref.split(keys)
    p64 = pts.astype(np.float64)
    dist, kidx = timed("cKDTree, k = 32", lambda: spatial.cKDTree(p64).query(p64, k=32))
    assert np.allclose(np.sqrt(d2.astype(np.float64)), dist, rtol=1e-12, atol=0)
    clear = (np.diff(dist, axis=1) > 0).all(1)                      # the index lists agree wherever no two distances tie
    assert clear.mean() > 0.1 and np.array_equal(idx[clear, :31], kidx[clear, :31])      # (the 32nd may tie with the 33rd)
    assert (label[idx] == label[:, None]).all()


def test_tetrahedra_closed_form_is_the_walk():
    n = 1000
    v, f = S.tetrahedra(n)
    want = timed(f"mesh_ref.clusters, {n} tetrahedra", lambda: mesh_ref.clusters(f, len(v)))
    labels, counts, stats = S.tetrahedra_clusters(n)
    assert np.array_equal(labels, want[0]) and np.array_equal(counts, want[1]) and stats == want[2]
    host = mesh_ref.host().clusters(f, len(v))
    assert np.array_equal(labels, host[0]) and np.array_equal(counts, host[1]) and stats == host[2]
    assert len(np.unique(v, axis=0)) == len(v)                      # the copies do not touch: a weld would leave them apart


def test_fans_header_references_are_tiled_single_fans():
    """The size tests run the headers on the whole mesh of 8200 fans (timed here).  The whole-mesh results must be the
    single fan's, tiled: every row's arithmetic is order-fixed and position-independent — which also checks the headers'
    own large-size paths (their sorts) against their small ones."""
    v, f = S.fans()
    v1, f1 = smooth_ref.fan(S.FAN_N)
    V1, T1, n = len(v1), len(f1), S.FAN_COPIES
    assert (len(v), len(f)) == (541200, 533000) == (V1 * n, T1 * n)
    for method, weights in ((smooth_ref.LAPLACIAN, smooth_ref.UNIFORM), (smooth_ref.TAUBIN, smooth_ref.INVERSE_DISTANCE)):
        got, status = timed("smooth_ref.host().smooth, 8200 fans", lambda: smooth_ref.host().smooth(v, f, 1, method, weights))
        one, status1 = smooth_ref.host().smooth(v1, f1, 1, method, weights)
        assert np.array_equal(mesh_ref.bits(got), mesh_ref.bits(np.tile(one, (n, 1))))
        assert status[smooth_ref.STATUS.index("max_row")] == S.FAN_N == status1[smooth_ref.STATUS.index("max_row")]
    room = fill_ref.room(len(v), len(f), 1.0)
    out_v, out_f, status = timed("fill_ref.host().fill, 8200 fans", lambda: fill_ref.host().fill(v, f, 128, 0.0, *room))
    one_v, one_f, status1 = fill_ref.host().fill(v1, f1, 128, 0.0, *fill_ref.room(V1, T1, 1.0))
    assert status1[:5] == [V1 + 1, 2 * T1, T1, 1, 1] and status[:5] == [(V1 + 1) * n, 2 * T1 * n, T1 * n, n, n]
    assert np.array_equal(mesh_ref.bits(out_v[:len(v)]), mesh_ref.bits(v)) and np.array_equal(out_f[:len(f)], f)
    assert np.array_equal(mesh_ref.bits(out_v[len(v):]), mesh_ref.bits(np.tile(one_v[V1:], (n, 1))))       # a centroid per loop, in loop order
    new = out_f[len(f):2 * len(f)].reshape(n, T1, 3)
    one_new = one_f[T1:2 * T1]
    rim = np.where(one_new == V1, -1, one_new)                       # the single fan's cap: its centroid's index set apart
    for k in (0, 1, n - 1):
        want = np.where(rim < 0, len(v) + k, rim + k * V1)
        assert np.array_equal(new[k], want)
