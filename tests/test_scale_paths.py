"""The geometry ops past one workgroup of chunks, at the sizes of a saved map: the second level of the wave radix sort
(sort_rowscan_kernel with P >= 2 entries per thread, and its tail loop behind the 8 register-held entries from P = 9 on), of
the chunked scan (Chunks::scan_totals / scan_in_place with more chunk totals than threads), of the k-NN box search (the
outward sweep over several chunks of 64 boxes), of the capped reductions (threads striding, more than 256 partials) and of the
long-row / long-loop kernels (waves striding) — through the public ops, bit for bit against the references of
tests/scale_ref.py, as the small-size siblings of these tests compare.  The only tolerances are those of the float64 sums
(scale_ref.sum_bound / std_bound / thr_bound, derived there).

Every test asserts on its own size that the path is entered, with the constants of scale_ref (which tests/test_scale_host.py
matches against the sources); the sizes are the smallest that cross each threshold.  Every test prints the wall time of its
reference and of its device calls."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import cloud_ref
import fill_ref
import mesh_ref
import nn_ref
import outlier_ref
import scale_ref as S
import simplify_ref
import smooth_ref
import tsdf_ref
from mesh_ref import bits
from splat_loam_amd import _abi, evaluation, mesh_ops, tsdf
from test_cloud_ops import assert_voxels_bitwise
from test_fill import _check_fill, _fill
from test_mesh_ops import _clusters
from test_nn_query import nn_stats
from test_outlier import bits64, check_nearest_k, lattice
from test_scale_host import SEED, fsum_mean
from test_simplify import _call as _simplify
from test_smooth import _smooth

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


class Clock:
    """wall times of a test's reference and device parts, printed at the end"""

    def __init__(self, device):
        self.device, self.t = device, {"reference": 0.0, "device": 0.0}

    def ref(self, fn):
        t = time.perf_counter()
        out = fn()
        self.t["reference"] += time.perf_counter() - t
        return out

    def dev(self, fn):
        torch.cuda.synchronize(self.device)
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(self.device)
        self.t["device"] += time.perf_counter() - t
        return out

    def report(self, what):
        print(f"{what}: reference {self.t['reference']:.2f} s, device calls {self.t['device']:.3f} s")


# ---- 1. the u32 sort and the head scan through weld --------------------------------------------------------------------
WELD_SIZES = (262143, 262144, 262145, 1048577, 2098177)


@pytest.mark.parametrize("n", WELD_SIZES)
def test_weld_rowscan_and_head_scan(device, n):
    """mesh_ops.weld_rows sorts n rows by three 32-bit words (nine 11-bit passes) and ranks the heads with the 512 x 4 scan."""
    if n <= 262144:
        assert S.rowscan_p(n) == 1                                  # the last sizes of the first level
    if n == 262145:
        assert n > S.ROWSCAN_THREADS * S.SORT_WAVE_ITEMS and S.rowscan_p(n) == 2       # sort_rowscan: P >= 2
    if n == 1048577:
        assert n > S.MESH_THREADS * S.MESH_CHUNK and S.chunks(n, S.MESH_CHUNK) == 513  # weld_scan_kernel: 513 totals, 512 threads
    if n == 2098177:
        assert n > S.ROWSCAN_KEEP * S.ROWSCAN_THREADS * S.SORT_WAVE_ITEMS and S.rowscan_p(n) == 9     # sort_rowscan: the tail loop
        assert S.chunks(n, S.SORT_WAVE_ITEMS) == 2050
    clock = Clock(device)
    rows = mesh_ref.sized_rows(n)
    want_v, want_i = clock.ref(lambda: S.weld_lexsort(rows))
    d = _dev(rows, device)
    v, index = clock.dev(lambda: mesh_ops.weld_rows(d))
    assert v.dtype == torch.float32 and index.dtype == torch.int32 and index.shape == (n,)
    assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(index.cpu().numpy(), want_i)
    uniq, inverse = torch.unique(d.view(torch.int32), dim=0, return_inverse=True)       # the same order
    assert torch.equal(v.view(torch.int32), uniq) and torch.equal(index.long(), inverse)
    v2, index2 = clock.dev(lambda: mesh_ops.weld_rows(d))                               # the same bytes on every run
    assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(index2, index)
    clock.report(f"weld, {n} rows -> {len(want_v)} vertices")


# ---- 2. the u64 sort and the 256 x 4 scan through voxel down-sampling --------------------------------------------------
@pytest.mark.parametrize("M", [262145, 263169])
def test_voxel_a_voxel_per_point(device, M):
    """Lattice points over half = 64 at voxel size 0.3: nearly every point has a voxel of its own, so the head scan adds
    257 / 258 chunk totals with 256 threads and (at the larger size) ranks beyond 262144."""
    assert M > S.CLOUD_THREADS * S.CLOUD_CHUNK and S.scan_p(M, S.CLOUD_THREADS, S.CLOUD_CHUNK) == 2     # scan_totals: P >= 2
    assert S.rowscan_p(M) == 2                                                                        # the u64 sort: P >= 2
    points = lattice(np.random.default_rng(M), M, half=64.0)
    t = time.perf_counter()
    rows, counts = assert_voxels_bitwise(device, points, 0.3, f"M={M}")
    print(f"voxel, M={M}: {len(rows)} voxels, largest {counts.max()}; reference + device {time.perf_counter() - t:.2f} s")
    assert counts.sum() == M
    if M == 263169:
        assert len(rows) > S.CLOUD_THREADS * S.CLOUD_CHUNK          # ranks past the first 256 chunks' worth


def test_voxel_one_long_segment_at_scale(device):
    """One voxel of 200001 points (the long-segment path: 64 lanes) beside 70560 voxels of one point, at voxel size 1."""
    rng = np.random.default_rng(7)
    dense = rng.integers(0, 8, (200001, 3)) / 16.0                  # inside the cell [-0.5, 0.5) of the cloud's minimum, 0
    dense[:3] = 0.0
    g = np.stack(np.meshgrid(np.arange(42), np.arange(42), np.arange(40), indexing="ij"), -1).reshape(-1, 3) + 20.0
    points = np.concatenate([dense, g]).astype(np.float32)
    points = points[rng.permutation(len(points))]
    M = len(points)
    assert M == 270561 and M > S.CLOUD_THREADS * S.CLOUD_CHUNK and np.abs(points).max() <= 64.0
    t = time.perf_counter()
    rows, counts = assert_voxels_bitwise(device, points, 1.0, "one long segment")
    print(f"voxel, one long segment: reference + device {time.perf_counter() - t:.2f} s")
    assert counts[0] == 200001 and len(counts) == 70561 and (counts[1:] == 1).all()


# ---- 3. the u64 sort's tail loop through TSDF block allocation ---------------------------------------------------------
def test_tsdf_blocks_sort_tail(device):
    """80000 points (and 22 that name nothing) give 27 x 80022 = 2160594 candidate keys: the sorter's rows have 2110 entries,
    P = 9, and the head scan 1055 chunk totals with 512 threads.  (sls_tsdf_blocks gives a point that names nothing 27 keys
    of 0, so the sorter's count word equals its capacity here; the 22 rows check the two counters and that the zeros, which
    sort to the front, start no block.)"""
    rng = np.random.default_rng(80)
    pts = rng.normal(0, 4, (80000, 3)).astype(np.float32)
    bad = pts[:22].copy()
    bad[:10, 0], bad[10:15, 1], bad[15:20, 2] = np.nan, np.inf, -np.inf
    bad[20], bad[21] = (1.2e6, 0.0, 0.0), (0.0, -1.1e6, 5.0)
    pts = np.concatenate([pts, bad])[rng.permutation(80022)]
    M, n = len(pts), 27 * len(pts)
    assert n > S.ROWSCAN_KEEP * S.ROWSCAN_THREADS * S.SORT_WAVE_ITEMS and S.rowscan_p(n) >= 9     # sort_rowscan: the tail loop
    assert S.scan_p(n, S.MESH_THREADS, S.MESH_CHUNK) >= 2                                         # tsdf_scan_kernel: P >= 2
    clock = Clock(device)
    VS, TRUNC, ORIGIN = tsdf_ref.VS, tsdf_ref.TRUNC, tsdf_ref.ORIGIN
    want, n_nf, n_rng = clock.ref(lambda: tsdf_ref.host().blocks_of_points(pts, VS, TRUNC, ORIGIN))
    assert (n_nf, n_rng) == (20, 2) and len(want) > 10000
    d = _dev(pts, device)
    got, det = clock.dev(lambda: tsdf.allocate_blocks(d, VS, TRUNC, ORIGIN, details=True))
    assert (det["n_nonfinite"], det["n_out_of_range"]) == (20, 2)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    # the C entry: all four status words, and the rows beyond the blocks untouched
    lib = _abi.lib()
    cap = len(want) + 50
    out = torch.full((cap, 3), -7, dtype=torch.int32, device=device)
    status = torch.full((4,), -7, dtype=torch.int32, device=device)
    nbytes = int(lib.sls_tsdf_blocks_scratch_bytes(M))
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    clock.dev(lambda: _abi.check(lib.sls_tsdf_blocks(M, d.data_ptr(), VS, TRUNC, (C.c_double * 3)(*ORIGIN), cap, out.data_ptr(), status.data_ptr(),
                                                     (scratch.data_ptr() + 255) & ~255, nbytes, torch.cuda.current_stream(device).cuda_stream),
                                 "sls_tsdf_blocks"))
    assert status.cpu().tolist() == [len(want), 20, 2, 1]
    assert np.array_equal(out[:len(want)].cpu().numpy(), want) and bool((out[len(want):] == -7).all())      # the same bytes again
    clock.report(f"tsdf blocks, {M} points -> {len(want)} blocks")


# ---- 4. the k-NN sweep over several chunks of boxes --------------------------------------------------------------------
def test_nearest_k_sweep_uniform(device):
    """50000 targets are 196 boxes, 4 sweep chunks.  The target rows are sorted by x, so the input order is not the curve's;
    the queries — 1024 of the targets, 1024 lattice points over twice the cube, partly outside it — start in every chunk."""
    rng = np.random.default_rng(50)
    target = lattice(rng, 50000, half=64.0)
    target = target[np.lexsort((target[:, 2], target[:, 1], target[:, 0]))]
    Mt = len(target)
    assert Mt > S.SWEEP_BOXES * S.KNN_BOX and S.sweep_chunks(Mt) == 4       # nn_query_k_kernel: nchunks > 1
    query = np.concatenate([target[rng.integers(0, Mt, 1024)], lattice(rng, 1024, half=128.0)])
    assert (np.abs(query[1024:]).max(1) > 64.0).mean() > 0.5
    t = time.perf_counter()
    check_nearest_k(device, target, query, "uniform, 4 sweep chunks", ks=(1, 3, 20, 32))
    print(f"nearest_k, uniform: reference + device {time.perf_counter() - t:.2f} s")


@functools.lru_cache(maxsize=None)
def lidar_cloud_large():
    """The LiDAR-like cloud of test_outlier.py at 40000 points: a dense slab (a fifth of a unit thick) and isolated far points
    whose neighbours lie in boxes of distant chunks"""
    rng = np.random.default_rng(78)
    n, n_far = 40000, 600
    slab = rng.integers(-256, 257, (n - n_far, 3)) / 16.0
    slab[:, 2] = rng.integers(-2, 3, n - n_far) / 16.0
    far = rng.integers(-1024, 1025, (n_far, 3)) / 16.0
    pts = np.concatenate([slab, far]).astype(np.float32)
    pts = pts[rng.permutation(n)]
    pts.setflags(write=False)
    return pts


def test_nearest_k_sweep_lidar_like(device):
    target = lidar_cloud_large()
    assert len(target) > S.SWEEP_BOXES * S.KNN_BOX and S.sweep_chunks(len(target)) == 3
    rng = np.random.default_rng(79)
    rows = np.concatenate([rng.integers(0, len(target), 1748), np.flatnonzero(np.abs(target).max(1) > 16.0)[:300]])
    assert len(rows) == 2048
    t = time.perf_counter()
    check_nearest_k(device, target, target[rows], "lidar-like, 3 sweep chunks", ks=(1, 3, 20, 32))
    print(f"nearest_k, lidar-like: reference + device {time.perf_counter() - t:.2f} s")


@functools.lru_cache(maxsize=None)
def cluster_keys():
    pts, label = S.clustered_cloud(540, SEED)
    keys = S.keys_k_blockdiag(pts, label, 32)
    keys.setflags(write=False)
    return keys


def test_nearest_k_large_self_query(device):
    """270000 points queried by themselves: 1055 boxes, 17 sweep chunks, 4219 query waves; the reference is block-diagonal
    (scale_ref.clustered_cloud asserts the separation it rests on)."""
    pts, label = S.clustered_cloud(540, SEED)
    M = len(pts)
    assert M == 270000 and M > S.REDUCE_THREADS * S.REDUCE_MAX_BLOCKS and S.sweep_chunks(M) == 17
    clock = Clock(device)
    want2, wanti = outlier_ref.split(clock.ref(cluster_keys))
    t = torch.tensor(pts, device=device)
    for k in (1, 20, 32):
        d2, idx = clock.dev(lambda: evaluation.nearest_k(t, t, k))
        assert d2.shape == idx.shape == (M, k) and d2.dtype == torch.float32 and idx.dtype == torch.int32
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        bad = np.flatnonzero(((d2.view(np.uint32) != want2[:, :k].view(np.uint32)) | (idx != wanti[:, :k])).any(1))
        assert bad.size == 0, f"k={k}: {bad.size} of {M} rows differ, first {bad[:3]}: got {d2[bad[:3]]} {idx[bad[:3]]}, " \
                              f"want {want2[bad[:3], :k]} {wanti[bad[:3], :k]}"
    clock.report("nearest_k, 270000 points by themselves, k = 1, 20, 32")


# ---- 5. the outlier filters and the cloud statistics above the grid caps -----------------------------------------------
def _check_statistical(device, n_clusters):
    pts, label, nrm = S.filter_cloud(n_clusters, SEED)
    M, k = len(pts), 20
    clock = Clock(device)
    want = S.statistical_from_keys(clock.ref(lambda: S.filter_keys(n_clusters, SEED)), k, 2.0)
    assert want["margin"] > 1e-6                                    # no mean at the threshold: the masks must be equal
    assert 0 < want["keep"].sum() < M
    p, n = torch.tensor(pts, device=device), torch.tensor(nrm, device=device)
    out, out_n, index, det = clock.dev(lambda: evaluation.remove_statistical_outlier(p, k, 2.0, normals=n, return_index=True, details=True))
    keep = np.flatnonzero(want["keep"])
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), keep)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pts[keep].view(np.uint32))
    assert np.array_equal(out_n.cpu().numpy().view(np.uint32), nrm[keep].view(np.uint32))
    assert det["kept"] == len(keep) and det["removed"] == M - len(keep) and det["zero_mean"] == want["zero_mean"]
    exact_mean = fsum_mean(want["mean"])
    cm, sd = want["cloud_mean"], want["std"]
    bounds = {"cloud_mean": S.sum_bound(M), "std": S.std_bound(M, cm, sd), "threshold": S.thr_bound(M, cm, sd)}
    wants = {"cloud_mean": exact_mean, "std": sd, "threshold": want["thr"]}
    errs = {key: abs(det[key] - wants[key]) / abs(wants[key]) for key in bounds}
    print(f"M={M}: relative errors " + ", ".join(f"{key} {errs[key]:.3g} (bound {bounds[key]:.3g})" for key in bounds))
    for key in bounds:
        assert errs[key] <= bounds[key], (key, det[key], wants[key])
    out2, det2 = clock.dev(lambda: evaluation.remove_statistical_outlier(p, k, 2.0, details=True))         # a second run: the same bits
    assert torch.equal(out2, out) and all(bits64(det2[key]) == bits64(det[key]) for key in ("cloud_mean", "std", "threshold"))
    clock.report(f"remove_statistical_outlier, M={M}")
    return p, n, pts, nrm


def test_statistical_outlier_above_the_grid_cap(device):
    """280800 points: the two reductions run 1024 blocks whose threads stride (M > 262144), the final kernel adds 1024
    partials with 256 threads, the compaction scans 275 chunk totals with 256 threads.  cloud_mean is compared with the
    exactly rounded sum (math.fsum) of the reference's means within scale_ref.sum_bound, std and threshold with the
    reference's within std_bound / thr_bound (derived in scale_ref)."""
    M = len(S.filter_cloud(540, SEED)[0])
    assert M > S.REDUCE_THREADS * S.REDUCE_MAX_BLOCKS and S.reduce_blocks(M) == S.REDUCE_MAX_BLOCKS        # threads stride
    assert S.reduce_blocks(M) > S.REDUCE_THREADS                                                          # the final kernel strides
    assert S.scan_p(M, S.CLOUD_THREADS, S.CLOUD_CHUNK) == 2                                               # outlier_scan_kernel: P >= 2
    _check_statistical(device, 540)


def test_statistical_outlier_more_than_256_partials(device):
    """70200 points: 275 partials — the final kernel's threads take a second one — below the grid cap."""
    M = len(S.filter_cloud(135, SEED)[0])
    assert S.REDUCE_THREADS < S.reduce_blocks(M) < S.REDUCE_MAX_BLOCKS and M > 65536
    _check_statistical(device, 135)


def test_radius_outlier_above_the_grid_cap(device):
    pts, label, nrm = S.filter_cloud(540, SEED)
    M = len(pts)
    assert S.scan_p(M, S.CLOUD_THREADS, S.CLOUD_CHUNK) == 2                                               # outlier_scan_kernel: P >= 2
    clock = Clock(device)
    keys = clock.ref(lambda: S.filter_keys(540, SEED))
    p, n = torch.tensor(pts, device=device), torch.tensor(nrm, device=device)
    for nb, radius in ((3, 0.375), (9, 0.75)):
        want = S.radius_from_keys(keys, nb, radius)
        keep = np.flatnonzero(want)
        print(f"M={M} nb_points={nb} radius={radius}: kept {len(keep)}")
        assert 0 < len(keep) < M and 0 < want[label < 540].sum() < 270000          # the rule cuts through the clusters
        out, out_n, index, det = clock.dev(lambda: evaluation.remove_radius_outlier(p, nb, radius, normals=n, return_index=True, details=True))
        assert np.array_equal(index.cpu().numpy(), keep) and det == {"kept": len(keep), "removed": M - len(keep)}
        assert np.array_equal(out.cpu().numpy().view(np.uint32), pts[keep].view(np.uint32))
        assert np.array_equal(out_n.cpu().numpy().view(np.uint32), nrm[keep].view(np.uint32))
        assert torch.equal(clock.dev(lambda: evaluation.remove_radius_outlier(p, nb, radius)), out)
    clock.report(f"remove_radius_outlier, M={M}")


def test_nearest_and_metrics_above_the_grid_cap(device):
    """270000 distances through evaluation.nearest, sls_nn_stats and cloud_metrics: 1024 blocks whose threads stride, 1024
    partials for 256 threads.  n and n_below are equal; the sum within scale_ref.sum_bound of NumPy's."""
    ref_pts, ref_label = S.clustered_cloud(540, SEED)
    est_pts, est_label = S.estimate_cloud(540, SEED)
    M = len(ref_pts)
    assert M > S.REDUCE_THREADS * S.REDUCE_MAX_BLOCKS and S.reduce_blocks(M) == S.REDUCE_MAX_BLOCKS > S.REDUCE_THREADS
    clock = Clock(device)
    acc2, acci = outlier_ref.split(clock.ref(lambda: S.keys_k_blockdiag(ref_pts, ref_label, 1, est_pts, est_label)))
    com2, comi = outlier_ref.split(clock.ref(lambda: S.keys_k_blockdiag(est_pts, est_label, 1, ref_pts, ref_label)))
    r, e = torch.tensor(ref_pts, device=device), torch.tensor(est_pts, device=device)
    d2, idx = clock.dev(lambda: evaluation.nearest(r, e))
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(d2.view(np.uint32), acc2[:, 0].view(np.uint32)) and np.array_equal(idx, acci[:, 0])
    kw = dict(threshold=0.09375, truncation_acc=0.15625, truncation_com=0.1875)
    bound = S.sum_bound(M)
    for inc in (0, 1):
        n, below, s, m, word = clock.dev(lambda: nn_stats(device, d2, kw["truncation_acc"], kw["threshold"], inc))
        rn, rbelow, rs, rm = nn_ref.stats(d2, kw["truncation_acc"], kw["threshold"], bool(inc))
        print(f"M={M} include_truncated={inc}: n {n} below {below} sum {s!r} (NumPy {rs!r}), relative error {abs(s - rs) / rs:.3g} (bound {bound:.3g})")
        assert (n, below, m) == (rn, rbelow, rm) and m == M and 0 < below < n and (inc or n < M)
        assert abs(s - rs) <= bound * abs(rs)
        assert nn_stats(device, d2, kw["truncation_acc"], kw["threshold"], inc)[4] == word              # the same bits on a second run
    want = S.metrics_from_dist2(acc2[:, 0], com2[:, 0], **kw)
    got = clock.dev(lambda: evaluation.cloud_metrics(r, e, **kw))
    assert set(got) == set(want) and 0 < want["n_accuracy"] < M and want["n_completeness"] == M
    for key in ("n_accuracy", "n_completeness", "precision", "recall", "threshold", "truncation_acc", "truncation_com"):
        assert got[key] == want[key], key
    for key in ("accuracy_m", "completeness_m", "chamfer_l1_m", "fscore"):                               # (a quotient or a mean of the sums)
        assert abs(got[key] - want[key]) <= (bound + 4 * S.U) * abs(want[key]), key
    clock.report(f"nearest / nn_stats / cloud_metrics, M={M}")


# ---- 6. the strided long-row and long-loop kernels ---------------------------------------------------------------------
def test_fans_smooth_long_rows_stride(device):
    """8200 hubs of 65 neighbours.  sls_mesh_smooth sizes the long-row grid by long_cap = min(6 T / 65 + 1, V) = 49201, not by
    the live count: 2048 blocks, 8192 waves, so the waves' stride loop takes a second trip from 8193 long rows on.  The
    reference is the header run on the whole mesh (0.3 - 0.5 s on the host; tests/test_scale_host.py shows it equal to the
    single fan's result, tiled)."""
    v, f = S.fans()
    V, T = len(v), len(f)
    assert S.smooth_long_waves(V, T) == S.LONG_MAX_BLOCKS * S.LONG_WAVES == 8192 and S.FAN_COPIES > 8192      # a second trip
    assert 6 * T > S.MESH_THREADS * S.MESH_CHUNK                                                              # adjacency scan: P >= 2
    clock = Clock(device)
    dv, df = _dev(v, device).contiguous(), _dev(f, device).contiguous()
    for method in (smooth_ref.LAPLACIAN, smooth_ref.TAUBIN):
        for weights in (smooth_ref.UNIFORM, smooth_ref.INVERSE_DISTANCE):
            want_v, want_s = clock.ref(lambda: smooth_ref.host().smooth(v, f, 1, method, weights))
            assert want_s[smooth_ref.STATUS.index("max_row")] == S.FAN_N
            got_v, status = clock.dev(lambda: _smooth(device, dv, df, V, T, method, weights, False, 1))
            assert status == want_s + [9, 9], (method, weights)
            assert np.array_equal(bits(got_v), bits(want_v)), (method, weights)
    clock.report(f"smooth, {S.FAN_COPIES} fans")


def test_fans_fill_long_loops_stride(device):
    """8200 boundary loops of 65 half-edges at max_edges = 128.  sls_mesh_fill_holes launches min((T / 65 + 4) / 4, 2048)
    blocks of four waves for the long loops: 8192 waves here, striding over all loops, so a second trip from 8193 loops on.
    The reference is the header run on the whole mesh (0.6 s on the host)."""
    v, f = S.fans()
    V, T = len(v), len(f)
    assert S.fill_long_waves(T) == S.LONG_MAX_BLOCKS * S.LONG_WAVES == 8192 and S.FAN_COPIES > 8192           # a second trip
    assert 3 * T > S.MESH_THREADS * S.MESH_CHUNK                                                              # the fill scans: P >= 2
    clock = Clock(device)
    cap_v, cap_t = fill_ref.room(V, T, 1.0)
    want = clock.ref(lambda: fill_ref.host().fill(v, f, 128, 0.0, cap_v, cap_t))
    assert want[2][:5] == [V + S.FAN_COPIES, 2 * T, S.FAN_N * S.FAN_COPIES, S.FAN_COPIES, S.FAN_COPIES] and want[2][14] == 0
    dv, df = _dev(v, device).contiguous(), _dev(f, device).contiguous()
    got = clock.dev(lambda: _fill(device, dv, df, None, V, T, 128, 0.0, cap_v, cap_t))
    _check_fill(got, want, cap_v)                                   # vertices, faces, the -1 padding and all status words
    clock.report(f"fill, {S.FAN_COPIES} loops")


# ---- 7. the mesh scans above 512 chunks --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [90000, 262145])
def test_tetrahedra_clusters(device, n):
    """n closed tetrahedra, labels t // 4 in closed form.  90000: 3 T = 1080000 edge keys, the u64 sort's rows have 1055
    entries (P = 5).  262145: T = 1048580 triangles, mesh_rootscan_kernel adds 513 chunk totals with 512 threads."""
    v, f = S.tetrahedra(n)
    T = len(f)
    if n == 90000:
        assert 3 * T > S.MESH_THREADS * S.MESH_CHUNK and S.rowscan_p(3 * T) == 5
    else:
        assert T > S.MESH_THREADS * S.MESH_CHUNK and S.scan_p(T, S.MESH_THREADS, S.MESH_CHUNK) == 2
    want_l, want_c, s = S.tetrahedra_clusters(n)
    clock = Clock(device)
    for run in range(2):
        labels, counts, w = clock.dev(lambda: _clusters(device, f, len(v)))
        assert list(w[:6]) == [n, 0, 0, 0, 0, 1] and list(w[6:]) == [9, 9]
        assert np.array_equal(labels, want_l) and np.array_equal(counts, want_c)
    clock.report(f"clusters, {n} tetrahedra")


def test_tetrahedra_vertex_normals(device):
    """3 T = 1080000 corners: the corner sort at P = 5 and the 512 x 4 scan over 528 chunks, against the header on the host"""
    v, f = S.tetrahedra(90000)
    assert 3 * len(f) > S.MESH_THREADS * S.MESH_CHUNK and S.scan_p(3 * len(f), S.MESH_THREADS, S.MESH_CHUNK) == 2
    clock = Clock(device)
    want = clock.ref(lambda: mesh_ref.host().normals(v, f))
    dv, df = _dev(v, device), _dev(f, device)
    got = clock.dev(lambda: mesh_ops.vertex_normals(dv, df)).cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and len(np.unique(bits(want), axis=0)) == 4
    assert np.array_equal(bits(clock.dev(lambda: mesh_ops.vertex_normals(dv, df)).cpu().numpy()), bits(got))
    clock.report("vertex normals, 90000 tetrahedra")


def test_mesh_sample_weight_scan_above_256_chunks(device):
    """evaluation.sample_mesh scans the faces' 64-bit weights with the 256 x 4 scan (the only 64-bit instance of
    scan_totals): 360000 faces are 352 chunk totals for 256 threads.  Faces and points against the restatement, the points
    in the header's float32 arithmetic bit for bit, as test_cloud_ops.py compares."""
    v, f = S.tetrahedra(90000)
    F, n = len(f), 20000
    assert F > S.CLOUD_THREADS * S.CLOUD_CHUNK and S.scan_p(F, S.CLOUD_THREADS, S.CLOUD_CHUNK) == 2     # mesh_scan_kernel: P >= 2
    clock = Clock(device)
    want32, want_face = clock.ref(lambda: cloud_ref.sample_mesh(v, f, n, seed=11, float32=True))
    dv, df = _dev(v, device), _dev(f, device)
    pts, face = clock.dev(lambda: evaluation.sample_mesh(dv, df, n, seed=11, return_faces=True))
    assert pts.dtype == torch.float32 and pts.shape == (n, 3) and face.dtype == torch.int32 and face.shape == (n,)
    assert np.array_equal(face.cpu().numpy(), want_face) and want_face.max() > S.CLOUD_THREADS * S.CLOUD_CHUNK
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), want32.view(np.uint32))
    clock.report(f"sample_mesh, {F} faces")


def test_filter_scans_above_512_chunks(device):
    """mesh_filter_scan_kernel's two direct scan_in_place calls with more totals than threads: 300000 tetrahedra, every
    seventh without its last face (a cluster of 3, dropped at min_triangles = 4), so V = 1200000 and T = 1157142 are both
    above 1048576 and the compaction of vertices and faces is not the identity.  Against the header on the host and the
    closed form."""
    n = 300000
    v, f = S.tetrahedra(n)
    t = np.arange(len(f))
    f = f[~((t // 4 % 7 == 0) & (t % 4 == 3))]
    V, T = len(v), len(f)
    assert T == 1157142 and min(V, T) > S.MESH_THREADS * S.MESH_CHUNK
    assert S.scan_p(V, S.MESH_THREADS, S.MESH_CHUNK) == 2 and S.scan_p(T, S.MESH_THREADS, S.MESH_CHUNK) == 2
    clock = Clock(device)
    want_v, want_f, want_n = clock.ref(lambda: mesh_ref.host().select(v, f, 1, 4))
    whole = np.arange(n) % 7 != 0                                   # the closed form: the whole tetrahedra, renumbered
    assert want_n == 4 and np.array_equal(bits(want_v), bits(v.reshape(n, 4, 3)[whole].reshape(-1, 3)))
    assert np.array_equal(want_f, S.tetrahedra(int(whole.sum()))[1])
    got_v, got_f, det = clock.dev(lambda: mesh_ops.keep_clusters(_dev(v, device), _dev(f, device), keep_clusters=1, min_triangles=4, details=True))
    assert det["n_min"] == 4 and det["clusters"] == n and got_f.dtype == torch.int32
    assert np.array_equal(bits(got_v.cpu().numpy()), bits(want_v)) and np.array_equal(got_f.cpu().numpy(), want_f)
    clock.report(f"keep_clusters, V={V} T={T}")


@pytest.mark.parametrize("contraction", (simplify_ref.AVERAGE, simplify_ref.QUADRIC))
def test_simplify_scans_above_512_chunks(device, contraction):
    """simplify_layout scans the chunk totals of the V vertices (simp_vscan_kernel: scan_totals; simp_scan_kernel: blk_v) and
    of the T triangles (simp_scan_kernel: blk_t).  simplify_ref.strip(n) has T = n and V = n + 2, so n = 1048577 is the
    smallest strip at which both have 513 totals for 512 threads."""
    n = 1048577
    v, f = simplify_ref.strip(n)
    assert S.chunks(len(f), S.MESH_CHUNK) == 513 and S.chunks(len(v), S.MESH_CHUNK) == 513 and S.chunks(n - 1, S.MESH_CHUNK) == 512
    clock = Clock(device)
    want_v, want_f, want_m, want_s = clock.ref(lambda: simplify_ref.host().simplify(v, f, 1.0, contraction))
    got_v, got_f, got_m, status = clock.dev(lambda: _simplify(device, v, f, 1.0, contraction))
    assert status == want_s + [9, 9]
    nv, nt = status[0], status[1]
    assert nv > 100000 and nt > 100000 and status[5] > 0            # kept triangles, and duplicates dropped
    assert np.array_equal(got_f[:nt], want_f) and np.array_equal(got_m, want_m)
    assert np.array_equal(bits(got_v[:nv]), bits(want_v))
    assert (got_v[nv:] == 7.0).all() and (got_f[nt:] == -7).all()   # rows beyond V' / T' are untouched
    clock.report(f"simplify, strip of {n}, contraction {contraction}")


# ---- 8. the cloud's component numbering and row compaction above 256 chunks --------------------------------------------
def test_cluster_scans_above_256_chunks(device):
    """90000 groups of three points, group g at a = (16 (g % 300), 16 (g // 300), 0): a, a + (1, 0, 0), a + (8, 0, 0).  At
    eps = 1.5 and min_points = 2 the first two are each other's neighbours and core, the third has nobody: labels g, g, -1
    in closed form.  M = 270000 is 264 chunks of 1024, so cluster_rootscan_kernel and cluster_keep_scan_kernel add 264 chunk
    totals with 256 threads, and cluster_rank / cluster_keep_write rank past the first 256 chunks.  Integers below 2^13:
    every distance is exact."""
    G = 90000
    M = 3 * G
    assert M > S.CLOUD_THREADS * S.CLOUD_CHUNK and S.chunks(M, S.CLOUD_CHUNK) == 264
    assert S.scan_p(M, S.CLOUD_THREADS, S.CLOUD_CHUNK) == 2         # cluster_rootscan_kernel, cluster_keep_scan_kernel: P >= 2
    clock = Clock(device)
    g = np.arange(G)
    a = np.stack([16 * (g % 300), 16 * (g // 300), 0 * g], 1)
    points = (a[:, None, :] + np.array([[0, 0, 0], [1, 0, 0], [8, 0, 0]])[None]).reshape(M, 3).astype(np.float32)
    assert points.max() < 2 ** 13
    want_labels = np.stack([g, g, -np.ones_like(g)], 1).reshape(M).astype(np.int32)
    want_index = np.flatnonzero(np.arange(M) % 3 != 2).astype(np.int32)
    want_details = {"clusters": G, "core": 2 * G, "border": 0, "noise": G, "largest": 2}
    p = _dev(points, device)
    labels, counts, det = clock.dev(lambda: evaluation.cluster_dbscan(p, 1.5, 2, return_counts=True, details=True))
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and counts.shape == (G,)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and bool((counts == 2).all()) and det == want_details
    out, index, kdet = clock.dev(lambda: evaluation.keep_clusters(p, 1.5, 2, keep=0, min_cluster_points=2, return_index=True, details=True))
    assert kdet == {"kept": 2 * G, "removed": G, "n_min": 2, **want_details}
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), want_index)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), points[want_index].view(np.uint32))
    clock.report(f"cluster_dbscan + keep_clusters, M={M}")
