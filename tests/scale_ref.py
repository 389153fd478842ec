"""What the size tests (tests/test_scale_paths.py) share: the constants that decide where the second level of the sorter, of
the chunked scan, of the box search and of the capped reductions begins, as the sources define them (tests/test_scale_host.py
matches them against the sources as text); references that stay a few seconds at 10^5 .. 10^6 items — a lexsort weld, a
block-diagonal k-NN over clouds whose parts are provably separated, closed forms for index-offset copies of one small mesh —
and the bounds of the float64 sums at these sizes.  Every large input is built once (functools.lru_cache) and is read-only."""
import functools
import math

import numpy as np

import nn_ref
import outlier_ref

# ---- the constants and where the sources define them -----------------------------------------------------------------
SORT_WAVE_ITEMS = 1024          # items per wave (= per chunk of the count table) of the radix sort: 64 lanes x 16 rounds
ROWSCAN_THREADS = 256           # sort_rowscan_kernel: thread t owns P = ceil(nchunks / 256) consecutive entries of a row
ROWSCAN_KEEP = 8                # ... of which it keeps 8 in registers; the tail loop runs from P = 9 on
CLOUD_THREADS, CLOUD_CHUNK = 256, 1024      # Chunks<256, 4>: voxel down-sampling, mesh sampling, the outlier filters, the clusters
MESH_THREADS, MESH_CHUNK = 512, 2048        # Chunks<512, 4>: weld, clusters, filter, simplify, adjacency, fill, TSDF blocks
KNN_BOX = 256                   # target points per box of the box search
SWEEP_BOXES = 64                # boxes per chunk of the outward sweep (a box per lane)
REDUCE_THREADS = 256            # outlier_partial / nn_stats_partial: points per block below the cap; the final kernel's threads
REDUCE_MAX_BLOCKS = 1024        # kOutMaxBlocks, kNnStatsMaxBlocks: the grid cap of both reductions
LONG_MAX_BLOCKS = 2048          # kLongMaxBlocks, kFillLongBlocks: the grid cap of the long-row and the long-loop kernel
LONG_WAVES = 4                  # waves per block of either (256 threads): a wave per row or loop
LONG_ROW = 64                   # SLS_SMOOTH_LONG, SLS_FILL_LONG: rows / loops above it are the long ones

# (file, the text the file must hold, the size tests that stop covering their path when it changes)
SOURCES = (
    ("splat_loam_amd/csrc/sls_radix.hip", "#define SLS_SORT_ROUNDS 16", "weld, voxel, tsdf: every P threshold of the sorter"),
    ("splat_loam_amd/csrc/sls_radix.hip", "constexpr int kSortWaveItems = kWave * kSortRounds;", "weld, voxel, tsdf"),
    ("splat_loam_amd/csrc/sls_common.hpp", "constexpr int kWave = 64;", "weld, voxel, tsdf"),
    ("splat_loam_amd/csrc/sls_radix.hip", "__global__ __launch_bounds__(256) void sort_rowscan_kernel(", "weld, voxel, tsdf"),
    ("splat_loam_amd/csrc/sls_radix.hip", "const int P = (nchunks + 255) / 256,", "weld, voxel, tsdf"),
    ("splat_loam_amd/csrc/sls_radix.hip", "constexpr int kKeep = 8;", "test_weld_rowscan_and_head_scan[2098177], test_tsdf_blocks_sort_tail"),
    ("splat_loam_amd/csrc/sls_cloud.hip", "constexpr int kCloudThreads = 256;", "test_voxel_*"),
    ("splat_loam_amd/csrc/sls_cloud.hip", "using CloudChunks = Chunks<kCloudThreads, 4>;", "test_voxel_*, test_mesh_sample_*"),
    ("splat_loam_amd/csrc/sls_outlier.hip", "constexpr int kOutThreads = 256;", "test_statistical_*, test_radius_*"),
    ("splat_loam_amd/csrc/sls_outlier.hip", "using OutChunks = Chunks<kOutThreads, 4>;", "test_statistical_*, test_radius_*"),
    ("splat_loam_amd/csrc/sls_outlier.hip", "constexpr int kOutMaxBlocks = 1024;", "test_statistical_*"),
    ("splat_loam_amd/csrc/sls_cluster.hip", "constexpr int kCluThreads = 256;", "test_cluster_scans_above_256_chunks"),
    ("splat_loam_amd/csrc/sls_cluster.hip", "using CluChunks = Chunks<kCluThreads, 4>;", "test_cluster_scans_above_256_chunks"),
    ("splat_loam_amd/csrc/sls_mesh.hip", "constexpr int kMeshThreads = 512;", "test_weld_*, test_tetrahedra_*"),
    ("splat_loam_amd/csrc/sls_mesh.hip", "using MeshChunks = Chunks<kMeshThreads, 4>;", "test_weld_*, test_tetrahedra_*"),
    ("splat_loam_amd/csrc/sls_simplify.hip", "constexpr int kSimpThreads = 512;", "test_simplify_*"),
    ("splat_loam_amd/csrc/sls_simplify.hip", "using SimpChunks = Chunks<kSimpThreads, 4>;", "test_simplify_*"),
    ("splat_loam_amd/csrc/sls_smooth.hip", "constexpr int kAdjThreads = 512;", "test_fans_smooth_long_rows_stride"),
    ("splat_loam_amd/csrc/sls_smooth.hip", "using AdjChunks = Chunks<kAdjThreads, 4>;", "test_fans_smooth_long_rows_stride"),
    ("splat_loam_amd/csrc/sls_smooth.hip", "constexpr int kStepThreads = 256;", "test_fans_smooth_long_rows_stride"),
    ("splat_loam_amd/csrc/sls_smooth.hip", "constexpr int kLongMaxBlocks = 2048;", "test_fans_smooth_long_rows_stride"),
    ("splat_loam_amd/csrc/sls_fill.hip", "constexpr int kFillThreads = 512;", "test_fans_fill_long_loops_stride"),
    ("splat_loam_amd/csrc/sls_fill.hip", "using FillChunks = Chunks<kFillThreads, 4>;", "test_fans_fill_long_loops_stride"),
    ("splat_loam_amd/csrc/sls_fill.hip", "constexpr int kFillLongBlocks = 2048;", "test_fans_fill_long_loops_stride"),
    ("splat_loam_amd/csrc/sls_fill.hip", "constexpr int kFillLongThreads = 256;", "test_fans_fill_long_loops_stride"),
    ("splat_loam_amd/csrc/sls_tsdf.hip", "constexpr int kTsdfThreads = SLS_TSDF_BLOCK_VOXELS;", "test_tsdf_blocks_sort_tail"),
    ("splat_loam_amd/csrc/sls_tsdf.hip", "using TsdfChunks = Chunks<kTsdfThreads, 4>;", "test_tsdf_blocks_sort_tail"),
    ("include/sls_tsdf_math.h", "#define SLS_TSDF_BLOCK_VOXELS 512", "test_tsdf_blocks_sort_tail"),
    ("include/sls_tsdf_math.h", "#define SLS_TSDF_POINT_KEYS 27", "test_tsdf_blocks_sort_tail"),
    ("splat_loam_amd/csrc/sls_sweep.hpp", "constexpr int kSweepBox = 256;", "test_nearest_k_*"),
    ("splat_loam_amd/csrc/sls_sweep.hpp", "const int nchunks = (nboxes + 63) / 64, c0 = start_box / 64;", "test_nearest_k_*"),
    ("splat_loam_amd/csrc/sls_metrics.hip", "constexpr int kNnStatsMaxBlocks = SLS_NN_STATS_SCRATCH_BYTES / 32;", "test_nearest_and_metrics_*"),
    ("include/sls_abi.h", "#define SLS_NN_STATS_SCRATCH_BYTES 32768", "test_nearest_and_metrics_*"),
    ("splat_loam_amd/csrc/sls_metrics.hip", "int nblocks = (M + 255) / 256;", "test_nearest_and_metrics_*"),
    ("include/sls_smooth_math.h", "#define SLS_SMOOTH_LONG 64", "test_fans_smooth_long_rows_stride"),
    ("include/sls_fill_math.h", "#define SLS_FILL_LONG 64", "test_fans_fill_long_loops_stride"),
)


def chunks(n, per):
    return (int(n) + per - 1) // per


def rowscan_p(n):
    """P of sort_rowscan_kernel for n items: the entries of a count-table row one thread owns"""
    return chunks(chunks(n, SORT_WAVE_ITEMS), ROWSCAN_THREADS)


def scan_p(n, threads, chunk):
    """P of scan_in_place over the chunk totals of n positions: the totals one thread owns"""
    return chunks(chunks(n, chunk), threads)


def sweep_chunks(Mt):
    """the chunks of 64 boxes the k-NN sweep steps over for Mt target points"""
    return chunks(chunks(Mt, KNN_BOX), SWEEP_BOXES)


def reduce_blocks(M):
    """the partials of the outlier and nn_stats reductions"""
    return min(chunks(M, REDUCE_THREADS), REDUCE_MAX_BLOCKS)


def smooth_long_waves(V, T):
    """the waves sls_mesh_smooth launches for its long rows: the launcher sizes the grid by long_cap = min(6 T / 65 + 1, V),
    not by the live count, a wave per row, four waves per block, at most LONG_MAX_BLOCKS blocks.  A wave takes a second row
    from this many long rows + 1 on."""
    long_cap = min(6 * T // (LONG_ROW + 1) + 1, V)
    return min(chunks(long_cap, LONG_WAVES), LONG_MAX_BLOCKS) * LONG_WAVES


def fill_long_waves(T):
    """the waves sls_mesh_fill_holes launches for its long loops: (T / 65 + 4) / 4 blocks, at most LONG_MAX_BLOCKS, four waves
    each; the waves stride over ALL loops and skip the short ones.  A wave takes a second loop from this many loops + 1 on."""
    return min((T // (LONG_ROW + 1) + LONG_WAVES) // LONG_WAVES, LONG_MAX_BLOCKS) * LONG_WAVES


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- weld ------------------------------------------------------------------------------------------------------------
def weld_lexsort(rows):
    """mesh_ref.weld without np.unique(axis=0): a lexsort of the int32 view (x the most significant word), heads where a
    sorted row differs from the one before, ranks by cumsum.  (vertices (V,3) float32, index (N,) int64)."""
    w = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 3).view(np.int32)
    if len(w) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0,), np.int64)
    order = np.lexsort((w[:, 2], w[:, 1], w[:, 0]))
    s = w[order]
    head = np.ones((len(s),), bool)
    head[1:] = (s[1:] != s[:-1]).any(1)
    index = np.empty((len(s),), np.int64)
    index[order] = np.cumsum(head) - 1
    return s[head].view(np.float32), index


# ---- clouds whose parts are separated: a block-diagonal k-NN -----------------------------------------------------------
CLUSTER_POINTS = 500
CLUSTER_HALF = 2.0              # a cluster's points lie within +-2 of its centre per axis: diameter <= 4 sqrt(3) < 6.93
CLUSTER_PITCH = 12.0            # the centres' grid: the gap between two clusters is >= 12 - 4 = 8 > the diameter
GRIDS = {540: (10, 9, 6), 135: (5, 9, 3), 6: (3, 2, 1)}
Z_LOW = -58.0                   # the lowest layer of centres: the clusters end at z = 4, the far slab begins at FAR_Z
FAR_Z = (24.0, 64.0)


def _snap(x):
    return np.round(np.asarray(x) * 16.0) / 16.0


@functools.lru_cache(maxsize=None)
def clustered_cloud(n_clusters, seed):
    """(points (n_clusters * 500, 3) float32, label (n,) int64), shuffled, read-only: clusters of 500 points of the 1/16
    lattice, each within +-2 of its centre, the centres on a grid 12 apart; every coordinate's magnitude is <= 64, so the
    float32 squared distance is exact.  Asserts what the block-diagonal reference rests on: the smallest gap between two
    clusters exceeds the largest diameter of one, so the 500 nearest points of a point are its own cluster."""
    gx, gy, gz = GRIDS[n_clusters]
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    centres = g * CLUSTER_PITCH - np.array([(gx - 1) * 6.0, (gy - 1) * 6.0, -Z_LOW])
    off = rng.integers(-int(CLUSTER_HALF * 16), int(CLUSTER_HALF * 16) + 1, (n_clusters, CLUSTER_POINTS, 3)) / 16.0
    pts = (centres[:, None, :] + off).reshape(-1, 3)
    label = np.repeat(np.arange(n_clusters), CLUSTER_POINTS)
    lo, hi = (centres[:, None, :] + off).min(1), (centres[:, None, :] + off).max(1)         # every cluster's box
    diameter = float(np.linalg.norm(hi - lo, axis=1).max())                               # >= the true diameter
    gap2 = np.full((n_clusters,), np.inf)
    for c in range(n_clusters):                                                           # box to box: <= the true gap
        d = np.maximum(0.0, np.maximum(lo - hi[c], lo[c] - hi))
        d2 = (d * d).sum(1)
        d2[c] = np.inf
        gap2[c] = d2.min()
    assert math.sqrt(gap2.min()) > diameter, (math.sqrt(gap2.min()), diameter)
    assert np.abs(pts).max() <= 64.0 and pts.shape[0] >= 32
    perm = rng.permutation(len(pts))
    return _frozen(pts[perm].astype(np.float32), label[perm])


def keys_k_blockdiag(target, target_label, k, query=None, query_label=None):
    """outlier_ref.keys_k on a cloud whose parts are separated (the caller asserts it): every part's queries against that
    part's targets alone, the indices mapped back to rows of `target`.  query None: the cloud queried by itself."""
    target = np.asarray(target, np.float32)
    if query is None:
        query, query_label = target, target_label
    query = np.asarray(query, np.float32)
    out = np.full((len(query), k), outlier_ref.KEY_NONE, np.uint64)
    t_order, q_order = np.argsort(target_label, kind="stable"), np.argsort(query_label, kind="stable")
    t_parts, t_start = np.unique(target_label[t_order], return_index=True)
    t_end = np.append(t_start[1:], len(t_order))
    q_sorted = query_label[q_order]
    for part, a, b in zip(t_parts, t_start, t_end):
        rows = t_order[a:b]                                             # ascending: the lowest index still wins a tie
        qa, qb = np.searchsorted(q_sorted, part, "left"), np.searchsorted(q_sorted, part, "right")
        if qa == qb:
            continue
        q_rows = q_order[qa:qb]
        keys = outlier_ref.keys_k(target[rows], query[q_rows], k)
        d2, local = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
        some = keys != outlier_ref.KEY_NONE
        mapped = np.where(some, rows[np.where(some, local, 0).astype(np.int64)].astype(np.uint64), np.uint64(0xFFFFFFFF))
        out[q_rows] = (d2 << np.uint64(32)) | mapped
    return out


@functools.lru_cache(maxsize=None)
def filter_cloud(n_clusters, seed):
    """(points (M,3) float32, label (M,), normals (M,3) float32), read-only: clustered_cloud and a share of M' // 25 far points
    added as outlier_ref.filter_cloud adds them — drawn from the 1/16 lattice, shuffled in — but confined to the slab
    FAR_Z above the clusters, so that they form one more separated part (label n_clusters) and the block-diagonal reference
    stays exact: filter_keys asserts that the slab is farther from the clusters than any far point's 32nd neighbour."""
    pts, label = clustered_cloud(n_clusters, seed)
    rng = np.random.default_rng(seed + 1)
    n_far = len(pts) // 25
    far = np.stack([rng.integers(-1024, 1025, n_far), rng.integers(-1024, 1025, n_far),
                    rng.integers(int(FAR_Z[0] * 16), int(FAR_Z[1] * 16) + 1, n_far)], 1) / 16.0
    allp = np.concatenate([pts, far.astype(np.float32)])
    alll = np.concatenate([label, np.full((n_far,), n_clusters)])
    perm = rng.permutation(len(allp))
    nrm = rng.normal(0, 1, (len(allp), 3)).astype(np.float32)
    return _frozen(allp[perm], alll[perm], nrm)


@functools.lru_cache(maxsize=None)
def filter_keys(n_clusters, seed):
    """(M, 32) uint64, read-only: the 32 smallest keys of every point of filter_cloud queried by itself"""
    pts, label, _ = filter_cloud(n_clusters, seed)
    keys = keys_k_blockdiag(pts, label, 32)
    far = label == n_clusters
    reach = float(np.sqrt(outlier_ref.split(keys[far, 31])[0].astype(np.float64)).max())     # the far points' 32nd neighbour
    gap = FAR_Z[0] - float(pts[~far, 2].max())
    assert gap > reach and gap > 2 * CLUSTER_HALF * math.sqrt(3.0), (gap, reach)
    return _frozen(keys)


def statistical_from_keys(keys, k, std_ratio):
    """outlier_ref.statistical from the self-query's keys (at least k columns): the same dictionary"""
    M = len(keys)
    mean = outlier_ref.means(keys[:, :k], M)
    counted = mean > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        cloud_mean = mean[counted].sum() / np.float64(M)
        std = np.sqrt(np.square(mean[counted] - cloud_mean).sum() / np.float64(M - 1))
        thr = cloud_mean + np.float64(std_ratio) * std
        keep = counted & (mean < thr)
        margin = float(np.abs(mean - thr).min() / thr) if M else float("nan")
    return {"keep": keep, "mean": mean, "cloud_mean": float(cloud_mean), "std": float(std), "thr": float(thr),
            "zero_mean": int((~counted).sum()), "margin": margin}


def radius_from_keys(keys, nb_points, radius_):
    """outlier_ref.radius from the self-query's keys (more than nb_points columns)"""
    r = np.float32(radius_)
    rank = keys[:, nb_points]
    return (rank != outlier_ref.KEY_NONE) & (outlier_ref.split(rank)[0] <= np.float32(r * r))


def metrics_from_dist2(d_acc, d_com, threshold=0.2, truncation_acc=0.5, truncation_com=0.5):
    """nn_ref.cloud_metrics from the two arrays of float32 squared distances (estimate -> reference, reference -> estimate)"""
    n_acc, below_acc, sum_acc, _ = nn_ref.stats(d_acc, truncation_acc, threshold, False)
    n_com, below_com, sum_com, _ = nn_ref.stats(d_com, truncation_com, threshold, True)
    accuracy = sum_acc / n_acc if n_acc else float("nan")
    precision = below_acc / n_acc if n_acc else float("nan")
    completeness, recall = sum_com / n_com, below_com / n_com
    pr = precision + recall
    return {"accuracy_m": accuracy, "completeness_m": completeness, "chamfer_l1_m": 0.5 * (accuracy + completeness),
            "precision": precision, "recall": recall, "fscore": 2.0 * precision * recall / pr if pr != 0 else 0.0,
            "n_accuracy": n_acc, "n_completeness": n_com,
            "threshold": float(threshold), "truncation_acc": float(truncation_acc), "truncation_com": float(truncation_com)}


@functools.lru_cache(maxsize=None)
def estimate_cloud(n_clusters, seed):
    """(estimate (M,3) float32, label): clustered_cloud moved by up to 3/16 per axis, reshuffled.  A moved point is within
    0.33 of its original and at least 8 - 0.33 from every other cluster, so either cloud's nearest point in the other lies
    in the same cluster: the block-diagonal reference holds in both directions."""
    pts, label = clustered_cloud(n_clusters, seed)
    rng = np.random.default_rng(seed + 2)
    moved = pts + (rng.integers(-3, 4, pts.shape) / 16.0).astype(np.float32)
    perm = rng.permutation(len(pts))
    assert np.abs(moved).max() <= 64.0
    return _frozen(moved[perm], label[perm])


# ---- the bounds of the float64 sums ------------------------------------------------------------------------------------
U = 2.0 ** -53


def sum_bound(M):
    """The relative distance of two float64 sums of the same M non-negative terms taken in any two orders: either is within
    (M - 1) u of the exact sum, the division that follows adds u: 2 M u."""
    return 2.0 * M * U


def std_bound(M, cloud_mean, std):
    """std = sqrt(Q / (M - 1)), Q = sum (mean_i - c)^2 with c the side's own cloud_mean = c* (1 + e), |e| <= M u.
    Q(c) - Q(c*) = -2 d sum (mean_i - c*) + n d^2 with d = c* e, and |sum (mean_i - c*)| <= sqrt(M Q) (Cauchy-Schwarz), so the
    shifted centre moves Q by at most 2 |e| (c* / s) relative, s = sqrt(Q / M) ~ std; the subtraction, the square and the
    sum of M non-negative terms add (M + 3) u.  The root halves the sum of both, the division and the root add 2 u:
    one side is within (M / 2 + M c / std + 4) u, two sides within (M (1 + 2 c / std) + 8) u.  (First order in u; the
    second-order terms are below 1e-20 here.)"""
    return (M * (1.0 + 2.0 * cloud_mean / std) + 8.0) * U


def thr_bound(M, cloud_mean, std):
    """threshold = cloud_mean + ratio * std, both terms non-negative: the larger of their bounds, the product and the sum
    add 2 u a side"""
    return max(sum_bound(M), std_bound(M, cloud_mean, std)) + 4.0 * U


# ---- index-offset copies of one small mesh -----------------------------------------------------------------------------
TET_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)     # closed and oriented
TET_V = np.array([[0, 0, 0], [1, 0.125, 0], [0.25, 1, 0.125], [0.25, 0.25, 1]], np.float32)


@functools.lru_cache(maxsize=None)
def tetrahedra(n):
    """(vertices (4n,3) float32, faces (4n,3) int32), read-only: n closed tetrahedra, copy i moved by (i % 64, i // 64 % 64,
    i // 4096) * 2 (so the normals of different copies are computed from different coordinates), its indices offset by 4 i"""
    i = np.arange(n)
    shift = np.stack([i % 64, i // 64 % 64, i // 4096], 1).astype(np.float32) * np.float32(2.0)
    v = (TET_V[None, :, :] + shift[:, None, :]).reshape(-1, 3)
    f = (TET_F[None, :, :] + (4 * i)[:, None, None].astype(np.int32)).reshape(-1, 3)
    return _frozen(np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32))


def tetrahedra_clusters(n):
    """What sls_mesh_clusters must give for tetrahedra(n), in closed form: labels t // 4, every count 4, and the status
    words (clusters n, nothing degenerate, no boundary and no non-manifold edge)"""
    stats = {"clusters": n, "degenerate": 0, "out_of_range": 0, "boundary_edges": 0, "nonmanifold_edges": 0}
    return np.arange(4 * n, dtype=np.int64) // 4, np.full((n,), 4, np.int64), stats


def copies(vertices, faces, n):
    """n index-offset copies of a mesh with the SAME coordinates: (vertices (n V,3), faces (n T,3) int32)"""
    V = len(vertices)
    f = (np.asarray(faces, np.int64)[None, :, :] + (np.arange(n, dtype=np.int64) * V)[:, None, None]).reshape(-1, 3)
    return np.ascontiguousarray(np.tile(np.asarray(vertices, np.float32), (n, 1))), f.astype(np.int32)


FAN_COPIES, FAN_N = 8200, 65


@functools.lru_cache(maxsize=None)
def fans():
    """(vertices (541200,3) float32, faces (533000,3) int32), read-only: 8200 copies of smooth_ref.fan(65).  Every hub is a
    row of 65 neighbours (a long row), every rim a boundary loop of 65 half-edges (a long loop)."""
    import smooth_ref
    v, f = smooth_ref.fan(FAN_N)
    return _frozen(*copies(v, f, FAN_COPIES))
