"""NumPy restatement of include/sls_cluster_math.h: DBSCAN over all pairs with the header's border rule, the numbering by
lowest core index, and the selection rule of the mesh filter.

Lattice inputs only for `dbscan`: coordinates that are multiples of 1/16 of magnitude <= 64 (and eps a multiple of 1/16),
where the header's float32 d2 and eps * eps are exact (include/sls_nn_math.h), so the integer arithmetic here — squared
distances counted in 1/256 — gives the same comparisons.  `dbscan` asserts that its input is such a lattice.  (line_cloud
alone reaches beyond +-64, to +-625: its y and z are 0, so the header's d2 is the rounded dx * dx — exact below 2^16, far
above every eps * eps used here, and rounding is monotone beyond.)"""
import numpy as np

NONE = np.int64(1) << 40


def _sixteenths(a, what):
    q = np.asarray(a, np.float64) * 16.0
    assert np.all(q == np.round(q)), f"{what}: not on the 1/16 lattice"
    assert np.all(np.abs(q) <= 64 * 16) or (q.ndim == 2 and not q[:, 1:].any() and np.all(np.abs(q) <= 1024 * 16)), f"{what}: beyond +-64"
    return q


def neighbour_pairs(points, eps, chunk=512):
    """(i, j) of every ordered pair with d2 <= eps * eps, i == j included: all pairs, exact on the lattice, in chunks of
    rows sorted along x against the rows whose x lies within eps of the chunk's (the others are farther than eps)."""
    P = _sixteenths(points, "points").reshape(-1, 3)
    reach = float(_sixteenths(eps, "eps"))
    r2 = reach ** 2
    order = np.argsort(P[:, 0], kind="stable")
    Q = P[order]
    xs, n2 = Q[:, 0], (Q * Q).sum(1)
    ii, jj = [], []
    for a in range(0, len(Q), chunk):
        b = min(a + chunk, len(Q))
        lo, hi = np.searchsorted(xs, xs[a] - reach, "left"), np.searchsorted(xs, xs[b - 1] + reach, "right")
        d2 = n2[a:b, None] + n2[None, lo:hi] - 2.0 * (Q[a:b] @ Q[lo:hi].T)        # integers below 2^53: exact
        i, j = np.nonzero(d2 <= r2)
        ii.append(order[i + a])
        jj.append(order[j + lo])
    return (np.concatenate(ii), np.concatenate(jj)) if ii else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def components(M, i, j):
    """root[x] = the lowest element of x's component of the graph with the edges (i, j): min-label propagation with
    pointer jumping until nothing changes."""
    root = np.arange(M, dtype=np.int64)
    while True:
        new = root.copy()
        np.minimum.at(new, i, root[j])
        np.minimum.at(new, j, root[i])
        new = new[new]
        if np.array_equal(new, root):
            return root
        root = new


def dbscan(points, eps, min_points):
    """dict(labels (M,) int32, counts (C,) int32, status (8,) uint32, core (M,) bool)"""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    M = len(P)
    i, j = neighbour_pairs(P, eps)
    core = np.bincount(i, minlength=M) >= min_points
    cc = core[i] & core[j]
    root = components(M, i[cc], j[cc])
    root[~core] = NONE
    # borders: the lowest root among the core neighbours
    b = ~core[i] & core[j]
    best = np.full(M, NONE)
    np.minimum.at(best, i[b], root[j[b]])
    root = np.where(core, root, best)
    roots = np.flatnonzero(core & (root == np.arange(M)))                       # ascending: the numbering
    number = np.full(M + 1, -1, np.int64)
    number[roots] = np.arange(len(roots))
    labels = number[np.where(root == NONE, M, root)].astype(np.int32)
    counts = np.bincount(labels[labels >= 0], minlength=len(roots)).astype(np.int32)
    border = ~core & (labels >= 0)
    status = np.array([len(roots), core.sum(), border.sum(), (labels < 0).sum(), counts.max() if len(roots) else 0, M, 0, 1], np.uint32)
    return {"labels": labels, "counts": counts, "status": status, "core": core}


def select(labels, counts, keep, min_cluster_points):
    """(kept rows ascending (int32), status (4,) uint32) — the rule of the mesh filter"""
    labels, counts = np.asarray(labels), np.asarray(counts)
    C = len(counts)
    k = min(keep, C) if keep > 0 else 0
    kth = int(np.sort(counts)[::-1][k - 1]) if k > 0 else 0
    n_min = max(max(int(min_cluster_points), 0), kth)
    keep_mask = (labels >= 0) & (counts[np.maximum(labels, 0)] >= n_min) if C else np.zeros(len(labels), bool)
    index = np.flatnonzero(keep_mask).astype(np.int32)
    return index, np.array([len(index), n_min, len(labels), 1], np.uint32)


# ---- the clouds of the tests (lattice unless said otherwise), each a function of its arguments alone -----------------
def lattice_cloud(M, seed, half=4.0):
    """M points of the 1/16 lattice in a cube: dense clumps, sparse background, duplicates, shuffled"""
    rng = np.random.default_rng(seed)
    n_clump = M // 2
    centres = rng.integers(-int(half * 16) + 16, int(half * 16) - 15, (max(1, M // 60), 3))
    clump = centres[rng.integers(0, len(centres), n_clump)] + rng.integers(-6, 7, (n_clump, 3))
    rest = rng.integers(-int(half * 16), int(half * 16) + 1, (M - n_clump, 3))
    pts = np.concatenate([clump, rest]) / 16.0
    if M >= 8:
        pts[-3:] = pts[:3]                                                      # exact duplicates
    return pts[rng.permutation(M)].astype(np.float32)


def saturation_cloud(min_points):
    """Three stars on the 1/16 lattice at eps = 0.25: a centre with exactly min_points - 2, - 1 and + 0 others AT distance
    eps (so the centre's count, itself included, is min_points - 1, min_points, min_points + 1), the others of a star
    pairwise farther than eps apart where the geometry allows; far apart from each other.  Returns (points, centre rows)."""
    dirs = np.array([[4, 0, 0], [-4, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 4], [0, 0, -4]], np.float64)     # |d| = 4/16 = eps
    pts, centres = [], []
    for s, others in enumerate((min_points - 2, min_points - 1, min_points)):
        c = np.array([s * 160.0 - 160.0, 0.0, 0.0])
        centres.append(len(pts))
        pts.append(c)
        for t in range(others):
            pts.append(c + dirs[t % 6])                                        # beyond six: exact copies of the arms
    return (np.array(pts) / 16.0).astype(np.float32), centres


def bridge_cloud():
    """Two dense blobs of 27 lattice points (spacing 1/16) whose nearest points are 7/16 apart, and ONE point between them,
    4/16 from one point of A and within 4/16 of ten points of B: at eps = 0.25 every blob point has its whole blob for
    neighbours (27 or 28 with the bridge) and the bridge has 12, so at min_points = 20 it is a border of both and joins
    nothing.  Row 0 is the bridge — lower than every core — then B (cluster 0), then A (cluster 1)."""
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float64)
    a = g + [-6, -1, -1]                                                        # x in -6 .. -4: the face x = -4, bridge at x = 0
    b = g + [3, -1, -1]                                                         # x in 3 .. 5
    bridge = np.array([[0.0, 0.0, 0.0]])
    return (np.concatenate([bridge, b, a]) / 16.0).astype(np.float32)


def line_cloud(n=5000, seed=5):
    """n points along x at 0.8 eps spacing for eps = 5/16: spacing 4/16, shuffled; one cluster that crosses many boxes"""
    x = (np.arange(n) - n // 2) * 4.0
    pts = np.stack([x, np.zeros(n), np.zeros(n)], 1) / 16.0
    return pts[np.random.default_rng(seed).permutation(n)].astype(np.float32)


def dense_cloud(n=20000, seed=6):
    """n distinct points of the 1/16 lattice filling a 28^3 block: one component at eps = 2/16, shuffled"""
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*(np.arange(side),) * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    return ((g - side // 2) / 16.0)[np.random.default_rng(seed).permutation(n)].astype(np.float32)


# ---- include/sls_cluster_math.h compiled for the host: the serial all-pairs routine, on any finite input -------------
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "sls_cluster_math.h"
/* in: M int32, eps float, min_points int32, keep int32, min_cluster_points int32, M x 3 floats
 * out: rc int32, 8 uint32, M int32 (labels), M int32 (counts; from C on: zeros), 4 uint32, M int32 (kept rows; from kept on: -1) */
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int32_t hdr[5];
    float eps;
    if (argc != 3 || !in || !out || fread(hdr, 4, 5, in) != 5) return 2;
    const int32_t M = hdr[0], mp = hdr[2], keep = hdr[3], mcp = hdr[4];
    __builtin_memcpy(&eps, &hdr[1], 4);
    const size_t n = (size_t)(M > 0 ? M : 0);
    float *xyz = malloc(12 * n + 4);
    int32_t *labels = malloc(4 * n + 4), *counts = malloc(4 * n + 4), *index = malloc(4 * n + 4);
    uint32_t *work = malloc(4 * n + 4), status[8] = { 0 }, sel[4] = { 0 };
    if (fread(xyz, 12, n, in) != n) return 2;
    int32_t rc = sls_cluster_dbscan_host(M, xyz, eps, mp, labels, counts, status, work);
    if (!rc) {
        for (size_t c = status[0]; c < n; ++c) counts[c] = 0;
        rc = sls_cluster_select_host(M, labels, counts, status[0], keep, mcp, index, sel);
        for (size_t c = sel[0]; c < n; ++c) index[c] = -1;
    }
    fwrite(&rc, 4, 1, out); fwrite(status, 4, 8, out); fwrite(labels, 4, n, out); fwrite(counts, 4, n, out);
    fwrite(sel, 4, 4, out); fwrite(index, 4, n, out);
    fclose(in); fclose(out);
    return 0;
}
'''


def build_host(directory):
    """gcc -> the program above (for the machine it runs on: fmaf is then one instruction, not a call — the result is the
    same correctly rounded value either way); returns its path, or None without gcc"""
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(str(directory), "cluster_math.c"), os.path.join(str(directory), "cluster_math")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-march=native", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), src, "-o", exe, "-lm"])
    return exe


def run_host(exe, directory, points, eps, min_points, keep=1, min_cluster_points=0):
    """dict(rc, labels, counts (C,), status, index (kept,), select_status) of the header's serial routines"""
    import os
    import struct
    import subprocess
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    M = len(P)
    fin, fout = os.path.join(str(directory), "in.bin"), os.path.join(str(directory), "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<ifiii", M, eps, min_points, keep, min_cluster_points) + P.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, np.int32)
    assert len(raw) == 1 + 8 + 2 * M + 4 + M
    status, sel = raw[1:9].view(np.uint32), raw[9 + 2 * M:13 + 2 * M].view(np.uint32)
    return {"rc": int(raw[0]), "status": status, "labels": raw[9:9 + M], "counts": raw[9 + M:9 + M + int(status[0])],
            "select_status": sel, "index": raw[13 + 2 * M:13 + 2 * M + int(sel[0])]}
