"""Mesh smoothing over the edge graph (sls_mesh_adjacency, sls_mesh_smooth) restated in NumPy — rules 1 to 3 of
include/sls_smooth_math.h, the float32 distance and the float64 sums in the header's order — and that header compiled as
plain C and run on the host (`host()`), plus the case table and the grid of settings the smoothing tests share."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import mesh_ref
from simplify_ref import segment_sum

ROOT = mesh_ref.ROOT
LONG = 64                       # SLS_SMOOTH_LONG
SIMPLE, LAPLACIAN, TAUBIN = 0, 1, 2
UNIFORM, INVERSE_DISTANCE = 0, 1
METHODS = {"simple": SIMPLE, "laplacian": LAPLACIAN, "taubin": TAUBIN}
WEIGHTS = {"uniform": UNIFORM, "inverse_distance": INVERSE_DISTANCE}
STATUS = ("live", "edges", "boundary", "nonfinite", "degenerate", "out_of_range", "max_row")
LAMBDA, MU = 0.5, -0.53


# ---- the restatement -------------------------------------------------------------------------------------------------
def adjacency(faces, V, vertices=None):
    """(offsets (V+1,) int64, neighbours (2E,) int64, boundary (V,) uint8, dict of the status words): np.unique on the directed
    pairs gives every row's distinct neighbours in ascending order, and how many triangles own each edge"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    deg = mesh_ref.degenerate(f, V)
    ok = f[deg == 0]
    pairs = np.concatenate([ok[:, [0, 1]], ok[:, [1, 0]], ok[:, [1, 2]], ok[:, [2, 1]], ok[:, [2, 0]], ok[:, [0, 2]]])
    uniq, owners = (np.unique(pairs, axis=0, return_counts=True) if len(pairs) else (np.zeros((0, 2), np.int64), np.zeros((0,), np.int64)))
    offsets = np.searchsorted(uniq[:, 0], np.arange(V + 1))
    boundary = np.zeros((V,), np.uint8)
    boundary[uniq[owners == 1, 0]] = 1
    lens = np.diff(offsets)
    nonfinite = 0
    if vertices is not None and V:
        with np.errstate(invalid="ignore"):
            nonfinite = int(((lens > 0) & ~np.isfinite(np.asarray(vertices, dtype=np.float32).reshape(-1, 3)).all(1)).sum())
    stats = dict(zip(STATUS, (int((lens > 0).sum()), len(uniq) // 2, int(boundary.sum()), nonfinite, int((deg != 0).sum()),
                             int((deg == 2).sum()), int(lens.max()) if V else 0)))
    return offsets, uniq[:, 1].copy(), boundary, stats


def _items(P, rows, nb, weights):
    """(n, 4) float64: (w x, w y, w z, w) of neighbour nb[j] for vertex rows[j]"""
    pi, pn = P[rows], P[nb]
    if weights == UNIFORM:
        w = np.ones((len(rows),))
    else:
        d = pn - pi                                                 # float32, every operation rounded once
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        w = 1.0 / (dist.astype(np.float64) + 1e-12)
    return np.concatenate([w[:, None] * pn.astype(np.float64), w[:, None]], 1)


def step(P, offsets, neighbours, pinned, simple, weights, f):
    """one step (rule 2): P (V,3) float32 -> (V,3) float32"""
    lens = np.diff(offsets)
    active = (lens > 0) & ~pinned
    out = P.copy()
    weights = UNIFORM if simple else weights
    acc = np.zeros((len(P), 4))
    with np.errstate(all="ignore"):
        rows = np.nonzero(active & (lens <= LONG))[0]
        for k in range(int(lens[rows].max()) if len(rows) else 0):  # item k of every short row at once: each row in ascending k
            has = k < lens[rows]
            nb = neighbours[offsets[rows] + np.where(has, k, 0)]
            acc[rows] = acc[rows] + np.where(has[:, None], _items(P, rows, nb, weights), 0.0)   # (+0.0 changes no sum that starts at +0.0)
        for v in np.nonzero(active & (lens > LONG))[0]:
            nb = neighbours[offsets[v]:offsets[v + 1]]
            acc[v] = segment_sum(_items(P, np.full((len(nb),), v), nb, weights))
        rows = np.nonzero(active)[0]
        x, S, W = P[rows].astype(np.float64), acc[rows, :3], acc[rows, 3:]
        if simple:
            out[rows] = ((x + S) / (lens[rows].astype(np.float64)[:, None] + 1.0)).astype(np.float32)
        else:
            out[rows] = (x + f * (S / W - x)).astype(np.float32)
    return out


def factors(method, iterations, lam=LAMBDA, mu=MU):
    """the factor of every step (None: a simple step)"""
    if method == SIMPLE:
        return [None] * iterations
    return [lam] * iterations if method == LAPLACIAN else [lam, mu] * iterations


def smooth(vertices, faces, iterations, method=TAUBIN, weights=INVERSE_DISTANCE, lam=LAMBDA, mu=MU, fix_boundary=False):
    """(vertices' (V,3) float32, dict of the status words)"""
    P = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    offsets, neighbours, boundary, stats = adjacency(faces, len(P), P)
    pinned = (boundary != 0) if fix_boundary else np.zeros((len(P),), bool)
    for f in factors(method, iterations, lam, mu):
        P = step(P, offsets, neighbours, pinned, f is None, weights, f)
    return P, stats


def status_words(stats):
    return [stats[k] for k in STATUS] + [1]


# ---- the header on the host ------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "sls_smooth_math.h"

static int cmp_u64(const void *pa, const void *pb)
{
    const uint64_t a = *(const uint64_t *)pa, b = *(const uint64_t *)pb;
    return a < b ? -1 : (a > b ? 1 : 0);
}

/* offsets: V + 1, neighbours: room for 6 T (2 E written), boundary: V, status: 8 words; xyz may be null */
void ref_adjacency(int V, int T, const int32_t *faces, const float *xyz, int32_t *offsets, int32_t *neighbours, uint8_t *boundary,
                   uint32_t *status)
{
    memset(status, 0, 8 * sizeof(uint32_t));
    status[7] = 1u;
    for (int v = 0; v <= V; ++v) offsets[v] = 0;
    for (int v = 0; v < V; ++v) boundary[v] = 0;
    if (V == 0 || T == 0) return;
    const int bits = sls_mesh_index_bits(V);
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * 6 * (size_t)T);
    size_t n = 0;
    for (int t = 0; t < T; ++t) {
        const int deg = sls_mesh_degenerate(faces + 3 * (size_t)t, V);
        if (deg) { status[4]++; if (deg == 2) status[5]++; continue; }
        for (int j = 0; j < 6; ++j) keys[n++] = sls_smooth_face_key(faces + 3 * (size_t)t, j, bits);
    }
    qsort(keys, n, sizeof(uint64_t), cmp_u64);
    uint32_t heads = 0;
    int row = 0;                                                   /* offsets[0 .. row] are final */
    for (size_t p = 0; p < n; ++p) {
        if (p > 0 && keys[p] == keys[p - 1]) continue;
        const int a = (int)(keys[p] >> bits);
        while (row < a) offsets[++row] = (int32_t)heads;
        neighbours[heads++] = (int32_t)(keys[p] & (((uint64_t)1 << bits) - 1u));
        if (p + 1 == n || keys[p + 1] != keys[p]) boundary[a] = 1;
    }
    while (row < V) offsets[++row] = (int32_t)heads;
    status[1] = heads / 2u;
    for (int v = 0; v < V; ++v) {
        const uint32_t len = (uint32_t)(offsets[v + 1] - offsets[v]);
        if (len) {
            status[0]++;
            if (xyz && !(sls_smooth_finite(xyz[3 * (size_t)v]) && sls_smooth_finite(xyz[3 * (size_t)v + 1]) && sls_smooth_finite(xyz[3 * (size_t)v + 2])))
                status[3]++;
        }
        status[2] += boundary[v];
        if (len > status[6]) status[6] = len;
    }
    free(keys);
}

/* "the order of every float64 sum" over the row [s, e) of vertex i */
static void row_sums(const float *P, const int32_t *neighbours, int i, int s, int e, int weights, double acc[4])
{
    const float *pi = P + 3 * (size_t)i;
    for (int k = 0; k < 4; ++k) acc[k] = 0.0;
    if (e - s <= SLS_SMOOTH_LONG) {
        for (int p = s; p < e; ++p) { const float *pn = P + 3 * (size_t)neighbours[p]; sls_smooth_add(acc, sls_smooth_weight(pi, pn, weights), pn); }
        return;
    }
    double part[64][4], next[64][4];
    memset(part, 0, sizeof(part));
    for (int p = s; p < e; ++p) { const float *pn = P + 3 * (size_t)neighbours[p]; sls_smooth_add(part[(p - s) % 64], sls_smooth_weight(pi, pn, weights), pn); }
    for (int off = 32; off > 0; off >>= 1) {
        for (int l = 0; l < 64; ++l) for (int k = 0; k < 4; ++k) next[l][k] = part[l][k] + part[l ^ off][k];
        memcpy(part, next, sizeof(part));
    }
    for (int k = 0; k < 4; ++k) acc[k] = part[0][k];
}

void ref_smooth(int V, const float *xyz, int T, const int32_t *faces, int method, int weights, int iterations, double lambda, double mu,
                int fix_boundary, float *out, uint32_t *status)
{
    int32_t *offsets = (int32_t *)malloc(sizeof(int32_t) * ((size_t)V + 1));
    int32_t *neighbours = (int32_t *)malloc(sizeof(int32_t) * (6 * (size_t)T + 1));
    uint8_t *boundary = (uint8_t *)malloc((size_t)V + 1);
    float *cur = (float *)malloc(sizeof(float) * (3 * (size_t)V + 1)), *nxt = (float *)malloc(sizeof(float) * (3 * (size_t)V + 1));
    ref_adjacency(V, T, faces, xyz, offsets, neighbours, boundary, status);
    memcpy(cur, xyz, sizeof(float) * 3 * (size_t)V);
    const int steps = method == SLS_SMOOTH_TAUBIN ? 2 * iterations : iterations;
    for (int k = 0; k < steps; ++k) {
        const double f = (method == SLS_SMOOTH_TAUBIN && (k & 1)) ? mu : lambda;
        for (int i = 0; i < V; ++i) {
            const int s = offsets[i], e = offsets[i + 1];
            memcpy(nxt + 3 * (size_t)i, cur + 3 * (size_t)i, 12);
            if (e == s || (fix_boundary && boundary[i])) continue;
            double acc[4];
            row_sums(cur, neighbours, i, s, e, method == SLS_SMOOTH_SIMPLE ? SLS_SMOOTH_UNIFORM : weights, acc);
            if (method == SLS_SMOOTH_SIMPLE) sls_smooth_simple(cur + 3 * (size_t)i, acc, (uint32_t)(e - s), nxt + 3 * (size_t)i);
            else sls_smooth_step(cur + 3 * (size_t)i, acc, f, nxt + 3 * (size_t)i);
        }
        float *t = cur; cur = nxt; nxt = t;
    }
    memcpy(out, cur, sizeof(float) * 3 * (size_t)V);
    free(offsets); free(neighbours); free(boundary); free(cur); free(nxt);
}
'''


class Host:
    """include/sls_smooth_math.h compiled as plain C and called through ctypes."""

    def __init__(self, lib):
        self.lib = lib
        lib.ref_adjacency.restype = None
        lib.ref_adjacency.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
        lib.ref_smooth.restype = None
        lib.ref_smooth.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                   C.c_void_p, C.c_void_p]

    def adjacency(self, faces, V):
        """(offsets (V+1,), neighbours (2E,), boundary (V,), status: 8 words)"""
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        offsets, nbr = np.zeros((V + 1,), np.int32), np.zeros((6 * len(f) + 1,), np.int32)
        boundary, status = np.zeros((V + 1,), np.uint8), np.zeros((8,), np.uint32)
        self.lib.ref_adjacency(V, len(f), f.ctypes.data, None, offsets.ctypes.data, nbr.ctypes.data, boundary.ctypes.data, status.ctypes.data)
        return offsets.astype(np.int64), nbr[:2 * int(status[1])].astype(np.int64), boundary[:V], [int(x) for x in status]

    def smooth(self, vertices, faces, iterations, method=TAUBIN, weights=INVERSE_DISTANCE, lam=LAMBDA, mu=MU, fix_boundary=False):
        """(vertices' (V,3) float32, status: 8 words)"""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        out, status = np.zeros((max(len(v), 1), 3), np.float32), np.zeros((8,), np.uint32)
        self.lib.ref_smooth(len(v), v.ctypes.data, len(f), f.ctypes.data, int(method), int(weights), int(iterations), float(lam), float(mu),
                            int(bool(fix_boundary)), out.ctypes.data, status.ctypes.data)
        return out[:len(v)], [int(x) for x in status]


_KEEP = []


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="smooth_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "smooth_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libsmooth_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- the case table --------------------------------------------------------------------------------------------------
def _f32(points):
    return np.asarray(points, dtype=np.float32).reshape(-1, 3)


def _i32(faces):
    return np.asarray(faces, dtype=np.int32).reshape(-1, 3)


SHEET_Z = 0.3
SHEET_N = 5


def sheet(noise=0.0, seed=3):
    """a SHEET_N x SHEET_N sheet of points 0.25 apart in the plane z = SHEET_Z (x, y irregular by a seeded quarter of the
    spacing, so that the inverse-distance weights differ), two triangles per square; `noise`: seeded z-noise of that size"""
    rng = np.random.default_rng(seed)
    n = SHEET_N
    xy = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="xy"), 2).reshape(-1, 2) * 0.25 + rng.uniform(-0.06, 0.06, (n * n, 2))
    z = SHEET_Z + noise * rng.uniform(-1.0, 1.0, (n * n,))
    quads = [(n * y + x, n * y + x + 1, n * y + x + n + 1, n * y + x + n) for y in range(n - 1) for x in range(n - 1)]
    return _f32(np.concatenate([xy, z[:, None]], 1)), _i32([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def sheet_border():
    n = SHEET_N
    return np.array([y * n + x for y in range(n) for x in range(n) if x in (0, n - 1) or y in (0, n - 1)])


def fan(n, seed=11):
    """a closed fan: hub 0 with exactly n neighbours on a seeded irregular ring"""
    rng = np.random.default_rng(seed + n)
    ang = 2 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    r = rng.uniform(0.7, 1.3, n)
    ring = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-0.2, 0.2, n)], 1)
    v = np.concatenate([[[0.05, -0.03, 0.4]], ring])
    return _f32(v), _i32([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)])


@functools.lru_cache(maxsize=None)
def sphere(noise=0.0, seed=7):
    """the welded marching-tetrahedra unit sphere of tsdf_ref (3578 vertices, 7152 triangles) with seeded radial noise of
    that size (uniform in [-noise, noise]): (V,3) float32, (T,3) int32, read-only"""
    v, index = mesh_ref.weld(mesh_ref.sphere_soup())
    f = index.reshape(-1, 3).astype(np.int32)
    d = v.astype(np.float64) - mesh_ref.tsdf_ref.CENTRE
    r = np.linalg.norm(d, axis=1, keepdims=True)
    v = (mesh_ref.tsdf_ref.CENTRE + d / r * (r + noise * np.random.default_rng(seed).uniform(-1.0, 1.0, r.shape))).astype(np.float32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def radii(v):
    return np.linalg.norm(np.asarray(v, dtype=np.float64) - mesh_ref.tsdf_ref.CENTRE, axis=1)


SPHERE_NOISE = 0.02
STRIPS = (341, 342, 682, 683)   # 6 T = 2046, 2052, 4092, 4098 directed pairs: either side of one and of two chunks of 2048 positions


def strip(T, seed=13):
    """an open strip of T triangles of one orientation over T + 2 vertices on two seeded irregular rows 0.25 apart: every
    vertex lies on the rim, 6 T directed pairs with 2 (2 T + 1) heads"""
    rng = np.random.default_rng(seed + T)
    i = np.arange(T + 2)
    v = np.stack([0.125 * i, 0.25 * (i % 2), np.zeros(T + 2)], 1) + rng.uniform(-0.05, 0.05, (T + 2, 3))
    t = np.arange(T)
    return _f32(v), _i32(np.stack([np.where(t % 2 == 0, t, t + 1), np.where(t % 2 == 0, t + 1, t), t + 2], 1))


def cases():
    """name -> (vertices (V,3) float32, faces (T,3) int32)"""
    nan = np.float32(np.nan)
    tet_v = [(0, 0, 0), (1, 0.1, 0), (0.2, 1, 0.1), (0.3, 0.2, 1)]
    tri_v = [(0, 0, 0), (1, 0.25, 0), (0.25, 1, 0.5)]
    five = [(0, 0, 0), (1, 0, 0.1), (0.5, 1, 0), (0.5, -1, 0.3), (0.5, 0.1, 1.2)]
    out = {}
    out["tetrahedron"] = (_f32(tet_v), _i32([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)]))                # closed, rows of 3
    out["triangle"] = (_f32(tri_v), _i32([(0, 1, 2)]))                                                   # all boundary
    out["sheet"] = sheet()
    out["sheet_noisy"] = sheet(0.05)
    for n in (64, 65, 100):                                                                             # the long-row switch and its tail
        out[f"fan_{n}"] = fan(n)
    out["three_on_edge"] = (_f32(five), _i32([(0, 1, 2), (1, 0, 3), (0, 1, 4)]))
    out["repeated"] = (_f32(five), _i32([(0, 1, 2), (0, 1, 2), (2, 1, 0), (0, 3, 1)]))                    # twice, and the opposite orientation
    # equal, negative and >= V indices, rows of -1, between good triangles
    out["bad_indices"] = (_f32(five), _i32([(0, 1, 2), (3, 3, 4), (-1, 0, 1), (0, 5, 1), (-1, -1, -1), (1, 0, 3), (4, 2, 4), (-1, -1, -1)]))
    # unreferenced vertices in the middle (1, 3) and at the end (7, 8); vertex 3 holds -0.0 and must be copied by bits
    out["unreferenced"] = (_f32([(0, 0, 0), (9, 9, 9), (1, 0, 0.2), (-0.0, -0.0, -0.0), (0, 1, 0.1), (1, 1.1, 0), (0.4, 0.5, 1), (5, 5, 5), (nan, 0, 0)]),
                           _i32([(0, 2, 4), (2, 5, 4), (0, 6, 2), (3, 3, 1)]))
    # two coincident vertices joined by an edge: d = 0, weight 1e12
    out["coincident"] = (_f32([(0, 0, 0), (1, 0, 0), (1, 0, 0), (0.5, 1, 0.2), (0.5, -1, 0.1)]), _i32([(0, 1, 3), (1, 2, 3), (0, 4, 1), (1, 4, 2)]))
    out["nan_live"] = (_f32([(0, 0, 0), (1, 0, 0), (nan, 1, 0), (1, 1, 0.5)]), _i32([(0, 1, 2), (1, 3, 2)]))
    out["sphere_noisy"] = sphere(SPHERE_NOISE)
    for T in STRIPS:                                                                                    # the edges of the scan's chunks
        out[f"strip_{T}"] = strip(T)
    out["no_vertices"] = (_f32([]), _i32([]))
    out["no_faces"] = (_f32(tet_v), _i32([]))
    return out


UNSPECIFIED = ("nan_live",)         # a live non-finite vertex: counted, the positions unspecified


def settings():
    """(method, weights, fix_boundary, iterations): methods x weights x fix_boundary, 1 / 2 / 5 iterations (1 / 2 for Taubin:
    2 and 4 steps; Laplacian and simple give both parities of the step count), and no iteration at all once per method"""
    out = []
    for method in (SIMPLE, LAPLACIAN, TAUBIN):
        for weights in (UNIFORM, INVERSE_DISTANCE):
            for fix in (False, True):
                out += [(method, weights, fix, n) for n in ((1, 2) if method == TAUBIN else (1, 2, 5))]
        out.append((method, INVERSE_DISTANCE, False, 0))
    return out
