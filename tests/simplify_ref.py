"""Mesh simplification by vertex clustering (sls_mesh_simplify) restated in NumPy and pure Python — rules 1 to 5 of
include/sls_simplify_math.h, the float64 operations in the header's order, every sum in the stated order — and that header
compiled as plain C and run on the host (`host()`), plus the case table the simplification tests share."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import mesh_ref

ROOT = mesh_ref.ROOT
LONG = 64                       # SLS_SIMPLIFY_LONG
LIMIT = 1 << 21                 # SLS_VOXEL_INDEX_LIMIT
AVERAGE, QUADRIC = 0, 1
STATUS = ("vertices", "triangles", "nonfinite", "out_of_grid", "collapsed", "duplicates", "fallbacks")


# ---- the restatement -------------------------------------------------------------------------------------------------
def segment_sum(items):
    """(n, N) float64 -> (N,): n <= 64 items one after the other from +0.0; more: 64 lanes, then the xor butterfly."""
    items = np.asarray(items, dtype=np.float64)
    n = len(items)
    if n <= LONG:
        acc = np.zeros(items.shape[1:])
        for row in items:
            acc = acc + row
        return acc
    part = np.zeros((LONG,) + items.shape[1:])
    for i0 in range(0, n, LONG):                                    # lane l adds l, l + 64, ... in that order
        rows = items[i0:i0 + LONG]
        part[:len(rows)] = part[:len(rows)] + rows
    lanes = np.arange(LONG)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ off]
    return part[0]


def clusters(vertices, faces, voxel_size):
    """(cid (V,) int64, -1 without a cluster; keys of the clusters; non-finite live count; out-of-grid count; degenerate (T,)
    bool INCLUDING the triangles with a non-finite vertex)"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    deg = mesh_ref.degenerate(f, V) != 0
    live = np.zeros((V,), bool)
    live[f[~deg].reshape(-1)] = True
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(v).all(1)
    ok = live & finite
    cid = np.full((V,), -1, np.int64)
    keys, big = np.zeros((0,), np.uint64), 0
    if ok.any():
        p = v[ok]
        origin = p.min(0).astype(np.float64) - 0.5 * voxel_size
        idx = np.floor((p.astype(np.float64) - origin) / voxel_size)
        inside = ((idx >= 0) & (idx < LIMIT)).all(1)
        big = int((~inside).sum())
        i = np.where(inside[:, None], idx, 0).astype(np.uint64)
        key = i[:, 0] | (i[:, 1] << np.uint64(21)) | (i[:, 2] << np.uint64(42))
        keys, inv = np.unique(key, return_inverse=True)
        cid[ok] = inv.reshape(-1)
    if len(f):
        deg = deg | (np.where(deg[:, None], 0, cid[np.where(deg[:, None], 0, f)]) < 0).any(1)
    return cid, keys, int((live & ~finite).sum()), big, deg


def rotate(c):
    """(n,3) distinct triples with the smallest entry first, the cyclic order kept"""
    k = np.argmin(c, axis=1)
    cols = (k[:, None] + np.arange(3)[None]) % 3
    return np.take_along_axis(c, cols, axis=1)


def quadrics(v, f):
    """(n, 9) float64 per triangle of f (all indices valid, all vertices finite) and (n,) bool: contributes"""
    p0, p1, p2 = (v[f[:, k]].astype(np.float64) for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(all="ignore"):
        L = np.sqrt((cx * cx + cy * cy) + cz * cz)
        has = (L > 0) & np.isfinite(L)
        Ls = np.where(has, L, 1.0)
        nx, ny, nz = cx / Ls, cy / Ls, cz / Ls
        w = 0.5 * Ls
        s = (nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2]
        wx, wy, wz, ws = w * nx, w * ny, w * nz, w * s
        q = np.stack([wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, ws * nx, ws * ny, ws * nz], 1)
    return q, has


def solve(q, m, lam, voxel_size):
    """sls_simplify_solve in Python floats (IEEE float64, one rounding per operation): ((3,) float32, fell back)"""
    q = [float(x) for x in q]
    m = [float(x) for x in m]
    mean = np.array(m, dtype=np.float64).astype(np.float32)
    tr = (q[0] + q[3]) + q[5]
    if not tr > 0.0:
        return mean, True
    reg = lam * tr
    m00, m11, m22, m01, m02, m12 = q[0] + reg, q[3] + reg, q[5] + reg, q[1], q[2], q[4]
    rx = q[6] - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2])
    ry = q[7] - ((q[1] * m[0] + q[3] * m[1]) + q[4] * m[2])
    rz = q[8] - ((q[2] * m[0] + q[4] * m[1]) + q[5] * m[2])
    c00 = m11 * m22 - m12 * m12
    c01 = m02 * m12 - m01 * m22
    c02 = m01 * m12 - m02 * m11
    c11 = m00 * m22 - m02 * m02
    c12 = m01 * m02 - m00 * m12
    c22 = m00 * m11 - m01 * m01
    det = (m00 * c00 + m01 * c01) + m02 * c02
    if not det > 0.0:
        return mean, True
    d = (((c00 * rx + c01 * ry) + c02 * rz) / det, ((c01 * rx + c11 * ry) + c12 * rz) / det, ((c02 * rx + c12 * ry) + c22 * rz) / det)
    if not all(abs(x) <= voxel_size for x in d):
        return mean, True
    return np.array([m[0] + d[0], m[1] + d[1], m[2] + d[2]], dtype=np.float64).astype(np.float32), False


def simplify(vertices, faces, voxel_size, contraction=AVERAGE, regularisation=1e-3):
    """(vertices' (V',3) float32, faces' (T',3) int64, vmap (V,) int64, dict of the status words + degenerate)"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, T = len(v), len(f)
    cid, keys, nonfinite, big, deg = clusters(v, f, voxel_size)
    c = cid[np.where(deg[:, None], 0, f)] if T and V else np.zeros((T, 3), np.int64)
    distinct = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 2] != c[:, 0])
    cand = ~deg & distinct
    collapsed = int((~deg & ~distinct).sum())
    kept, seen, rows = np.zeros((T,), bool), set(), rotate(c[cand]) if cand.any() else np.zeros((0, 3), np.int64)
    for t, row in zip(np.nonzero(cand)[0], map(tuple, rows.tolist())):          # input order: the lowest index stays
        if row not in seen:
            seen.add(row)
            kept[t] = True
    duplicates = int(cand.sum() - kept.sum())
    rf = np.zeros((T, 3), np.int64)
    rf[cand] = rows
    survives = np.zeros((len(keys),), bool)
    survives[rf[kept].reshape(-1)] = True
    cnew = np.cumsum(survives) - 1
    vmap = np.where((cid >= 0) & survives[np.maximum(cid, 0)] if len(keys) else np.zeros((V,), bool), cnew[np.maximum(cid, 0)] if len(keys) else -1, -1)
    out_v = np.zeros((int(survives.sum()), 3), np.float32)
    order = np.argsort(cid, kind="stable")                          # a cluster's vertices in ascending index
    starts = np.searchsorted(cid[order], np.arange(len(keys) + 1))
    fallbacks = 0
    if contraction == QUADRIC:
        adds = ~deg
        q, has = quadrics(v, f[adds])
        corner_c = c[adds].reshape(-1)                              # corner 3 t + k in ascending corner id
        q3, has3 = np.repeat(q, 3, axis=0), np.repeat(has, 3)
        corder = np.argsort(corner_c, kind="stable")
        cstarts = np.searchsorted(corner_c[corder], np.arange(len(keys) + 1))
    for k in np.nonzero(survives)[0]:
        members = order[starts[k]:starts[k + 1]]
        m = segment_sum(v[members].astype(np.float64)) / float(len(members))
        pos = m.astype(np.float32)
        if contraction == QUADRIC:
            run = corder[cstarts[k]:cstarts[k + 1]]
            items = np.where(has3[run][:, None], q3[run], 0.0)      # (adding +0.0 changes no bit of a sum that starts at +0.0)
            pos, fell = solve(segment_sum(items) if len(run) else np.zeros((9,)), m, regularisation, voxel_size)
            fallbacks += int(fell)
        out_v[cnew[k]] = pos
    stats = dict(zip(STATUS, (len(out_v), int(kept.sum()), nonfinite, big, collapsed, duplicates, fallbacks)), degenerate=int(deg.sum()))
    return out_v, cnew[rf[kept]].reshape(-1, 3), vmap.astype(np.int64), stats


# ---- the header on the host ------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "sls_simplify_math.h"

typedef struct { uint64_t key; uint32_t id; } KV;
static int cmp_kv(const void *pa, const void *pb)
{
    const KV *a = (const KV *)pa, *b = (const KV *)pb;
    if (a->key != b->key) return a->key < b->key ? -1 : 1;
    return a->id < b->id ? -1 : (a->id > b->id ? 1 : 0);
}
typedef struct { int32_t r[3]; uint32_t t; } Tri;
static int cmp_tri(const void *pa, const void *pb)
{
    const Tri *a = (const Tri *)pa, *b = (const Tri *)pb;
    for (int k = 0; k < 3; ++k) if (a->r[k] != b->r[k]) return a->r[k] < b->r[k] ? -1 : 1;
    return a->t < b->t ? -1 : (a->t > b->t ? 1 : 0);
}

/* "the order of every float64 sum": n items of N words, has[i] = 0: item i adds nothing */
static void segment_sum(int n, int N, const double *items, const uint8_t *has, double *acc)
{
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if (n <= SLS_SIMPLIFY_LONG) {
        for (int i = 0; i < n; ++i)
            if (!has || has[i]) for (int k = 0; k < N; ++k) acc[k] += items[(size_t)i * N + k];
        return;
    }
    double part[64][9], next[64][9];
    memset(part, 0, sizeof(part));
    for (int i = 0; i < n; ++i)
        if (!has || has[i]) for (int k = 0; k < N; ++k) part[i % 64][k] += items[(size_t)i * N + k];
    for (int off = 32; off > 0; off >>= 1) {
        for (int l = 0; l < 64; ++l) for (int k = 0; k < N; ++k) next[l][k] = part[l][k] + part[l ^ off][k];
        memcpy(part, next, sizeof(part));
    }
    for (int k = 0; k < N; ++k) acc[k] = part[0][k];
}

static int finite3(const float *p) { return sls_simplify_finite(p[0]) && sls_simplify_finite(p[1]) && sls_simplify_finite(p[2]); }

/* status: 8 words; out_vertices: room for V rows, out_faces: room for T rows, vmap: V */
void ref_simplify(int V, const float *xyz, int T, const int32_t *faces, double h, int contraction, double lambda,
                  float *out_vertices, int32_t *out_faces, int32_t *vmap, uint32_t *status)
{
    memset(status, 0, 8 * sizeof(uint32_t));
    status[7] = 1u;
    for (int v = 0; v < V; ++v) vmap[v] = -1;
    if (V == 0 || T == 0) return;
    uint8_t *live = (uint8_t *)calloc((size_t)V, 1);
    int32_t *cid = (int32_t *)malloc(sizeof(int32_t) * (size_t)V);
    KV *vk = (KV *)malloc(sizeof(KV) * (size_t)V);
    uint32_t *seg = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)V + 1));
    for (int t = 0; t < T; ++t)
        if (!sls_mesh_degenerate(faces + 3 * (size_t)t, V)) for (int k = 0; k < 3; ++k) live[faces[3 * (size_t)t + k]] = 1;
    float mn[3] = { INFINITY, INFINITY, INFINITY };
    for (int v = 0; v < V; ++v) {
        if (!live[v]) continue;
        if (finite3(xyz + 3 * (size_t)v)) { for (int a = 0; a < 3; ++a) mn[a] = fminf(mn[a], xyz[3 * (size_t)v + a]); }
        else status[2]++;
    }
    int nl = 0;                                                    /* the finite live vertices, to be sorted by key */
    for (int v = 0; v < V; ++v) {
        cid[v] = -1;
        if (!live[v] || !finite3(xyz + 3 * (size_t)v)) continue;
        uint64_t key;
        if (!sls_voxel_key(xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2], sls_voxel_origin(mn[0], h),
                           sls_voxel_origin(mn[1], h), sls_voxel_origin(mn[2], h), h, &key)) status[3]++;
        vk[nl].key = key; vk[nl].id = (uint32_t)v; ++nl;
    }
    qsort(vk, (size_t)nl, sizeof(KV), cmp_kv);
    int nc = 0;
    for (int j = 0; j < nl; ++j) {
        if (j == 0 || vk[j].key != vk[j - 1].key) seg[nc++] = (uint32_t)j;
        cid[vk[j].id] = nc - 1;
    }
    seg[nc] = (uint32_t)nl;

    Tri *tri = (Tri *)malloc(sizeof(Tri) * (size_t)T);
    uint8_t *kept = (uint8_t *)calloc((size_t)T, 1), *adds = (uint8_t *)calloc((size_t)T, 1);
    int32_t *rf = (int32_t *)malloc(3 * sizeof(int32_t) * (size_t)T);
    int nt = 0;
    for (int t = 0; t < T; ++t) {
        const int32_t *f = faces + 3 * (size_t)t;
        if (sls_mesh_degenerate(f, V)) continue;
        const int32_t c[3] = { cid[f[0]], cid[f[1]], cid[f[2]] };
        if (c[0] < 0 || c[1] < 0 || c[2] < 0) continue;            /* a non-finite vertex: treated as degenerate */
        adds[t] = 1;
        if (sls_simplify_rotate(c, tri[nt].r)) { status[4]++; continue; }
        memcpy(rf + 3 * (size_t)t, tri[nt].r, 12);
        tri[nt].t = (uint32_t)t; ++nt;
    }
    qsort(tri, (size_t)nt, sizeof(Tri), cmp_tri);
    uint8_t *surv = (uint8_t *)calloc((size_t)nc + 1, 1);
    int32_t *cnew = (int32_t *)malloc(sizeof(int32_t) * ((size_t)nc + 1));
    for (int j = 0; j < nt; ++j) {
        if (j > 0 && !memcmp(tri[j].r, tri[j - 1].r, 12)) { status[5]++; continue; }
        kept[tri[j].t] = 1;
        for (int k = 0; k < 3; ++k) surv[tri[j].r[k]] = 1;
    }
    int nv = 0, nf = 0;
    for (int c = 0; c < nc; ++c) cnew[c] = surv[c] ? nv++ : -1;
    for (int t = 0; t < T; ++t)
        if (kept[t]) { for (int k = 0; k < 3; ++k) out_faces[3 * (size_t)nf + k] = cnew[rf[3 * (size_t)t + k]]; ++nf; }
    for (int v = 0; v < V; ++v) vmap[v] = cid[v] >= 0 ? cnew[cid[v]] : -1;
    status[0] = (uint32_t)nv; status[1] = (uint32_t)nf;

    KV *ck = NULL;
    uint32_t *cseg = NULL;
    int ncorn = 0;
    if (contraction == 1) {                                        /* the contributing corners, sorted by cluster */
        ck = (KV *)malloc(sizeof(KV) * (3 * (size_t)T + 1));
        cseg = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)nc + 2));
        for (int t = 0; t < T; ++t)
            if (adds[t]) for (int k = 0; k < 3; ++k) { ck[ncorn].key = (uint64_t)cid[faces[3 * (size_t)t + k]]; ck[ncorn].id = (uint32_t)(3 * t + k); ++ncorn; }
        qsort(ck, (size_t)ncorn, sizeof(KV), cmp_kv);
        int j = 0;
        for (int c = 0; c <= nc; ++c) { while (j < ncorn && ck[j].key < (uint64_t)c) ++j; cseg[c] = (uint32_t)j; }
    }
    for (int c = 0; c < nc; ++c) {
        if (!surv[c]) continue;
        const int n = (int)(seg[c + 1] - seg[c]);
        double *items = (double *)malloc(sizeof(double) * 3 * (size_t)n), m[3];
        for (int i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) items[3 * (size_t)i + a] = (double)xyz[3 * (size_t)vk[seg[c] + i].id + a];
        segment_sum(n, 3, items, NULL, m);
        free(items);
        float out[3];
        for (int a = 0; a < 3; ++a) { m[a] = sls_simplify_mean(m[a], (uint32_t)n); out[a] = (float)m[a]; }
        if (contraction == 1) {
            const int nq = (int)(cseg[c + 1] - cseg[c]);
            double *q = (double *)calloc(9 * (size_t)(nq ? nq : 1), sizeof(double)), sum[9];
            uint8_t *has = (uint8_t *)calloc((size_t)(nq ? nq : 1), 1);
            for (int i = 0; i < nq; ++i) {
                const int32_t *f = faces + 3 * (size_t)(ck[cseg[c] + i].id / 3u);
                has[i] = (uint8_t)sls_simplify_quadric(xyz + 3 * (size_t)f[0], xyz + 3 * (size_t)f[1], xyz + 3 * (size_t)f[2], q + 9 * (size_t)i);
            }
            segment_sum(nq, 9, q, has, sum);
            status[6] += (uint32_t)sls_simplify_solve(sum, m, lambda, h, out);
            free(q); free(has);
        }
        memcpy(out_vertices + 3 * (size_t)cnew[c], out, 12);
    }
    free(live); free(cid); free(vk); free(seg); free(tri); free(kept); free(adds); free(rf); free(surv); free(cnew); free(ck); free(cseg);
}
'''


class Host:
    """include/sls_simplify_math.h compiled as plain C and called through ctypes."""

    def __init__(self, lib):
        self.lib = lib
        lib.ref_simplify.restype = None
        lib.ref_simplify.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_double] + [C.c_void_p] * 4

    def simplify(self, vertices, faces, voxel_size, contraction=AVERAGE, regularisation=1e-3):
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        out_v, out_f = np.zeros((max(len(v), 1), 3), np.float32), np.zeros((max(len(f), 1), 3), np.int32)
        vmap, status = np.zeros((max(len(v), 1),), np.int32), np.zeros((8,), np.uint32)
        self.lib.ref_simplify(len(v), v.ctypes.data, len(f), f.ctypes.data, float(voxel_size), int(contraction), float(regularisation),
                              out_v.ctypes.data, out_f.ctypes.data, vmap.ctypes.data, status.ctypes.data)
        return out_v[:int(status[0])], out_f[:int(status[1])].astype(np.int64), vmap[:len(v)].astype(np.int64), [int(x) for x in status]


_KEEP = []


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="simplify_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "simplify_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libsimplify_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


def status_words(stats):
    return [stats[k] for k in STATUS] + [1]


# ---- the case table --------------------------------------------------------------------------------------------------
# One workgroup's share of every chunked pass: the sorter takes 1024 items per wave and 4096 per workgroup (11-bit digits),
# the head / compaction scans take 2048 positions (SimpChunks::kChunk); a segment of more than 64 items is summed by 64 lanes.
CHUNKS = {"sort_wave": 1024, "scan": 2048, "sort_workgroup": 4096}
SIZED = sorted({n + d for n in CHUNKS.values() for d in (-1, 0, 1)} | {n + d - 2 for n in CHUNKS.values() for d in (-1, 0, 1)})


def strip(n, seed=5):
    """n triangles (i, i + 1, i + 2) in a seeded random order over n + 2 DISTINCT lattice vertices (multiples of 1/16, magnitude
    <= 64): T = n, n + 2 live vertices.  Two rows 4 apart, columns 17/16 apart, folded every 48 columns into layers 3/16
    apart: at voxel_size 1 a cluster holds the same column of about five layers (kept triangles, and duplicates from layer
    to layer), at 4 about eighty vertices (long segments).  Every mean over such points is exact in any order."""
    i = np.arange(n + 2)
    col = i // 2
    v = np.stack([(col % 48) * (17 / 16.0) - 16.0, (i % 2) * 4.0, (col // 48) * (3 / 16.0) + 3.0], 1).astype(np.float32)
    f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)
    return v, f[np.random.default_rng(seed + n).permutation(n)]


@functools.lru_cache(maxsize=None)
def cube(cells=24):
    """the surface of the unit cube, `cells` squares per edge, two triangles per square, outward: (V,3) float32, (T,3) int32"""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]
    for axis in range(3):
        for side in (0, cells):
            for a in range(cells):
                for b in range(cells):
                    quad = []
                    for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, a + da, b + db
                        quad.append(vid(tuple(p)))
                    if side == 0:
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    v = (np.asarray(verts, dtype=np.float64) / cells).astype(np.float32)
    f = np.asarray(faces, dtype=np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def cube_distance(p):
    """the distance of every point from the surface of the unit cube, float64"""
    p = np.asarray(p, dtype=np.float64)
    outside = np.linalg.norm(np.maximum(np.maximum(-p, p - 1.0), 0.0), axis=1)
    inside = np.minimum(p, 1.0 - p).min(1)
    return np.where(outside > 0, outside, inside)


SPHERE_CENTRE = (0.3, -0.2, 0.1)


@functools.lru_cache(maxsize=None)
def sphere(n_lat=96, n_lon=192, centre=SPHERE_CENTRE):
    """a latitude-longitude unit sphere: n_lat bands, n_lon sectors, fans at the poles — 36 480 triangles for 96 x 192"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None]], 2)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) + np.asarray(centre)
    faces = []
    south = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        k = (j + 1) % n_lon
        faces.append((0, 1 + j, 1 + k))
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
            faces += [(a + j, b + j, b + k), (a + j, b + k, a + k)]
        faces.append((south, south - n_lon + k, south - n_lon + j))
    v, f = v.astype(np.float32), np.asarray(faces, dtype=np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def _grid(points):
    return np.asarray(points, dtype=np.float32)


def hand_cases():
    """name -> (vertices, faces, voxel_size): at most 20 triangles each"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # a 4 x 4 sheet of points one voxel apart, and satellites a quarter of a voxel from some of them
    sheet = [(x, y, 0.25 * ((x + y) % 2)) for y in range(4) for x in range(4)]
    quads = [(4 * y + x, 4 * y + x + 1, 4 * y + x + 5, 4 * y + x + 4) for y in range(3) for x in range(3)]
    sheet_f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    cases = {}
    # a triangle collapsing to a point (16, 17, 18 all next to point 5) and one collapsing to an edge (5, 16, 6)
    v = sheet + [(1.2, 1.1, 0.3), (1.1, 1.25, 0.2), (1.25, 1.2, 0.35)]
    cases["collapse"] = (_grid(v), np.array(sheet_f + [(16, 17, 18), (5, 16, 6)], np.int32), 1.0)
    # the same cluster triple twice (the lower index stays), once more reversed (stays), once more rotated (a duplicate)
    v = sheet + [(0.1, 0.1, 0.05), (1.1, 0.1, 0.3), (1.1, 1.1, 0.05)]
    cases["duplicates"] = (_grid(v), np.array([(16, 17, 18), (0, 1, 5), (5, 1, 0), (1, 5, 0)] + sheet_f[2:], np.int32), 1.0)
    # an index of -1, one >= V, two equal indices, an unreferenced vertex far away and one referenced by degenerate rows alone
    v = sheet + [(-1000.0, -2000.0, 500.0), (-50.0, 3.0, 3.0)]
    cases["bad_indices"] = (_grid(v), np.array(sheet_f + [(-1, 0, 1), (0, 18, 1), (2, 2, 17), (17, 3, 17)], np.int32), 1.0)
    # a referenced NaN / inf vertex (counted, its triangles leave) and an unreferenced one (ignored)
    v = sheet + [(nan, 0.0, 0.0), (inf, 1.0, 1.0), (1.0, -inf, 2.0)]
    cases["nonfinite"] = (_grid(v), np.array(sheet_f + [(0, 1, 16), (16, 5, 4), (17, 17, 2), (18, 2, 3)], np.int32), 1.0)
    # a far cluster pair whose only triangles collapse: both clusters vanish
    v = sheet + [(9.1, 9.1, 0.0), (9.2, 9.3, 0.1), (9.3, 9.1, 0.2), (10.2, 9.2, 0.0)]
    cases["vanish"] = (_grid(v), np.array(sheet_f + [(16, 17, 18), (16, 17, 19), (19, 18, 17)], np.int32), 1.0)
    # zero-area triangles: three collinear clusters (kept, no quadric: a fallback) next to the sheet
    v = sheet + [(6.0, 0.0, 0.0), (7.0, 0.0, 0.0), (8.0, 0.0, 0.0), (6.1, 0.0, 0.0)]
    cases["zero_area"] = (_grid(v), np.array(sheet_f + [(16, 17, 18), (19, 18, 17), (16, 19, 17)], np.int32), 1.0)
    cases["empty"] = (_grid(sheet), np.zeros((0, 3), np.int32), 1.0)
    cases["one_voxel"] = (_grid(sheet), np.array(sheet_f, np.int32), 100.0)     # everything collapses
    return cases


def big_case():
    """a vertex whose voxel index reaches 2^21: counted, the outputs unspecified"""
    v = _grid([(0, 0, 0), (1, 0, 0), (0, 1, 0), (float(LIMIT), 0, 0), (float(LIMIT), 1, 0)])
    return v, np.array([(0, 1, 2), (1, 3, 2), (3, 4, 2)], np.int32), 1.0


def cases():
    """name -> (vertices, faces, voxel_size); the strip cases hold lattice points only"""
    out = dict(hand_cases())
    for n in SIZED:
        v, f = strip(n)
        out[f"strip_{n}"] = (v, f, 1.0)
    v, f = strip(CHUNKS["scan"] + 1)
    out["strip_identity"] = (v, f, 1.0 / 32.0)
    out["strip_long"] = strip(CHUNKS["sort_workgroup"] + 1) + (4.0,)
    for h in (1.0 / 6.0, 0.21, 0.5):
        out[f"cube_{h:.3f}"] = cube() + (h,)
    out["sphere"] = sphere() + (0.1,)
    return out


LATTICE = lambda name: name.startswith("strip")                     # noqa: E731
