"""The mesh cleaning stage (sls_mesh_weld, sls_mesh_clusters, sls_mesh_filter, sls_mesh_vertex_normals) restated in
NumPy and pure Python — np.unique on the int32 view, a breadth-first walk, the selection rule, float64 normals — and
include/sls_mesh_math.h compiled as plain C and run on the host (`host()`), plus the inputs the mesh tests share."""
import collections
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import tsdf_ref

ROOT = tsdf_ref.ROOT


# ---- the restatement -------------------------------------------------------------------------------------------------
def weld(rows):
    """(vertices (V,3) float32, index (N,) int64): unique rows in signed-int32 lexicographic order, the rank of every row."""
    bits = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 3).view(np.int32)
    if len(bits) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0,), np.int64)
    uniq, inv = np.unique(bits, axis=0, return_inverse=True)
    return uniq.view(np.float32), inv.reshape(-1).astype(np.int64)


def degenerate(faces, V):
    """(T,) 0: fine, 1: a repeated index, 2: an index outside [0, V)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    outside = ((f < 0) | (f >= V)).any(1)
    repeated = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    return np.where(outside, 2, np.where(repeated, 1, 0))


def clusters(faces, V):
    """(labels (T,) int64, counts (C,) int64, dict(clusters, degenerate, out_of_range, boundary_edges, nonmanifold_edges)):
    a breadth-first walk from triangle 0 upward over the shared-edge adjacency."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    T = len(f)
    deg = degenerate(f, V)
    owners = collections.defaultdict(list)
    for t in range(T):
        if deg[t]:
            continue
        for e in range(3):
            a, b = int(f[t, e]), int(f[t, (e + 1) % 3])
            owners[(min(a, b), max(a, b))].append(t)
    labels = np.full((T,), -1, np.int64)
    counts = []
    for seed in range(T):
        if deg[seed] or labels[seed] >= 0:
            continue
        c = len(counts)
        labels[seed] = c
        queue, n = collections.deque([seed]), 0
        while queue:
            t = queue.popleft()
            n += 1
            for e in range(3):
                a, b = int(f[t, e]), int(f[t, (e + 1) % 3])
                for u in owners[(min(a, b), max(a, b))]:
                    if labels[u] < 0:
                        labels[u] = c
                        queue.append(u)
        counts.append(n)
    stats = {"clusters": len(counts), "degenerate": int((deg != 0).sum()), "out_of_range": int((deg == 2).sum()),
             "boundary_edges": sum(1 for o in owners.values() if len(o) == 1),
             "nonmanifold_edges": sum(1 for o in owners.values() if len(o) > 2)}
    return labels, np.asarray(counts, dtype=np.int64), stats


def n_min(counts, keep_clusters, min_triangles):
    C_ = len(counts)
    k = min(keep_clusters, C_) if keep_clusters > 0 else 0
    kth = int(np.sort(np.asarray(counts))[::-1][k - 1]) if k > 0 else 0
    return max(max(int(min_triangles), 0), kth)


def select(vertices, faces, keep_clusters, min_triangles):
    """(vertices', faces' int64, n_min) by the selection rule."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    labels, counts, _ = clusters(f, len(v))
    nm = n_min(counts, keep_clusters, min_triangles)
    kept = np.zeros((len(f),), bool)
    ok = labels >= 0
    kept[ok] = counts[labels[ok]] >= nm
    fk = f[kept]
    used = np.zeros((len(v),), bool)
    used[fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return v[used], remap[fk].reshape(-1, 3), nm


def normals64(vertices, faces):
    """(V,3) float64: the normalised sum of the un-normalised face normals over the non-degenerate triangles; zeros where
    there is none or the sum vanishes.  Also the conditioning |sum n| / sum |n| per vertex (1 where there is none)."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[degenerate(f, len(v)) == 0]
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    s, mag = np.zeros_like(v), np.zeros((len(v),))
    for c in range(3):
        np.add.at(s, f[:, c], fn)
        np.add.at(mag, f[:, c], np.linalg.norm(fn, axis=1))
    length = np.linalg.norm(s, axis=1)
    good = np.isfinite(length) & (length > 0)
    out = np.zeros_like(v)
    out[good] = s[good] / length[good, None]
    return out, np.where(mag > 0, length / np.where(mag > 0, mag, 1.0), 1.0)


def clean(vertices, faces, keep_clusters=1, min_triangles=50):
    """weld + select + float64 normals of a mesh: (vertices, faces int64, normals float64)."""
    v, index = weld(vertices)
    f = index[np.asarray(faces, dtype=np.int64).reshape(-1)].reshape(-1, 3)
    v, f, _ = select(v, f, keep_clusters, min_triangles)
    return v, f, normals64(v, f)[0]


def euler(faces):
    """V - E + F over the vertices and undirected edges the faces reference"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    edges = np.unique(np.sort(d, axis=1), axis=0)
    return len(np.unique(f)) - len(edges) + len(f)


# ---- the header on the host ------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "sls_mesh_math.h"

static const uint32_t *g_soup;
static int cmp_rows(const void *pa, const void *pb)
{
    const uint32_t a = *(const uint32_t *)pa, b = *(const uint32_t *)pb;
    for (int w = 0; w < 3; ++w) {
        const uint32_t ka = sls_mesh_word_key(g_soup[3 * (size_t)a + w]), kb = sls_mesh_word_key(g_soup[3 * (size_t)b + w]);
        if (ka != kb) return ka < kb ? -1 : 1;
    }
    return a < b ? -1 : (a > b ? 1 : 0);
}

/* returns V; out_vertices: room for n rows */
int ref_weld(int n, const uint32_t *soup, uint32_t *out_vertices, int32_t *out_index)
{
    uint32_t *order = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1));
    int V = 0;
    for (int i = 0; i < n; ++i) order[i] = (uint32_t)i;
    g_soup = soup;
    qsort(order, (size_t)n, sizeof(uint32_t), cmp_rows);
    for (int j = 0; j < n; ++j) {
        const uint32_t r = order[j];
        if (j == 0 || !sls_mesh_same_row(soup + 3 * (size_t)r, soup + 3 * (size_t)order[j - 1])) {
            memcpy(out_vertices + 3 * (size_t)V, soup + 3 * (size_t)r, 12);
            ++V;
        }
        out_index[r] = V - 1;
    }
    free(order);
    return V;
}

typedef struct { uint64_t key; uint32_t id; } Edge;
static int cmp_edges(const void *pa, const void *pb)
{
    const Edge *a = (const Edge *)pa, *b = (const Edge *)pb;
    if (a->key != b->key) return a->key < b->key ? -1 : 1;
    return a->id < b->id ? -1 : (a->id > b->id ? 1 : 0);
}
static uint32_t find(uint32_t *parent, uint32_t x)
{
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}

/* status: [C, degenerate, out_of_range, boundary_edges, nonmanifold_edges]; counts: room for T */
void ref_clusters(int T, const int32_t *faces, int V, int32_t *labels, int32_t *counts, uint32_t *status)
{
    const int bits = sls_mesh_index_bits(V);
    Edge *edges = (Edge *)malloc(sizeof(Edge) * (size_t)(3 * T + 1));
    uint32_t *parent = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(T + 1));
    int n = 0;
    memset(status, 0, 5 * sizeof(uint32_t));
    for (int t = 0; t < T; ++t) {
        const int d = sls_mesh_degenerate(faces + 3 * (size_t)t, V);
        parent[t] = (uint32_t)t;
        labels[t] = d ? -1 : -2;
        if (d) { status[1]++; if (d == 2) status[2]++; continue; }
        for (int e = 0; e < 3; ++e) { edges[n].key = sls_mesh_edge_key(faces + 3 * (size_t)t, e, bits); edges[n].id = (uint32_t)(3 * t + e); ++n; }
    }
    qsort(edges, (size_t)n, sizeof(Edge), cmp_edges);
    for (int j = 0; j < n;) {
        int len = 1;
        while (j + len < n && edges[j + len].key == edges[j].key) {
            uint32_t a = find(parent, edges[j + len].id / 3u), b = find(parent, edges[j + len - 1].id / 3u);
            if (a != b) { if (a < b) parent[b] = a; else parent[a] = b; }
            ++len;
        }
        if (len == 1) status[3]++;
        if (len > 2) status[4]++;
        j += len;
    }
    int Cn = 0;
    for (int t = 0; t < T; ++t)
        if (labels[t] != -1) {
            const uint32_t r = find(parent, (uint32_t)t);
            if (r == (uint32_t)t) { labels[t] = Cn; counts[Cn] = 0; ++Cn; }     /* (a root is its component's lowest triangle) */
            else labels[t] = labels[r];
            counts[labels[t]]++;
        }
    status[0] = (uint32_t)Cn;
    free(edges); free(parent);
}

static int cmp_desc(const void *pa, const void *pb)
{
    const int32_t a = *(const int32_t *)pa, b = *(const int32_t *)pb;
    return a > b ? -1 : (a < b ? 1 : 0);
}

/* status: [V', T', n_min]; out_vertices: room for V rows, out_faces: room for T rows */
void ref_filter(int V, const uint32_t *vertices, int T, const int32_t *faces, const int32_t *labels, const int32_t *counts, int Cn,
                int keep_clusters, int min_triangles, uint32_t *out_vertices, int32_t *out_faces, uint32_t *status)
{
    const uint32_t k = sls_mesh_keep_rank(keep_clusters, (uint32_t)Cn);
    uint32_t kth = 0;
    if (k > 0) {
        int32_t *sorted = (int32_t *)malloc(sizeof(int32_t) * (size_t)Cn);
        memcpy(sorted, counts, sizeof(int32_t) * (size_t)Cn);
        qsort(sorted, (size_t)Cn, sizeof(int32_t), cmp_desc);
        kth = (uint32_t)sorted[k - 1];
        free(sorted);
    }
    const uint32_t nm = sls_mesh_n_min(min_triangles, kth);
    int32_t *vmap = (int32_t *)malloc(sizeof(int32_t) * (size_t)(V + 1));
    int nv = 0, nt = 0;
    for (int v = 0; v < V; ++v) vmap[v] = -1;
    for (int t = 0; t < T; ++t)
        if (labels[t] >= 0 && (uint32_t)counts[labels[t]] >= nm)
            for (int c = 0; c < 3; ++c) vmap[faces[3 * (size_t)t + c]] = 0;
    for (int v = 0; v < V; ++v)
        if (vmap[v] == 0) { memcpy(out_vertices + 3 * (size_t)nv, vertices + 3 * (size_t)v, 12); vmap[v] = nv++; }
    for (int t = 0; t < T; ++t)
        if (labels[t] >= 0 && (uint32_t)counts[labels[t]] >= nm) {
            for (int c = 0; c < 3; ++c) out_faces[3 * (size_t)nt + c] = vmap[faces[3 * (size_t)t + c]];
            ++nt;
        }
    status[0] = (uint32_t)nv; status[1] = (uint32_t)nt; status[2] = nm;
    free(vmap);
}

void ref_normals(int V, const float *vertices, int T, const int32_t *faces, float *normals)
{
    float *sum = (float *)calloc((size_t)(3 * V + 1), sizeof(float));
    for (int t = 0; t < T; ++t) {
        const int32_t *f = faces + 3 * (size_t)t;
        float fn[3];
        if (sls_mesh_degenerate(f, V)) continue;
        sls_mesh_face_normal(vertices + 3 * (size_t)f[0], vertices + 3 * (size_t)f[1], vertices + 3 * (size_t)f[2], fn);
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) sum[3 * (size_t)f[c] + a] += fn[a];
    }
    for (int v = 0; v < V; ++v) sls_mesh_normalise(sum + 3 * (size_t)v, normals + 3 * (size_t)v);
    free(sum);
}

int ref_index_bits(int V) { return sls_mesh_index_bits(V); }
'''


class Host:
    """include/sls_mesh_math.h compiled as plain C and called through ctypes."""

    def __init__(self, lib):
        self.lib = lib
        lib.ref_weld.argtypes = [C.c_int] + [C.c_void_p] * 3
        lib.ref_clusters.restype = None
        lib.ref_clusters.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        lib.ref_filter.restype = None
        lib.ref_filter.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 3
        lib.ref_normals.restype = None
        lib.ref_normals.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.ref_index_bits.argtypes = [C.c_int]

    def weld(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((max(len(rows), 1), 3), np.float32)
        index = np.zeros((max(len(rows), 1),), np.int32)
        V = self.lib.ref_weld(len(rows), rows.ctypes.data, out.ctypes.data, index.ctypes.data)
        return out[:V], index[:len(rows)].astype(np.int64)

    def clusters(self, faces, V):
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        T = len(f)
        labels, counts = np.zeros((max(T, 1),), np.int32), np.zeros((max(T, 1),), np.int32)
        status = np.zeros((5,), np.uint32)
        self.lib.ref_clusters(T, f.ctypes.data, int(V), labels.ctypes.data, counts.ctypes.data, status.ctypes.data)
        stats = dict(zip(("clusters", "degenerate", "out_of_range", "boundary_edges", "nonmanifold_edges"), (int(x) for x in status)))
        return labels[:T].astype(np.int64), counts[:int(status[0])].astype(np.int64), stats

    def select(self, vertices, faces, keep_clusters, min_triangles):
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        labels, counts, _ = self.clusters(f, len(v))
        labels, counts = labels.astype(np.int32), np.ascontiguousarray(counts.astype(np.int32))
        cbuf = np.concatenate([counts, np.zeros((1,), np.int32)])
        out_v, out_f = np.zeros((max(len(v), 1), 3), np.float32), np.zeros((max(len(f), 1), 3), np.int32)
        status = np.zeros((3,), np.uint32)
        self.lib.ref_filter(len(v), v.ctypes.data, len(f), f.ctypes.data, labels.ctypes.data, cbuf.ctypes.data, len(counts), int(keep_clusters),
                            int(min_triangles), out_v.ctypes.data, out_f.ctypes.data, status.ctypes.data)
        return out_v[:int(status[0])], out_f[:int(status[1])].astype(np.int64), int(status[2])

    def normals(self, vertices, faces):
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((max(len(v), 1), 3), np.float32)
        self.lib.ref_normals(len(v), v.ctypes.data, len(f), f.ctypes.data, out.ctypes.data)
        return out[:len(v)]


_KEEP = []


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="mesh_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "mesh_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libmesh_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- shared test inputs ----------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def sphere_soup(radius=1.0, offset=(0.0, 0.0, 0.0)):
    """(3T,3) float32, read-only: the marching-tetrahedra soup of a sphere around tsdf_ref.CENTRE + offset (7152 triangles
    for radius 1 without an offset)."""
    centre = tsdf_ref.CENTRE + np.asarray(offset, dtype=np.float64)
    blocks, t, w = tsdf_ref.sphere_volume(centre, radius, tsdf_ref.VS, tsdf_ref.TRUNC, tsdf_ref.ORIGIN)
    tris, _ = tsdf_ref.host().extract(blocks, t, w, tsdf_ref.VS, tsdf_ref.ORIGIN)
    soup = np.ascontiguousarray(tris.reshape(-1, 3))
    soup.setflags(write=False)
    return soup


FAR = (6.0, 0.5, -0.25)


@functools.lru_cache(maxsize=None)
def floater_scene():
    """(vertices (V,3) float32, faces (T,3) int32), read-only: the welded unit sphere, a welded far sphere of radius 0.5 and
    five single floating triangles, concatenated in that order — 7 clusters."""
    parts, faces, base = [], [], 0
    for soup in (sphere_soup(), sphere_soup(0.5, FAR)):
        v, index = weld(soup)
        parts.append(v)
        faces.append(index.reshape(-1, 3) + base)
        base += len(v)
    rng = np.random.default_rng(11)
    for i in range(5):
        tri = (np.array([-4.0 - i, 3.0, 1.0]) + rng.normal(0, 0.05, (3, 3))).astype(np.float32)
        parts.append(tri)
        faces.append(np.arange(3).reshape(1, 3) + base)
        base += 3
    v, f = np.concatenate(parts).astype(np.float32), np.concatenate(faces).astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def strip(n=4096, seed=5):
    """n triangles (i, i + 1, i + 2) in a seeded random order over n + 2 vertices: one cluster of diameter n."""
    f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)
    return f[np.random.default_rng(seed).permutation(n)], n + 2


TWO_TETS = (np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0], [0, 4, 5], [0, 6, 4], [4, 6, 5], [5, 6, 0]], np.int32), 7)
FAN = (np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32), 5)
DEGENERATE = (np.array([[0, 1, 2], [3, 3, 4], [2, 1, 5], [0, 6, 1], [4, 5, 4], [-1, 0, 1], [5, 3, 4]], np.int32), 6)   # V = 6: index 6 is outside
ISOLATED = (np.array([[2, 0, 1]], np.int32), 3)


def cluster_cases():
    """name -> (faces, V)"""
    sv, sf = floater_scene()
    return {"two_tets": TWO_TETS, "strip": strip(), "fan": FAN, "degenerate": DEGENERATE, "isolated": ISOLATED,
            "scene": (sf, len(sv)), "empty": (np.zeros((0, 3), np.int32), 0)}


def weld_cases():
    """name -> (N,3) float32 rows"""
    rng = np.random.default_rng(3)
    lattice = rng.normal(0, 2, (40, 3)).astype(np.float32)
    nan_a, nan_b = 0x7FC00000, 0xFFC00123                     # two NaN payloads, set as bits
    nans = np.zeros((6, 3), np.uint32)
    nans[0, 0], nans[1, 0], nans[2, 0], nans[3, 1], nans[4, 2], nans[5, 1] = nan_a, nan_b, nan_a, nan_b, nan_a, nan_a
    cases = {
        "one_triangle": np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32),
        "shared_edge": np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32),
        "only_x": np.array([[3, 1, 1], [1, 1, 1], [2, 1, 1]], np.float32),
        "only_y": np.array([[1, 3, 1], [1, 1, 1], [1, 2, 1]], np.float32),
        "only_z": np.array([[1, 1, 3], [1, 1, 1], [1, 1, 2]], np.float32),
        "pass_order": np.array([[1, 2, 3], [1, 3, 2], [2, 1, 3], [2, 3, 1], [3, 1, 2], [3, 2, 1], [1, 2, 3], [3, 2, 1], [2, 2, 2]], np.float32),
        "negative": np.array([[-1, 2, 0], [1, -2, 0], [-3, -1, 5], [0.5, 0, -7], [-1, 2, 0], [-1, -2, 0]], np.float32),
        "signed_zero": np.array([[0.0, 1, 1], [-0.0, 1, 1], [0.0, 1, 1], [1, -0.0, 1], [1, 0.0, 1], [1, 1, -0.0]], np.float32),
        "nan_payloads": nans.view(np.float32),
        "lattice": lattice[rng.integers(0, 40, 9000)],
        "sphere": sphere_soup(),
        "empty": np.zeros((0, 3), np.float32),
    }
    return cases


def sized_rows(n, seed=0):
    """n rows over a lattice of about n / 3 points: every chunk boundary falls inside runs of equal rows and between them"""
    rng = np.random.default_rng(seed + n)
    pts = rng.normal(0, 3, (max(n // 3, 1), 3)).astype(np.float32)
    return pts[rng.integers(0, len(pts), n)]
