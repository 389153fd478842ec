"""include/sls_signdist_math.h compiled for the host (`host()`: the bit-for-bit reference of the device tests — the tables,
the status words, and a brute force over ALL faces with the float32 header for the nearest face, its feature and the sign),
a float64 NumPy restatement (`tables64`, `signed64`: brute force over all faces, libm's atan2 for the angles, the same
tables and the same sign rule) and the meshes the tests share."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import meshdist_ref
import nn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.float32

_DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "sls_signdist_math.h"
#include "sls_nn_math.h"

/* rows of 12 floats: q, a, b, c -> d2[n], rel[3 n], feature[n] */
void sd_triangles(long n, const float *rows, float *d2, float *rel, int32_t *feature)
{
    for (long i = 0; i < n; ++i) {
        const float *r = rows + 12 * i;
        int ft;
        d2[i] = sls_sd_triangle(r, r + 3, r + 6, r + 9, rel + 3 * i, &ft);
        feature[i] = ft;
    }
}
void sd_atan(long n, const double *x, double *out) { for (long i = 0; i < n; ++i) out[i] = sls_sd_atan(x[i]); }
/* rows of 6 doubles: u, w */
void sd_angles(long n, const double *uw, double *out) { for (long i = 0; i < n; ++i) out[i] = sls_sd_angle(uw + 6 * i, uw + 6 * i + 3); }

typedef struct { uint64_t key; uint32_t corner; } sd_edge;
static int sd_edge_cmp(const void *a, const void *b)
{
    const sd_edge *x = (const sd_edge *)a, *y = (const sd_edge *)b;
    if (x->key != y->key) return x->key < y->key ? -1 : 1;
    return x->corner < y->corner ? -1 : (x->corner > y->corner ? 1 : 0);
}

/* the three tables and the eight status words of sls_mesh_pseudonormals */
void sd_tables(int V, const float *vertices, int F, const int32_t *faces, float *face_n, float *edge_n, float *vertex_n, uint32_t *status)
{
    const int bits = sls_mesh_index_bits(V);
    double *fn = (double *)malloc(sizeof(double) * 3 * (size_t)F), *ang = (double *)malloc(sizeof(double) * 3 * (size_t)F);
    double *vs = (double *)calloc(3 * (size_t)V, sizeof(double));
    sd_edge *e = (sd_edge *)malloc(sizeof(sd_edge) * 3 * (size_t)F);
    size_t ne = 0;
    memset(status, 0, 8 * sizeof(uint32_t));
    memset(edge_n, 0, sizeof(float) * 9 * (size_t)F);
    for (size_t f = 0; f < (size_t)F; ++f) {
        const int cls = sls_sd_face(vertices, faces + 3 * f, V, fn + 3 * f, ang + 3 * f);
        status[0] += cls == 1 || cls == 2; status[1] += cls == 2; status[2] += cls == 3; status[3] += cls == 4;
        for (int k = 0; k < 3; ++k) {
            face_n[3 * f + k] = (float)fn[3 * f + k];
            if (cls == 1 || cls == 2) continue;
            e[ne].key = sls_mesh_edge_key(faces + 3 * f, k, bits); e[ne].corner = (uint32_t)(3 * f + k); ++ne;
            sls_sd_accumulate(vs + 3 * (size_t)faces[3 * f + k], ang[3 * f + k], fn + 3 * f);      /* ascending corner id */
        }
    }
    qsort(e, ne, sizeof(sd_edge), sd_edge_cmp);
    for (size_t j = 0; j < ne;) {
        size_t end = j;
        double s[3] = { 0.0, 0.0, 0.0 };
        for (; end < ne && e[end].key == e[j].key; ++end) sls_sd_accumulate(s, 1.0, fn + 3 * (size_t)(e[end].corner / 3u));
        for (size_t i = j; i < end; ++i)
            for (int k = 0; k < 3; ++k) edge_n[3 * (size_t)e[i].corner + k] = (float)s[k];
        status[4] += end - j == 1; status[5] += end - j >= 3;
        status[6] += end - j == 2 && faces[e[j].corner] == faces[e[j + 1].corner];
        j = end;
    }
    for (size_t i = 0; i < 3 * (size_t)V; ++i) vertex_n[i] = (float)vs[i];
    status[7] = 1;
    free(fn); free(ang); free(vs); free(e);
}

/* sls_mesh_signed_distance by brute force: the float32 header against every face a query may meet */
void sd_query(int V, const float *vertices, int F, const int32_t *faces, const float *face_n, const float *edge_n,
              const float *vertex_n, long M, const float *q, float *sd, int32_t *face, float *closest, uint8_t *feature)
{
    uint8_t *ok = (uint8_t *)malloc((size_t)F);
    for (size_t f = 0; f < (size_t)F; ++f) {
        const int32_t *x = faces + 3 * f;
        ok[f] = sls_mesh_degenerate(x, V) != 2 && sls_sd_finite3(vertices + 3 * (size_t)x[0]) && sls_sd_finite3(vertices + 3 * (size_t)x[1]) &&
                sls_sd_finite3(vertices + 3 * (size_t)x[2]);
    }
#pragma omp parallel for schedule(static)
    for (long i = 0; i < M; ++i) {
        const float *p = q + 3 * i;
        uint64_t best = SLS_NN_KEY_NONE;
        for (size_t f = 0; f < (size_t)F; ++f) {
            if (!ok[f]) continue;
            const float *a = vertices + 3 * (size_t)faces[3 * f], *b = vertices + 3 * (size_t)faces[3 * f + 1], *c = vertices + 3 * (size_t)faces[3 * f + 2];
            const uint64_t key = sls_nn_key(sls_meshdist_triangle(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], 0), (uint32_t)f);
            best = key < best ? key : best;
        }
        const uint32_t f = sls_nn_key_index(best);
        const float d2 = sls_nn_key_dist2(best);
        int ft = 0;
        sd[i] = sqrtf(d2); face[i] = (int32_t)f; closest[3 * i] = p[0]; closest[3 * i + 1] = p[1]; closest[3 * i + 2] = p[2];
        if (f < (uint32_t)F) {
            const int32_t *x = faces + 3 * (size_t)f;
            const float *a = vertices + 3 * (size_t)x[0], *b = vertices + 3 * (size_t)x[1], *c = vertices + 3 * (size_t)x[2];
            float rel[3];
            const float *row = face_n + 3 * (size_t)f;
            sls_meshdist_triangle(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], closest + 3 * i);
            sls_sd_triangle(p, a, b, c, rel, &ft);
            if (ft >= 4) row = vertex_n + 3 * (size_t)x[ft - 4];
            else if (ft >= 1) row = edge_n + 3 * (3 * (size_t)f + (size_t)(ft - 1));
            sd[i] = sls_sd_signed(d2, rel, row);
        }
        feature[i] = (uint8_t)ft;
    }
    free(ok);
}

void sd_colors(long n, const float *sd, float truncation, uint8_t *rgb)
{
    for (long i = 0; i < n; ++i) sls_signed_error_color(sd[i], truncation, rgb + 3 * i);
}
'''

_KEEP = []


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp, L = C.c_void_p, C.c_long
        lib.sd_triangles.argtypes = [L, vp, vp, vp, vp]
        lib.sd_atan.argtypes = [L, vp, vp]
        lib.sd_angles.argtypes = [L, vp, vp]
        lib.sd_tables.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
        lib.sd_query.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp, L, vp, vp, vp, vp, vp]
        lib.sd_colors.argtypes = [L, vp, C.c_float, vp]

    def triangles(self, q, a, b, c):
        """(d2 (n,), rel (n,3) float32, feature (n,) int32) of sls_sd_triangle for rows of queries and triangles."""
        rows = np.ascontiguousarray(np.concatenate(np.broadcast_arrays(*(np.asarray(x, _f) for x in (q, a, b, c))), axis=1))
        n = len(rows)
        d2, rel, feature = np.empty(n, _f), np.empty((n, 3), _f), np.empty(n, np.int32)
        self.lib.sd_triangles(n, rows.ctypes.data, d2.ctypes.data, rel.ctypes.data, feature.ctypes.data)
        return d2, rel, feature

    def atan(self, x):
        x = np.ascontiguousarray(x, np.float64)
        out = np.empty_like(x)
        self.lib.sd_atan(len(x), x.ctypes.data, out.ctypes.data)
        return out

    def angles(self, u, w):
        uw = np.ascontiguousarray(np.concatenate([np.asarray(u, np.float64), np.asarray(w, np.float64)], axis=1))
        out = np.empty(len(uw))
        self.lib.sd_angles(len(uw), uw.ctypes.data, out.ctypes.data)
        return out

    def tables(self, vertices, faces):
        """(face_n (F,3), edge_n (F,3,3), vertex_n (V,3) float32, status (8,) uint32)"""
        v, f = np.ascontiguousarray(vertices, _f), np.ascontiguousarray(faces, np.int32)
        fn, en, vn = np.empty((len(f), 3), _f), np.empty((len(f), 3, 3), _f), np.empty((len(v), 3), _f)
        status = np.empty(8, np.uint32)
        self.lib.sd_tables(len(v), v.ctypes.data, len(f), f.ctypes.data, fn.ctypes.data, en.ctypes.data, vn.ctypes.data, status.ctypes.data)
        return fn, en, vn, status

    def query(self, vertices, faces, tables, q):
        """(sdist (M,), face (M,) int32, closest (M,3), feature (M,) uint8): the header against every face."""
        v, f, q = np.ascontiguousarray(vertices, _f), np.ascontiguousarray(faces, np.int32), np.ascontiguousarray(q, _f)
        fn, en, vn = (np.ascontiguousarray(t, _f) for t in tables[:3])
        M = len(q)
        sd, face, closest, feature = np.empty(M, _f), np.empty(M, np.int32), np.empty((M, 3), _f), np.empty(M, np.uint8)
        self.lib.sd_query(len(v), v.ctypes.data, len(f), f.ctypes.data, fn.ctypes.data, en.ctypes.data, vn.ctypes.data, M, q.ctypes.data,
                          sd.ctypes.data, face.ctypes.data, closest.ctypes.data, feature.ctypes.data)
        return sd, face, closest, feature

    def colors(self, sd, truncation):
        sd = np.ascontiguousarray(sd, _f)
        rgb = np.empty((len(sd), 3), np.uint8)
        self.lib.sd_colors(len(sd), sd.ctypes.data, float(truncation), rgb.ctypes.data)
        return rgb


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="signdist_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "signdist_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libsigndist_host.so")
    cmd = ["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-o", so, "-lm"]
    # the brute force is a loop over independent queries: threads where the compiler has them, the same bits without
    if subprocess.call(cmd + ["-fopenmp"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd + ["-Wno-unknown-pragmas"])
    return Host(C.CDLL(so))


def stats(sd, truncation):
    """(n, negative, float64 sum) of sls_signed_stats; the sum in NumPy's order, not the device's"""
    sd = np.asarray(sd, _f)
    with np.errstate(invalid="ignore"):
        m = np.abs(sd) < _f(truncation)
    return int(m.sum()), int((sd[m] < 0).sum()), float(sd[m].astype(np.float64).sum())


def stats_device_order(sd, truncation):
    """stats with the sum in the device's order (nn_ref.device_sum): the first three words of sls_signed_stats, bit for bit"""
    sd = np.asarray(sd, _f)
    with np.errstate(invalid="ignore"):
        m = np.abs(sd) < _f(truncation)
    return stats(sd, truncation)[:2] + (nn_ref.device_sum(np.where(m, sd.astype(np.float64), 0.0)),)


# ---- the float64 restatement -----------------------------------------------------------------------------------------
def tables64(vertices, faces):
    """(face_n (F,3), edge_n (F,3,3), vertex_n (V,3)) float64; the angles by libm's atan2, the sums by np.add.at.  For
    meshes without index-degenerate faces."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    p = v[f]                                                            # (F, 3, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    fn = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
    vn = np.zeros((len(v), 3))
    en = np.zeros((len(f), 3, 3))
    lo, hi = np.minimum(f, np.roll(f, -1, 1)), np.maximum(f, np.roll(f, -1, 1))
    _, group = np.unique(lo.reshape(-1) * (len(v) + 1) + hi.reshape(-1), return_inverse=True)
    sums = np.zeros((group.max() + 1, 3))
    np.add.at(sums, group, np.repeat(fn, 3, axis=0))
    en[:] = sums[group].reshape(len(f), 3, 3)
    for k in range(3):
        u, w = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        theta = np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(1))
        np.add.at(vn, f[:, k], np.where(ln > 0, theta[:, None], 0.0) * fn)
    return fn, en, vn


def signed64(q, vertices, faces, chunk=4096):
    """(signed distance (M,) float64, face (M,)): the float64 brute force over all faces, the feature of the closest point
    read off its position (within 1e-9 of a vertex, else of an edge, else the face), the float64 tables, the same sign rule."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    fn, en, vn = tables64(v, f)
    q = np.asarray(q, np.float64)
    a, b, c = (v[f[:, k]] for k in range(3))
    out, face = np.empty(len(q)), np.empty(len(q), np.int64)
    for i in range(0, len(q), chunk):
        qq = q[i:i + chunk]
        d2, cl = meshdist_ref.triangle64(qq[:, None, :], a[None], b[None], c[None])
        j = d2.argmin(1)
        rows = np.arange(len(qq))
        cp, tri = cl[rows, j], v[f[j]]
        n = fn[j]
        for k in range(3):                                              # an edge, where the closest point lies on one
            e0, e1 = tri[:, k], tri[:, (k + 1) % 3]
            t = ((cp - e0) * (e1 - e0)).sum(1) / ((e1 - e0) ** 2).sum(1)
            on = np.linalg.norm(cp - (e0 + t[:, None] * (e1 - e0)), axis=1) < 1e-9
            n = np.where(on[:, None], en[j, k], n)
        for k in range(3):                                              # a vertex beats an edge
            n = np.where((np.linalg.norm(cp - tri[:, k], axis=1) < 1e-9)[:, None], vn[f[j, k]], n)
        s = ((qq - cp) * n).sum(1)
        out[i:i + chunk] = np.where(s < 0, -1.0, 1.0) * np.sqrt(d2[rows, j])
        face[i:i + chunk] = j
    return out, face


# ---- the shared meshes ---------------------------------------------------------------------------------------------------
def _ro(v, f):
    v, f = np.ascontiguousarray(v, _f), np.ascontiguousarray(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def _outward(v, f):
    """the faces of a CONVEX mesh turned so that their normals point away from its centroid"""
    v64, f = np.asarray(v, np.float64), np.array(f, np.int64)
    p = v64[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    flip = (n * (p.mean(1) - v64.mean(0))).sum(1) < 0
    f[flip] = f[flip][:, ::-1]
    return f


def inside_convex(q, vertices, faces):
    """behind all planes of a convex, outward-oriented mesh: float64"""
    v, q = np.asarray(vertices, np.float64), np.asarray(q, np.float64)
    p = v[np.asarray(faces)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return ((q[:, None, :] - p[None, :, 0]) * n[None]).sum(-1).max(1) < 0


@functools.lru_cache(maxsize=None)
def blade():
    """A thin tetrahedron, half a metre thick at one end and an edge at the other: its two large faces meet along the edge
    (0,0,0)-(4,0,0) at about ten degrees, so a large share of the space around it is nearest to an edge or a vertex where
    the normal of the face the search happens to name points the wrong way."""
    v = np.array([[0, 0, 0], [4, 0, 0], [2, 3, 0.25], [2, 3, -0.25]], np.float64)
    return _ro(v, _outward(v, [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]))


def blade_queries(n, seed):
    return np.random.default_rng(seed).uniform([-1, -1, -1], [5, 4, 1], (n, 3)).astype(_f)


@functools.lru_cache(maxsize=None)
def cube():
    """[1/16, 17/16]^3, twelve outward faces"""
    g = np.array([1 / 16, 17 / 16])
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return _ro(v, _outward(v, f))


def cube_queries():
    """the 1/16 lattice of [0, 18/16]^3: on the surface, inside and outside"""
    g = np.arange(0, 19) / 16.0
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(_f)


_L = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)


@functools.lru_cache(maxsize=None)
def l_prism(h=1.0):
    """The L-shaped hexagon extruded along z: closed, oriented outward, with one reflex edge at (1, 1)."""
    n = len(_L)
    v = np.concatenate([np.c_[_L, np.zeros(n)], np.c_[_L, np.full(n, h)]])
    f = []
    for i in range(1, n - 1):                                           # the fan from (0, 0) stays inside the L
        f += [(0, i + 1, i), (n, n + i, n + i + 1)]                     # bottom looks down, top looks up
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, n + j), (i, n + j, n + i)]
    return _ro(v, np.array(f))


def l_prism_inside(q, h=1.0):
    x, y, z = (np.asarray(q, np.float64)[:, k] for k in range(3))
    return (((x > 0) & (x < 2) & (y > 0) & (y < 1)) | ((x > 0) & (x < 1) & (y > 0) & (y < 2))) & (z > 0) & (z < h)


@functools.lru_cache(maxsize=None)
def folded_sheet():
    """An open sheet folded along the y axis with 20 degrees between its wings: a sharp ridge and boundary edges."""
    half = np.deg2rad(10.0)
    xs = np.array([[-np.sin(half), -np.cos(half)], [0.0, 0.0], [np.sin(half), -np.cos(half)]]) * 2.0
    ys = np.arange(4) * 0.5
    v = np.array([[x, y, z] for y in ys for x, z in xs])
    f = []
    for r in range(3):
        for c in range(2):
            k = 3 * r + c
            f += [(k, k + 1, k + 4), (k, k + 4, k + 3)]
    return _ro(v, np.array(f))


@functools.lru_cache(maxsize=None)
def defects():
    """The cube with one of each defect: a flipped triangle, a fin on an edge (three owners), a repeated triangle, a
    zero-area face and an index-degenerate face."""
    v, f = cube()
    v = np.concatenate([v, [[0.5, 0.5, 2.0], [3, 3, 3], [3.5, 3.5, 3.5], [4, 4, 4]]])
    f = np.array(f)
    f[3] = f[3][::-1]
    extra = [[f[0][0], f[0][1], 8], list(f[5]), [9, 10, 11], [2, 2, 5]]
    return _ro(v, np.concatenate([f, extra]))


@functools.lru_cache(maxsize=None)
def icosphere(level=4, r=1.0):
    """20 x 4^level faces (4: 5 120), outward, vertices on the sphere of radius r in float64 then rounded"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    v = np.array(v) * r
    return _ro(v, _outward(v, f))


def mean_radius(vertices, faces, n=8):
    """The area-weighted mean distance of a mesh's SURFACE from the origin, float64: every face cut into n^2 equal
    sub-triangles, their centroids weighted by the face's area.  An icosphere with its vertices on the sphere of radius r
    lies inside that sphere everywhere else: its mean radius is below r by the mean sagitta of its facets."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces)
    p = v[f]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    w = []
    for i in range(n):
        for j in range(n - i):
            w.append(((i + 1 / 3) / n, (j + 1 / 3) / n))                # the upright sub-triangles
            if j < n - i - 1:
                w.append(((i + 2 / 3) / n, (j + 2 / 3) / n))            # the inverted ones
    w = np.array(w)
    pts = p[:, None, 0] + w[None, :, :1] * (p[:, None, 1] - p[:, None, 0]) + w[None, :, 1:] * (p[:, None, 2] - p[:, None, 0])
    return float((np.linalg.norm(pts, axis=2).mean(1) * area).sum() / area.sum())


@functools.lru_cache(maxsize=None)
def wavy_grid(n=320):
    """the wavy n x n grid of tests/test_raycast_scale.py: 2 n^2 shuffled faces (320: 204 800 faces, 614 400 corners)"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i * 0.05, j * 0.05, 0.25 * np.sin(i * 0.07) + 0.02 * j], -1).reshape(-1, 3).astype(_f)
    k = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([k, k + n + 1, k + 1], 1), np.stack([k + 1, k + n + 1, k + n + 2], 1)]).astype(np.int32)
    return _ro(v, f[np.random.default_rng(5).permutation(len(f))])
