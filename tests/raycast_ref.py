"""The ray caster's references: include/sls_raycast_math.h compiled for the host (the bit-for-bit reference of the device
tests: `host().cast` is the brute force over ALL faces with the header's routine and its key rule), a float64
Möller-Trumbore that also says how clear each case is, and the meshes and rays the tests share."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # the project's float bar, of the scale
_f = np.float32

_DRIVER = r'''
#include "sls_raycast_math.h"
/* rows of 15 floats: o, d, a, b, c -> hit[n], tuv[3 n] */
void rc_triangles(int n, const float *rows, float t_min, float t_max, int *hit, float *tuv)
{
    for (long i = 0; i < n; ++i) {
        const float *r = rows + 15 * i;
        tuv[3 * i] = tuv[3 * i + 1] = tuv[3 * i + 2] = 0.0f;
        hit[i] = sls_ray_triangle(r, r + 3, r + 6, r + 9, r + 12, t_min, t_max, tuv + 3 * i, tuv + 3 * i + 1, tuv + 3 * i + 2);
    }
}
/* rows of 12 floats: o, d, mn, mx; t_hi per row -> pass[n] */
void rc_boxes(int n, const float *rows, float t_lo, const float *t_hi, int *pass)
{
    for (long i = 0; i < n; ++i) {
        const float *r = rows + 12 * i;
        float inv[3];
        sls_ray_inverse(r + 3, inv);
        pass[i] = sls_ray_box(r, inv, sls_ray_axis(r + 3), r + 6, r + 9, t_lo, t_hi[i]);
    }
}
void rc_valid(int n, const float *o, const float *d, int *ok)
{
    for (long i = 0; i < n; ++i) ok[i] = sls_ray_valid(o + 3 * i, d + 3 * i);
}
/* the brute force: every ray against every face, the minimum key; a face with a vertex index outside [0, V) or a
 * non-finite vertex never hits, a refused ray misses */
void rc_cast(int V, const float *vertices, int F, const int *faces, int n, const float *o, const float *d, float t_min,
             float t_max, float *out_t, int *out_face, float *out_uv)
{
    for (long i = 0; i < n; ++i) {
        uint64_t best = SLS_NN_KEY_NONE;
        float bu = 0.0f, bv = 0.0f;
        if (sls_ray_valid(o + 3 * i, d + 3 * i)) {
            sls_ray_frame fr;
            sls_ray_setup(o + 3 * i, d + 3 * i, &fr);
            for (long f = 0; f < F; ++f) {
                const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
                float t, u, v;
                int k, fin = 1;
                if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;
                for (k = 0; k < 3; ++k)
                    fin = fin && fabsf(vertices[3 * i0 + k]) <= FLT_MAX && fabsf(vertices[3 * i1 + k]) <= FLT_MAX &&
                          fabsf(vertices[3 * i2 + k]) <= FLT_MAX;
                if (!fin) continue;
                if (sls_ray_triangle_frame(&fr, vertices + 3 * i0, vertices + 3 * i1, vertices + 3 * i2, t_min, t_max, &t, &u, &v)) {
                    const uint64_t key = sls_nn_key(t, (uint32_t)f);
                    if (key < best) { best = key; bu = u; bv = v; }
                }
            }
        }
        out_t[i] = sls_nn_key_dist2(best);
        out_face[i] = (int)sls_nn_key_index(best);
        out_uv[2 * i] = bu;
        out_uv[2 * i + 1] = bv;
    }
}
'''

_KEEP = []


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp = C.c_void_p
        lib.rc_triangles.argtypes = [C.c_int, vp, C.c_float, C.c_float, vp, vp]
        lib.rc_boxes.argtypes = [C.c_int, vp, C.c_float, vp, vp]
        lib.rc_valid.argtypes = [C.c_int, vp, vp, vp]
        lib.rc_cast.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_float, C.c_float, vp, vp, vp]

    def triangles(self, o, d, a, b, c, t_min=0.0, t_max=np.inf):
        """(hit (n,) bool, t, u, v (n,) float32) of sls_ray_triangle for rows of rays and triangles."""
        rows = np.ascontiguousarray(np.concatenate(np.broadcast_arrays(*(np.asarray(x, _f) for x in (o, d, a, b, c))), axis=1))
        n = len(rows)
        hit, tuv = np.empty(n, np.int32), np.empty((n, 3), _f)
        self.lib.rc_triangles(n, rows.ctypes.data, float(t_min), float(t_max), hit.ctypes.data, tuv.ctypes.data)
        return hit != 0, tuv[:, 0].copy(), tuv[:, 1].copy(), tuv[:, 2].copy()

    def boxes(self, o, d, mn, mx, t_hi, t_lo=0.0):
        rows = np.ascontiguousarray(np.concatenate(np.broadcast_arrays(*(np.asarray(x, _f) for x in (o, d, mn, mx))), axis=1))
        n = len(rows)
        t_hi = np.ascontiguousarray(np.broadcast_to(np.asarray(t_hi, _f), (n,)))
        out = np.empty(n, np.int32)
        self.lib.rc_boxes(n, rows.ctypes.data, float(t_lo), t_hi.ctypes.data, out.ctypes.data)
        return out != 0

    def valid(self, o, d):
        o, d = np.ascontiguousarray(o, _f), np.ascontiguousarray(d, _f)
        out = np.empty(len(o), np.int32)
        self.lib.rc_valid(len(o), o.ctypes.data, d.ctypes.data, out.ctypes.data)
        return out != 0

    def cast(self, vertices, faces, o, d, t_min=0.0, t_max=np.inf):
        """(t (n,) float32 (+inf: miss), face (n,) int32 (-1: miss), uv (n,2) float32): the brute force."""
        v, f = np.ascontiguousarray(vertices, _f), np.ascontiguousarray(faces, np.int32)
        o, d = np.ascontiguousarray(o, _f), np.ascontiguousarray(d, _f)
        n = len(o)
        t, face, uv = np.empty(n, _f), np.empty(n, np.int32), np.empty((n, 2), _f)
        self.lib.rc_cast(len(v), v.ctypes.data, len(f), f.ctypes.data, n, o.ctypes.data, d.ctypes.data, float(t_min), float(t_max),
                         t.ctypes.data, face.ctypes.data, uv.ctypes.data)
        return t, face, uv


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="raycast_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "raycast_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libraycast_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- float64 ------------------------------------------------------------------------------------------------------------
def moller_trumbore64(o, d, a, b, c, t_min=0.0, t_max=np.inf):
    """(hit, t, u, v, margin) in float64 for rows of rays and triangles.  margin says how clear the decision is, each part
    relative: the smallest barycentric weight (negative outside), the distance of t from the ends of [t_min, t_max] over
    max(|t|, 1e-300) (negative outside), and |cos| between the ray and the face's normal; `margin` is the SMALLEST ABSOLUTE
    value of the three — a case is clear when it is large, whichever side of hit / miss it lies on."""
    o, d, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (o, d, a, b, c)))
    e1, e2 = b - a, c - a
    n = np.cross(e1, e2)
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = o - a
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        cos = np.abs((n * d).sum(-1)) / (np.linalg.norm(n, axis=-1) * np.linalg.norm(d, axis=-1))
        wmin = np.minimum(np.minimum(u, v), 1.0 - u - v)
        tdist = np.minimum(t - t_min, t_max - t) / np.maximum(np.abs(t), 1e-300)
    hit = (det != 0) & (wmin >= 0) & (t >= t_min) & (t <= t_max)
    margin = np.minimum(np.minimum(np.abs(wmin), np.abs(tdist)), cos)
    margin = np.where(np.isfinite(margin), margin, 0.0)
    return hit, t, u, v, margin


def scale_of(o, a, b, c):
    """The largest distance from the ray's origin to the face's three vertices, float64."""
    o, a, b, c = (np.asarray(x, np.float64) for x in (o, a, b, c))
    return np.maximum(np.maximum(np.linalg.norm(a - o, axis=-1), np.linalg.norm(b - o, axis=-1)), np.linalg.norm(c - o, axis=-1))


def shape_of(a, b, c):
    """(longest edge, height over it) of rows of triangles, float64."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    longest = np.maximum(np.maximum(np.linalg.norm(b - a, axis=-1), np.linalg.norm(c - b, axis=-1)), np.linalg.norm(a - c, axis=-1))
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=-1)
    return longest, area2 / np.maximum(longest, 1e-300)


def random_cases(n, seed, sliver_share=0.25, aligned_slivers=True):
    """(o, d, a, b, c) float32 (n,3) each, the triangles in the style of meshdist_ref.random_cases: coordinates up to 64 m,
    sizes 1 cm to 10 m (log-uniform), a share of them slivers of height 1e-4 of their size.  Half of the rays aim at a
    point drawn uniformly ON the triangle (Dirichlet weights), half at a point of its plane up to about one size outside.
    An ordinary face is seen from 0.1 to 100 sizes away, from any side, at least 3 degrees off its plane.
    A SLIVER is what float32 cannot range in general: the edge functions of a face 10^4 times longer than high carry a
    weight noise of about 2^-24 10^4 / cos, and t = (U Az + V Bz + W Cz) / det moves by that noise times the spread of the
    vertices along the ray's DOMINANT AXIS — up to 1e-3 of the face's length, far above 1e-5 of the scale unless the face
    is seen from hundreds of lengths away, where no hit / miss decision on it is clear any more (it is thinner than an ulp
    of the scale).  So the slivers here have their long axis along a coordinate axis and are seen from 0.3 to 3 sizes
    away ACROSS it (the ray within 0.3 degrees of the plane through the normal and the thin direction, up to 60 degrees
    off the normal): the long axis then has no extent along the dominant axis, the decision is as hard as ever, and t
    can be held to the bar.  test_raycast_math.py measures the general orientation separately, against the figure above."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-2, 1, (n, 1))
    a = rng.uniform(-54, 54, (n, 3))
    e0, e1 = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))
    e0 /= np.linalg.norm(e0, axis=1, keepdims=True)
    e1 -= (e1 * e0).sum(1, keepdims=True) * e0
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    sliver = rng.random((n, 1)) < sliver_share
    height = np.where(sliver, 1e-4, rng.uniform(0.1, 1.0, (n, 1)))
    if aligned_slivers:
        axis = np.eye(3)[rng.integers(0, 3, n)]
        e0 = np.where(sliver, axis, e0)
        e1 = np.where(sliver, e1 - (e1 * e0).sum(1, keepdims=True) * e0, e1)
        e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    a = a.astype(_f).astype(np.float64)         # so that b - a stays along e0 after the rounding
    b = a + size * e0
    c = a + size * (rng.uniform(-0.5, 1.5, (n, 1)) * e0 + height * e1)
    a, b, c = (np.clip(x, -64, 64).astype(_f) for x in (a, b, c))
    a64, b64, c64 = (x.astype(np.float64) for x in (a, b, c))
    w = rng.dirichlet((1, 1, 1), n)
    w = np.where(rng.random((n, 1)) < 0.5, w, w + rng.normal(0, 1.0, (n, 3)))
    w /= w.sum(1, keepdims=True)
    target = w[:, :1] * a64 + w[:, 1:2] * b64 + w[:, 2:] * c64
    # the frame of the triangle AS ROUNDED to float32 (a 1 cm sliver is lower than an ulp of its coordinates: what is
    # cast against is whatever the rounding left): the longest edge, the normal, the thin direction
    edges = np.stack([b64 - a64, c64 - b64, a64 - c64], 1)
    e0 = edges[np.arange(n), np.argmax((edges * edges).sum(2), 1)]
    e0 /= np.linalg.norm(e0, axis=1, keepdims=True)
    nrm = np.cross(b64 - a64, c64 - a64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    e1 = np.cross(nrm, e0)
    # the direction from the target back to the origin
    any_dir = rng.normal(0, 1, (n, 3))
    any_dir /= np.linalg.norm(any_dir, axis=1, keepdims=True)
    off = (any_dir * nrm).sum(1, keepdims=True)
    any_dir = np.where(np.abs(off) < 0.05, any_dir + np.sign(off + 1e-30) * 0.1 * nrm, any_dir)
    alpha = rng.uniform(-np.pi / 3, np.pi / 3, (n, 1))
    across = np.cos(alpha) * nrm * np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0) + np.sin(alpha) * e1 + rng.uniform(-0.005, 0.005, (n, 1)) * e0
    back = np.where(sliver, across, any_dir)
    dist = size * np.where(sliver, 10.0 ** rng.uniform(-0.5, 0.5, (n, 1)), 10.0 ** rng.uniform(-1, 2, (n, 1)))
    o = np.clip(target + back * dist, -64, 64).astype(_f)
    d = (target - o.astype(np.float64)) * 10.0 ** rng.uniform(-1, 1, (n, 1))      # not unit
    return o, d.astype(_f), a, b, c


# ---- meshes -------------------------------------------------------------------------------------------------------------
def _ro(v, f):
    v, f = np.ascontiguousarray(v, _f), np.ascontiguousarray(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def octahedron(r=4):
    v = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]])
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return _ro(v, f)


@functools.lru_cache(maxsize=None)
def cube(n=1, half=4.0, seed=None):
    """A closed cube [-half, half]^3, every side n x n quads of two triangles (n = 1: 12 faces), vertices shared between
    the sides (welded), so every edge belongs to exactly two faces.  seed: the faces in a seeded random order."""
    pts, index = [], {}

    def vid(p):
        key = tuple(int(round(x)) for x in p)       # lattice units: 2 half / n
        if key not in index:
            index[key] = len(pts)
            pts.append(key)
        return index[key]

    faces = []
    for axis in range(3):
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        p = [0, 0, 0]
                        p[axis] = side
                        p[(axis + 1) % 3] = i + di
                        p[(axis + 2) % 3] = j + dj
                        return vid(p)
                    q = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
                    if side == 0:
                        q = q[::-1]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    v = np.array(pts, np.float64) * (2.0 * half / n) - half
    f = np.array(faces)
    if seed is not None:
        f = f[np.random.default_rng(seed).permutation(len(f))]
    return _ro(v, f)


@functools.lru_cache(maxsize=None)
def sphere(n_lat=24, n_lon=48, r=3.0):
    """A closed latitude / longitude sphere about the origin, every vertex at radius r: (vertices, faces)."""
    v = [[0.0, 0.0, r]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)])
    v.append([0.0, 0.0, -r])
    south = len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)
    f = []
    for j in range(n_lon):
        f.append([0, ring(1, j), ring(1, j + 1)])
        f.append([south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return _ro(np.array(v), np.array(f))


def edges_of(faces):
    """The undirected edges (E,2) of a mesh."""
    f = np.asarray(faces)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


def rays_at(points, origin):
    """Rays from `origin` exactly at `points`: direction = point - origin (exact on a lattice)."""
    p = np.asarray(points, np.float64)
    o = np.broadcast_to(np.asarray(origin, np.float64), p.shape)
    return o.astype(_f), (p - o).astype(_f)


def rays_for(vertices, faces, m, seed):
    """(origins, directions) (m,3) float32 against a mesh, in turn: aimed at a point on a random face from nearby, aimed at
    a face from far away, a random direction from inside the bounding box, and a ray that starts outside and points away."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max()) or 1.0
    tri = v[np.asarray(faces)[rng.integers(0, len(faces), m)]]
    w = rng.dirichlet((1, 1, 1), m)
    on = (w[:, :, None] * tri).sum(1)
    kind = np.arange(m) % 4
    unit = rng.normal(0, 1, (m, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    o = np.where((kind == 0)[:, None], on + unit * 0.3 * ext, 0)
    o = np.where((kind == 1)[:, None], on + unit * 20 * ext, o)
    o = np.where((kind == 2)[:, None], rng.uniform(lo, hi + 1e-9, (m, 3)), o)
    o = np.where((kind == 3)[:, None], hi + 2 * ext, o)
    d = np.where((kind <= 1)[:, None], on - o, unit)
    d = np.where((kind == 3)[:, None], np.abs(unit), d)
    return o.astype(_f), (d * 10.0 ** rng.uniform(-1, 1, (m, 1))).astype(_f)
