"""NumPy restatement of the point-to-triangle distance and of the error colours (include/sls_meshdist_math.h), the header
itself compiled for the host, and the meshes the tests share.

`triangle64` is the float64 brute force: the minimum over the three edge segments and the plane's foot point where it
falls inside — in float64 the decision errs by 1e-16 of the scale over the height, nothing a float32 result could see.
`triangle32` is the float32 twin of the header's steps.  Its fmaf is the float64 product-sum rounded to float32: the
product of two float32 is exact in float64, the sum is rounded to 53 bits and then to 24, so it differs from a true fma
only where that double rounding bites (about one operation in 2^29); the twin is a restatement to read and to measure
with, the bit-for-bit reference of the device tests is the header compiled for the host (`host()`)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # the project's float bar, of the scale


def scale_of(q, a, b, c):
    """The largest distance from the query to the face's three vertices, float64."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    return np.maximum(np.maximum(np.linalg.norm(a - q, axis=-1), np.linalg.norm(b - q, axis=-1)), np.linalg.norm(c - q, axis=-1))


def _segment64(P, e):
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, -(P * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    p = P + np.clip(t, 0.0, 1.0)[..., None] * e
    return (p * p).sum(-1), p


def triangle64(q, a, b, c):
    """(d2, closest) in float64 for rows of queries and triangles (broadcast against each other)."""
    q, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (q, a, b, c)))
    A, B, Cc = a - q, b - q, c - q
    d2, best = _segment64(A, B - A)
    for P, e in ((B, Cc - B), (Cc, A - Cc)):
        e2, p = _segment64(P, e)
        lower = e2 < d2
        d2, best = np.where(lower, e2, d2), np.where(lower[..., None], p, best)
    n = np.cross(B - A, Cc - A)
    nn = (n * n).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = (A * n).sum(-1) / nn                                    # the origin's foot point is h n
        foot = h[..., None] * n
        inside = nn > 0
        for P, e in ((A, B - A), (B, Cc - B), (Cc, A - Cc)):        # on the inner side of all three edges
            inside &= (np.cross(e, foot - P) * n).sum(-1) > 0
        e2 = h * h * nn
    lower = inside & (e2 < d2)
    d2, best = np.where(lower, e2, d2), np.where(lower[..., None], foot, best)
    return d2, best + q


_f = np.float32


def _fma(x, y, z):
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(_f)


def _dot32(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, ax * bx))


def _det32(u0, v1, u1, v0):
    return _fma(u0, v1, -(u1 * v0))


def _segment32(P, e):
    ee = _dot32(*e, *e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, -_dot32(*P, *e) / ee, _f(0))
    t = np.where(t > 0, np.where(t < 1, t, _f(1)), _f(0)).astype(_f)
    p = [_fma(t, e[k], P[k]) for k in range(3)]
    return _dot32(*p, *p), p


def triangle32(q, a, b, c):
    """(d2, closest) float32: the header's steps, one NumPy operation per rounding (rows of queries and triangles)."""
    q, a, b, c = np.broadcast_arrays(*(np.asarray(x, _f) for x in (q, a, b, c)))
    col = lambda m: [np.ascontiguousarray(m[..., k]) for k in range(3)]
    q3 = col(q)
    A, B, Cc = ([v[k] - q3[k] for k in range(3)] for v in (col(a), col(b), col(c)))
    ab, bc, ca = [B[k] - A[k] for k in range(3)], [Cc[k] - B[k] for k in range(3)], [A[k] - Cc[k] for k in range(3)]
    d2, best = _segment32(A, ab)
    for P, e in ((B, bc), (Cc, ca)):
        e2, p = _segment32(P, e)
        lower = e2 < d2
        d2, best = np.where(lower, e2, d2), [np.where(lower, p[k], best[k]) for k in range(3)]
    n = [_det32(ca[1], ab[2], ca[2], ab[1]), _det32(ca[2], ab[0], ca[0], ab[2]), _det32(ca[0], ab[1], ca[1], ab[0])]
    cross = lambda P, e: (_det32(P[1], e[2], P[2], e[1]), _det32(P[2], e[0], P[0], e[2]), _det32(P[0], e[1], P[1], e[0]))
    va, vb, vc = _dot32(*n, *cross(B, bc)), _dot32(*n, *cross(Cc, ca)), _dot32(*n, *cross(A, ab))
    inside = (va > 0) & (vb > 0) & (vc > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (va + vb) + vc
        wa, wb, wc = va / s, vb / s, vc / s
        p = [_fma(wc, Cc[k], _fma(wb, B[k], wa * A[k])) for k in range(3)]
        # one line search along the longest edge, clamped so that the point stays inside
        lab, lbc, lca = _dot32(*ab, *ab), _dot32(*bc, *bc), _dot32(*ca, *ca)
        use_ab = (lab >= lbc) & (lab >= lca)
        use_bc = ~use_ab & (lbc >= lca)
        pick = lambda x_ab, x_bc, x_ca: np.where(use_ab, x_ab, np.where(use_bc, x_bc, x_ca))
        e = [pick(ab[k], bc[k], ca[k]) for k in range(3)]
        ee, lo, hi = pick(lab, lbc, lca), pick(-wb, -wc, -wa), pick(wa, wb, wc)
        t = -_dot32(*p, *e) / ee
        t = np.where(t < lo, lo, np.where(t > hi, hi, t)).astype(_f)
        p = [_fma(t, e[k], p[k]) for k in range(3)]
        e2 = _dot32(*p, *p)
    lower = inside & (e2 < d2)
    d2, best = np.where(lower, e2, d2), [np.where(lower, p[k], best[k]) for k in range(3)]
    return d2.astype(_f), np.stack([best[k] + q3[k] for k in range(3)], -1).astype(_f)


def error_colors(d2, truncation):
    """(M,3) uint8: the header's colour rule, float32."""
    d2 = np.asarray(d2, _f)
    with np.errstate(invalid="ignore"):
        t = (np.sqrt(d2) / _f(truncation)).astype(_f)
        L = np.where(t >= 1, 255, (np.where(t < 1, t, _f(0)) * _f(256)).astype(np.int64))
    rgb = np.where((L <= 127)[:, None], np.stack([2 * L, np.full_like(L, 255), 0 * L], 1),
                   np.stack([np.full_like(L, 255), 2 * (255 - L), 0 * L], 1))
    rgb = np.where((t == t)[:, None], rgb, np.array([0, 0, 255]))
    return rgb.astype(np.uint8)


def mesh64(points, vertices, faces, chunk=64):
    """(d2 (M,) float64, face (M,) int64): the float64 minimum over ALL faces and the lowest face attaining it."""
    points, v = np.asarray(points, np.float64), np.asarray(vertices, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    d2, face = np.empty(len(points)), np.empty(len(points), np.int64)
    for i in range(0, len(points), chunk):
        all_d2, _ = triangle64(points[i:i + chunk, None, :], a[None], b[None], c[None])
        face[i:i + chunk] = all_d2.argmin(1)
        d2[i:i + chunk] = all_d2.min(1)
    return d2, face


# ---- the header on the host --------------------------------------------------------------------------------------------
_DRIVER = r'''
#include "sls_meshdist_math.h"
/* rows of 12 floats: q, a, b, c -> d2[n], closest[3 n] */
void md_triangles(int n, const float *rows, float *d2, float *closest)
{
    for (int i = 0; i < n; ++i) {
        const float *r = rows + 12 * (long)i;
        d2[i] = sls_meshdist_triangle(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], closest + 3 * (long)i);
    }
}
/* the same without the closest point: the null pointer's path */
void md_triangles_d2(int n, const float *rows, float *d2)
{
    for (int i = 0; i < n; ++i) {
        const float *r = rows + 12 * (long)i;
        d2[i] = sls_meshdist_triangle(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], 0);
    }
}
void md_colors(int n, const float *d2, float truncation, uint8_t *rgb)
{
    for (int i = 0; i < n; ++i) sls_error_color(d2[i], truncation, rgb + 3 * (long)i);
}
'''

_KEEP = []


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp = C.c_void_p
        lib.md_triangles.argtypes = [C.c_int, vp, vp, vp]
        lib.md_triangles_d2.argtypes = [C.c_int, vp, vp]
        lib.md_colors.argtypes = [C.c_int, vp, C.c_float, vp]

    def triangles(self, q, a, b, c):
        """(d2 (n,), closest (n,3)) float32 of the header for rows of queries and triangles."""
        rows = np.ascontiguousarray(np.concatenate(np.broadcast_arrays(*(np.asarray(x, _f) for x in (q, a, b, c))), axis=1))
        n = len(rows)
        d2, closest, d2b = np.empty(n, _f), np.empty((n, 3), _f), np.empty(n, _f)
        self.lib.md_triangles(n, rows.ctypes.data, d2.ctypes.data, closest.ctypes.data)
        self.lib.md_triangles_d2(n, rows.ctypes.data, d2b.ctypes.data)
        assert np.array_equal(d2.view(np.uint32), d2b.view(np.uint32))
        return d2, closest

    def colors(self, d2, truncation):
        d2 = np.ascontiguousarray(d2, _f)
        rgb = np.empty((len(d2), 3), np.uint8)
        self.lib.md_colors(len(d2), d2.ctypes.data, float(truncation), rgb.ctypes.data)
        return rgb


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="meshdist_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "meshdist_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libmeshdist_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- shared test inputs ------------------------------------------------------------------------------------------------
def random_cases(n, seed, sliver_share=0.25):
    """(q, a, b, c) float32 (n,3) each: coordinates up to 64 m, triangle sizes 1 cm to 10 m (log-uniform), a share of them
    slivers of height 1e-4 of their size; the query anywhere from on the triangle to 10 sizes away."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-2, 1, (n, 1))
    a = rng.uniform(-54, 54, (n, 3))
    e0, e1 = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))
    e0 /= np.linalg.norm(e0, axis=1, keepdims=True)
    e1 -= (e1 * e0).sum(1, keepdims=True) * e0
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    height = np.where(rng.random((n, 1)) < sliver_share, 1e-4, rng.uniform(0.1, 1.0, (n, 1)))
    b = a + size * e0
    c = a + size * (rng.uniform(-0.5, 1.5, (n, 1)) * e0 + height * e1)
    w = rng.dirichlet((1, 1, 1), n)
    on = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    away = rng.normal(0, 1, (n, 3)) * size * 10.0 ** rng.uniform(-3, 1, (n, 1)) * (rng.random((n, 1)) < 0.9)
    q = on + away
    return tuple(np.clip(x, -64, 64).astype(_f) for x in (q, a, b, c))


@functools.lru_cache(maxsize=None)
def grid_mesh(n=92, step=0.125):
    """(vertices, faces) read-only: an n x n grid of quads in z = 0.5 x, two triangles each (92: 16 928 faces, more than
    64 boxes of 256), the faces in a seeded random order so that curve order is not input order."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i * step, j * step, 0.5 * i * step], -1).reshape(-1, 3).astype(_f)
    k = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([k, k + n + 1, k + 1], 1), np.stack([k + 1, k + n + 1, k + n + 2], 1)]).astype(np.int32)
    f = f[np.random.default_rng(n).permutation(len(f))]
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def queries_for(vertices, faces, m, seed):
    """(m,3) float32: on the surface, near it, inside the bounding box, and 100 extents away, in turn."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max()) or 1.0
    tri = v[np.asarray(faces)[rng.integers(0, len(faces), m)]]
    w = rng.dirichlet((1, 1, 1), m)
    on = (w[:, :, None] * tri).sum(1)
    kind = np.arange(m) % 4
    q = np.where((kind == 0)[:, None], on, 0)
    q = np.where((kind == 1)[:, None], on + rng.normal(0, 0.01 * ext, (m, 3)), q)
    q = np.where((kind == 2)[:, None], rng.uniform(lo, hi + 1e-9, (m, 3)), q)
    q = np.where((kind == 3)[:, None], lo + rng.normal(0, 1, (m, 3)) * 100 * ext, q)
    return q.astype(_f)
