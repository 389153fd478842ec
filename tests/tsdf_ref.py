"""Reference side of the TSDF volume ("TSDF volume"; sls_tsdf_blocks / _integrate / _extract) — shared
by tests/test_tsdf_math.py, tests/test_tsdf_host.py (CPU) and tests/test_tsdf.py (GPU).  Not a test module.

NumPy restatements written from the rules of the contract, not from the kernels: the block keys in float64 and Python
integers, the integration in float64, the extraction in float32 element-wise NumPy operations (each rounded once, so its
bits are comparable) with the 16 tetrahedron cases rebuilt from the even-permutation rule.  `host()` compiles
include/sls_tsdf_math.h as plain C99 with -ffp-contract=off into a small shared library and runs the header itself on the
host: what the device results are compared with bit for bit."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = 1 << 20


# ---- block keys ------------------------------------------------------------------------------------------------------
def block_key(b):
    b = np.asarray(b, dtype=np.int64)
    return (b[..., 0] + BIAS) | ((b[..., 1] + BIAS) << 21) | ((b[..., 2] + BIAS) << 42)


def blocks_of_points(points, voxel_size, trunc, origin=(0.0, 0.0, 0.0)):
    """((B,3) int32 in ascending key order, n_nonfinite, n_out_of_range): every block the box [p - m, p + m] touches,
    m = trunc + voxel_size: per axis the indices floor((c - origin) / (8 voxel_size)) of c = p - m, p, p + m in float64."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float64)
    m = np.float64(trunc) + np.float64(voxel_size)
    finite = np.isfinite(p).all(1)
    q = p[finite]
    with np.errstate(over="ignore", invalid="ignore"):
        lo = np.floor(((q - m) - o) / (8.0 * np.float64(voxel_size)))
        hi = np.floor(((q + m) - o) / (8.0 * np.float64(voxel_size)))
        mid = np.floor((q - o) / (8.0 * np.float64(voxel_size)))
    ok = ((lo > -BIAS) & (lo < BIAS) & (hi > -BIAS) & (hi < BIAS)).all(1)
    lo, mid, hi = lo[ok].astype(np.int64), mid[ok].astype(np.int64), hi[ok].astype(np.int64)
    found = set()
    for l, c, h in zip(lo.tolist(), mid.tolist(), hi.tolist()):
        found.update(itertools.product(*({l[a], c[a], h[a]} for a in range(3))))
    order = sorted(found, key=lambda b: (b[0] + BIAS) | ((b[1] + BIAS) << 21) | ((b[2] + BIAS) << 42))
    return np.array(order, dtype=np.int32).reshape(-1, 3), int((~finite).sum()), int((~ok).sum())


def shell_blocks(centre, radius, voxel_size, trunc, origin=(0.0, 0.0, 0.0)):
    """All blocks a spherical shell of half thickness trunc + 2 voxels touches, in key order (from a dense scan of voxel
    centres: independent of the point rule)."""
    o, c = np.asarray(origin, np.float64), np.asarray(centre, np.float64)
    reach = radius + trunc + 4 * voxel_size
    lo = np.floor((c - reach - o) / (8 * voxel_size)).astype(int)
    hi = np.floor((c + reach - o) / (8 * voxel_size)).astype(int)
    out = []
    for b in itertools.product(*(range(lo[a], hi[a] + 1) for a in range(3))):
        d = np.linalg.norm(voxel_centres(np.array([b], np.int32), voxel_size, origin).astype(np.float64)[0] - c, axis=1)
        if (np.abs(d - radius) <= trunc + 2 * voxel_size).any():
            out.append(b)
    out.sort(key=lambda b: (b[0] + BIAS) | ((b[1] + BIAS) << 21) | ((b[2] + BIAS) << 42))
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def centre_axis(g, origin_a, voxel_size):
    """(float)(origin + (g + 0.5) voxel_size) of integer global voxel coordinates g, float64 rounded once."""
    return (np.float64(origin_a) + (np.asarray(g, dtype=np.float64) + 0.5) * np.float64(voxel_size)).astype(np.float32)


def voxel_centres(blocks, voxel_size, origin=(0.0, 0.0, 0.0)):
    """(B,512,3) float32: voxel l = x | y << 3 | z << 6."""
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    l = np.arange(512)
    local = np.stack([l & 7, (l >> 3) & 7, l >> 6], 1)
    g = 8 * b[:, None, :] + local[None]
    return np.stack([centre_axis(g[..., a], origin[a], voxel_size) for a in range(3)], -1)


# ---- integration, float64 --------------------------------------------------------------------------------------------
def project(centres, cam):
    """float64 (rho, u, v) of float32 voxel centres under cam = dict(R (3,3) f32, t (3,) f32, fx, fy, cx, cy f32, ...)."""
    c = np.asarray(centres, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    q = c @ np.asarray(cam["R"], np.float32).astype(np.float64).reshape(3, 3).T + np.asarray(cam["t"], np.float32).astype(np.float64)
    rho = np.linalg.norm(q, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        az = np.arctan2(q[:, 1], q[:, 0])
        el = np.arcsin(np.clip(q[:, 2] / rho, -1.0, 1.0))
    u = np.float64(np.float32(cam["fx"])) * az + np.float64(np.float32(cam["cx"]))
    v = np.float64(np.float32(cam["fy"])) * el + np.float64(np.float32(cam["cy"]))
    return rho, u, v


def integrate(tsdf, weight, blocks, allmap, cam, voxel_size, trunc, origin, min_opacity, max_depth_dist, depth_ratio):
    """One keyframe into float64 copies of (tsdf, weight) (B,512).  Returns (tsdf, weight, edge) with edge (B,512) the
    distance in pixels of the voxel's float64 image coordinate from the nearest pixel boundary (the smaller of both axes;
    inf for a voxel below the near cut): the comparison with float32 results leaves out the voxels with a small one."""
    am = np.asarray(allmap, dtype=np.float32)
    _, H, W = am.shape
    B = len(blocks)
    tsdf, weight = np.array(tsdf, dtype=np.float64).reshape(B, 512), np.array(weight, dtype=np.float64).reshape(B, 512)
    rho, u, v = project(voxel_centres(blocks, voxel_size, origin), cam)
    near = rho >= np.float64(np.float32(cam["near_cut"]))
    with np.errstate(invalid="ignore"):
        edge = np.minimum(np.abs(u - np.round(u)), np.abs(v - np.round(v)))
        cf, rf = np.floor(u + 1.0), np.floor(v + 1.0)
    edge = np.where(near, edge, np.inf).reshape(B, 512)
    ok = near & np.isfinite(cf) & np.isfinite(rf)
    c = np.where(ok, cf, 0).astype(np.int64)
    r = np.where(ok, rf, -1).astype(np.int64)
    if cam["wrap"]:
        c = np.mod(c, W)
    ok &= (c >= 0) & (c < W) & (r >= 0) & (r < H)
    px = np.where(ok, r * W + c, 0)
    flat = am.reshape(7, -1)
    D, alpha, med, dist = (flat[k][px] for k in (0, 1, 5, 6))
    with np.errstate(invalid="ignore", divide="ignore"):
        ok &= ~(alpha < np.float32(min_opacity)) & ~(dist > np.float32(max_depth_dist))
        a64 = alpha.astype(np.float64)
        Dh = np.where(a64 > 0, D.astype(np.float64) / np.where(a64 > 0, a64, 1.0), D.astype(np.float64))
        ratio = np.float64(np.float32(depth_ratio))
        depth = Dh * (1.0 - ratio) + med.astype(np.float64) * ratio
        ok &= depth > 0
        sdf = depth - rho
        tr = np.float64(np.float32(trunc))
        ok &= sdf >= -tr
        t = np.minimum(1.0, sdf / tr)
    ok = ok.reshape(B, 512)
    t = t.reshape(B, 512)
    new = (tsdf * weight + t) / (weight + 1.0)
    return np.where(ok, new, tsdf), np.where(ok, weight + 1.0, weight), edge


# ---- extraction, float32 ---------------------------------------------------------------------------------------------
PERMS = list(itertools.permutations(range(3)))                          # lexicographic: tetrahedron t
LONE = {0: (0, 1, 2, 3), 1: (1, 0, 3, 2), 2: (2, 0, 1, 3), 3: (3, 0, 2, 1)}
PAIR = {(0, 1): (0, 1, 2, 3), (0, 2): (0, 2, 3, 1), (0, 3): (0, 3, 1, 2), (1, 2): (1, 2, 0, 3), (1, 3): (1, 3, 2, 0), (2, 3): (2, 3, 0, 1)}


def tet_corners(t):
    """(cube corners of tetrahedron t, +1 / -1 its orientation)"""
    a, b, c = PERMS[t]
    v = (0, 1 << a, (1 << a) | (1 << b), 7)
    e = np.array([[(x >> k) & 1 for k in range(3)] for x in v], dtype=np.float64)
    return v, int(round(np.linalg.det(e[1:] - e[0])))


def tet_case(mask):
    """The triangles of a positively oriented tetrahedron whose corners in `mask` are inside: a list of triangles, each
    three edges (i, j) of tetrahedron corners."""
    inside = [i for i in range(4) if (mask >> i) & 1]
    if len(inside) in (0, 4):
        return []
    if len(inside) == 1:
        i, a, b, c = LONE[inside[0]]
        return [[(i, a), (i, b), (i, c)]]
    if len(inside) == 3:
        i, a, b, c = LONE[[x for x in range(4) if x not in inside][0]]
        return [[(i, a), (i, c), (i, b)]]
    i, j, k, l = PAIR[tuple(inside)]
    return [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]


def corner_tiles(blocks, tsdf, weight):
    """(B,9,9,9) tiles [z, y, x] of tsdf and weight; weight -1 where the corner's block is absent."""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    B = len(blocks)
    index = {tuple(b): k for k, b in enumerate(blocks.tolist())}
    t = np.asarray(tsdf, dtype=np.float32).reshape(B, 8, 8, 8)
    w = np.asarray(weight, dtype=np.float32).reshape(B, 8, 8, 8)
    T = np.zeros((B, 9, 9, 9), np.float32)
    Wt = np.full((B, 9, 9, 9), -1.0, np.float32)
    for k, b in enumerate(blocks.tolist()):
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            nb = index.get((b[0] + dx, b[1] + dy, b[2] + dz))
            if nb is None:
                continue
            sz, sy, sx = (slice(8, 9) if d else slice(0, 8) for d in (dz, dy, dx))
            fz, fy, fx = (slice(0, 1) if d else slice(0, 8) for d in (dz, dy, dx))
            T[k, sz, sy, sx] = t[nb, fz, fy, fx]
            Wt[k, sz, sy, sx] = w[nb, fz, fy, fx]
    return T, Wt


def extract(blocks, tsdf, weight, voxel_size, origin=(0.0, 0.0, 0.0), min_weight=1.0):
    """(T,3,3) float32 triangles in the order block, cube, tetrahedron, triangle; (B,) their number per block."""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    B = len(blocks)
    if B == 0:
        return np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.int64)
    T, Wt = corner_tiles(blocks, tsdf, weight)
    f = np.stack([T[:, (j >> 2):(j >> 2) + 8, ((j >> 1) & 1):((j >> 1) & 1) + 8, (j & 1):(j & 1) + 8] for j in range(8)], -1).reshape(B * 512, 8)
    w = np.stack([Wt[:, (j >> 2):(j >> 2) + 8, ((j >> 1) & 1):((j >> 1) & 1) + 8, (j & 1):(j & 1) + 8] for j in range(8)], -1).reshape(B * 512, 8)
    with np.errstate(invalid="ignore"):
        observed = (w >= np.float32(min_weight)).all(1) & ~np.isnan(f).any(1)
    l = np.arange(512)
    g = (8 * blocks[:, None, :] + np.stack([l & 7, (l >> 3) & 7, l >> 6], 1)[None]).reshape(B * 512, 3)
    c0 = np.stack([centre_axis(g[:, a], origin[a], voxel_size) for a in range(3)], 1)
    c1 = np.stack([centre_axis(g[:, a] + 1, origin[a], voxel_size) for a in range(3)], 1)
    tris, keys = [], []
    for t in range(6):
        v, orient = tet_corners(t)
        mask = sum(((f[:, v[i]] < 0) & observed).astype(np.int64) << i for i in range(4))
        for m in range(1, 15):
            rows = np.flatnonzero(mask == m)
            if rows.size == 0:
                continue
            for n, tri in enumerate(tet_case(m)):
                if orient < 0:
                    tri = [tri[0], tri[2], tri[1]]
                verts = []
                for (i, j) in tri:
                    A, Bc = sorted((v[i], v[j]))
                    tA, tB = f[rows, A], f[rows, Bc]
                    s = (tA / (tA - tB)).astype(np.float32)
                    pa = np.where([(A >> k) & 1 for k in range(3)], c1[rows], c0[rows])
                    pb = np.where([(Bc >> k) & 1 for k in range(3)], c1[rows], c0[rows])
                    verts.append((pa + (s[:, None] * (pb - pa).astype(np.float32)).astype(np.float32)).astype(np.float32))
                tris.append(np.stack(verts, 1))
                keys.append(rows * 12 + t * 2 + n)
    if not tris:
        return np.zeros((0, 3, 3), np.float32), np.zeros((B,), np.int64)
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    counts = np.bincount(keys // (12 * 512), minlength=B)
    return np.ascontiguousarray(tris[order]), counts


# ---- mesh checks -----------------------------------------------------------------------------------------------------
def weld(tris):
    """(vertices (V,3) float32, faces (T,3)) with bit-equal vertices merged."""
    bits = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3).view(np.uint32)
    uniq, inv = np.unique(bits, axis=0, return_inverse=True)
    return uniq.view(np.float32), inv.reshape(-1, 3)


def manifold_report(tris):
    """dict(V, E, F, bad_edges: undirected edges not used exactly twice in opposite directions, degenerate: faces with a
    repeated vertex) of a triangle soup, vertices compared by their bits."""
    vertices, faces = weld(tris)
    degenerate = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0])
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    V = len(vertices)
    fwd = d[:, 0] * V + d[:, 1]
    und = np.minimum(d[:, 0], d[:, 1]) * V + np.maximum(d[:, 0], d[:, 1])
    uu, cu = np.unique(und, return_counts=True)
    uf, cf = np.unique(fwd, return_counts=True)
    bad = int((cu != 2).sum()) + int((cf != 1).sum())
    return {"V": V, "E": len(uu), "F": len(faces), "bad_edges": bad, "degenerate": int(degenerate.sum())}


def sphere_volume(centre, radius, voxel_size, trunc, origin=(0.0, 0.0, 0.0)):
    """(blocks, tsdf (B,512) float32, weight (B,512) float32) of a sphere: tsdf = min(1, max(-1, (|c - centre| - radius)
    / trunc)) at every voxel centre (positive outside), weight 1, all blocks the shell touches."""
    blocks = shell_blocks(centre, radius, voxel_size, trunc, origin)
    c = voxel_centres(blocks, voxel_size, origin).astype(np.float64)
    d = np.linalg.norm(c - np.asarray(centre, np.float64), axis=2) - radius
    tsdf = np.clip(d / trunc, -1.0, 1.0).astype(np.float32)
    return blocks, tsdf, np.ones_like(tsdf)


# ---- the header on the host ------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <string.h>
#include "sls_tsdf_math.h"

int ref_point_keys(int M, const float *xyz, const double *origin, double voxel_size, double margin, uint64_t *keys, int *ok)
{
    for (int i = 0; i < M; ++i) ok[i] = sls_tsdf_point_keys(xyz + 3 * i, origin, voxel_size, margin, keys + SLS_TSDF_POINT_KEYS * (size_t)i);
    return 0;
}

void ref_key_block(uint64_t key, int32_t *b) { sls_tsdf_key_block(key, b); }
uint64_t ref_key(int32_t x, int32_t y, int32_t z) { return sls_tsdf_key(x, y, z); }
uint32_t ref_tet_case(int mask) { return sls_tet_case(mask); }
int ref_tet_corners(int t, int *v) { return sls_tet_corners(t, v); }

void ref_integrate(int B, const int32_t *blocks, float *tsdf, float *weight, const float *allmap, int H, int W, int wrap,
                   const float *K4, float near_cut, const float *R, const float *t, const double *origin, double voxel_size,
                   float min_opacity, float max_depth_dist, float depth_ratio, float trunc, int32_t *pixel_out)
{
    const size_t P = (size_t)H * (size_t)W;
    for (int k = 0; k < B; ++k)
        for (int l = 0; l < 512; ++l) {
            float c[3], q[3];
            const size_t slot = (size_t)k * 512 + l;
            c[0] = sls_tsdf_centre(8 * blocks[3 * k] + (l & 7), origin[0], voxel_size);
            c[1] = sls_tsdf_centre(8 * blocks[3 * k + 1] + ((l >> 3) & 7), origin[1], voxel_size);
            c[2] = sls_tsdf_centre(8 * blocks[3 * k + 2] + (l >> 6), origin[2], voxel_size);
            const float rho = sls_tsdf_view(R, t, c, q);
            if (pixel_out) pixel_out[slot] = -1;
            if (!(rho >= near_cut) || !(rho > 0.0f) || !(rho <= 3.0e38f)) continue;
            const int32_t px = sls_tsdf_pixel(q, rho, K4[0], K4[1], K4[2], K4[3], H, W, wrap);
            if (pixel_out) pixel_out[slot] = px;
            if (px < 0) continue;
            sls_tsdf_update(allmap[px], allmap[P + px], allmap[5 * P + px], allmap[6 * P + px], rho, min_opacity, max_depth_dist,
                            depth_ratio, trunc, tsdf + slot, weight + slot);
        }
}

static int find_block(int B, const int32_t *blocks, int32_t x, int32_t y, int32_t z)
{
    for (int k = 0; k < B; ++k) if (blocks[3 * k] == x && blocks[3 * k + 1] == y && blocks[3 * k + 2] == z) return k;
    return -1;
}

/* out: null (count only) or room for the triangles; counts: B ints.  Returns the total. */
long ref_extract(int B, const int32_t *blocks, const float *tsdf, const float *weight, float min_weight, const double *origin,
                 double voxel_size, int *counts, float *out)
{
    long total = 0;
    for (int k = 0; k < B; ++k) {
        int nb[8];
        for (int j = 0; j < 8; ++j) nb[j] = find_block(B, blocks, blocks[3 * k] + (j & 1), blocks[3 * k + 1] + ((j >> 1) & 1), blocks[3 * k + 2] + (j >> 2));
        counts[k] = 0;
        for (int l = 0; l < 512; ++l) {
            const int x = l & 7, y = (l >> 3) & 7, z = l >> 6;
            float f[8], c0[3], c1[3];
            int observed = 1;
            for (int j = 0; j < 8; ++j) {
                const int cx = x + (j & 1), cy = y + ((j >> 1) & 1), cz = z + (j >> 2);
                const int n = nb[(cx >> 3) | ((cy >> 3) << 1) | ((cz >> 3) << 2)];
                if (n < 0) { observed = 0; f[j] = 0.0f; continue; }
                const size_t slot = (size_t)n * 512 + ((cx & 7) | ((cy & 7) << 3) | ((cz & 7) << 6));
                f[j] = tsdf[slot];
                if (!(weight[slot] >= min_weight) || f[j] != f[j]) observed = 0;
            }
            if (!observed) continue;
            const int32_t g[3] = { 8 * blocks[3 * k] + x, 8 * blocks[3 * k + 1] + y, 8 * blocks[3 * k + 2] + z };
            for (int d = 0; d < 3; ++d) { c0[d] = sls_tsdf_centre(g[d], origin[d], voxel_size); c1[d] = sls_tsdf_centre(g[d] + 1, origin[d], voxel_size); }
            const int n = sls_tsdf_cube(f, c0, c1, out ? out + 9 * total : (float *)0);
            counts[k] += n;
            total += n;
        }
    }
    return total;
}
'''


class Host:
    """include/sls_tsdf_math.h compiled as plain C and called through ctypes."""

    def __init__(self, lib):
        self.lib = lib
        lib.ref_key.restype = C.c_uint64
        lib.ref_key.argtypes = [C.c_int32] * 3
        lib.ref_key_block.argtypes = [C.c_uint64, C.c_void_p]
        lib.ref_tet_case.restype = C.c_uint32
        lib.ref_tet_case.argtypes = [C.c_int]
        lib.ref_tet_corners.argtypes = [C.c_int, C.c_void_p]
        lib.ref_point_keys.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        lib.ref_integrate.restype = None
        lib.ref_integrate.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                                  C.c_double] + [C.c_float] * 4 + [C.c_void_p]
        lib.ref_extract.restype = C.c_long
        lib.ref_extract.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]

    def point_keys(self, points, voxel_size, trunc, origin=(0.0, 0.0, 0.0)):
        """(keys (M,27) uint64, ok (M,) bool) of FINITE points."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        keys = np.zeros((len(p), 27), np.uint64)
        ok = np.zeros((len(p),), np.int32)
        self.lib.ref_point_keys(len(p), p.ctypes.data, o.ctypes.data, float(voxel_size), float(trunc) + float(voxel_size), keys.ctypes.data,
                                ok.ctypes.data)
        return keys, ok.astype(bool)

    def blocks_of_points(self, points, voxel_size, trunc, origin=(0.0, 0.0, 0.0)):
        """What sls_tsdf_blocks must return: ((B,3) int32, n_nonfinite, n_out_of_range)."""
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        finite = np.isfinite(p).all(1)
        keys, ok = self.point_keys(p[finite], voxel_size, trunc, origin)
        uniq = np.unique(keys[ok].reshape(-1))
        out = np.zeros((len(uniq), 3), np.int32)
        for i, k in enumerate(uniq.tolist()):
            self.lib.ref_key_block(k, out[i].ctypes.data)
        return out, int((~finite).sum()), int((~ok).sum())

    def integrate(self, blocks, tsdf, weight, allmap, cam, voxel_size, trunc, origin, min_opacity, max_depth_dist, depth_ratio):
        """One keyframe into float32 copies of (tsdf, weight); also the pixel of every voxel (-1: none)."""
        blocks = np.ascontiguousarray(blocks, dtype=np.int32)
        B = len(blocks)
        tsdf, weight = np.array(tsdf, dtype=np.float32).reshape(B, 512), np.array(weight, dtype=np.float32).reshape(B, 512)
        am = np.ascontiguousarray(allmap, dtype=np.float32)
        K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
        R, t = np.ascontiguousarray(cam["R"], dtype=np.float32).reshape(9), np.ascontiguousarray(cam["t"], dtype=np.float32)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        pixel = np.zeros((B, 512), np.int32)
        self.lib.ref_integrate(B, blocks.ctypes.data, tsdf.ctypes.data, weight.ctypes.data, am.ctypes.data, am.shape[1], am.shape[2],
                               int(cam["wrap"]), K4.ctypes.data, float(cam["near_cut"]), R.ctypes.data, t.ctypes.data, o.ctypes.data,
                               float(voxel_size), float(min_opacity), float(max_depth_dist), float(depth_ratio), float(np.float32(trunc)),
                               pixel.ctypes.data)
        return tsdf, weight, pixel

    def extract(self, blocks, tsdf, weight, voxel_size, origin=(0.0, 0.0, 0.0), min_weight=1.0):
        """((T,3,3) float32, (B,) counts)"""
        blocks = np.ascontiguousarray(blocks, dtype=np.int32)
        B = len(blocks)
        tsdf, weight = np.ascontiguousarray(tsdf, dtype=np.float32), np.ascontiguousarray(weight, dtype=np.float32)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        counts = np.zeros((max(B, 1),), np.int32)
        T = self.lib.ref_extract(B, blocks.ctypes.data, tsdf.ctypes.data, weight.ctypes.data, float(min_weight), o.ctypes.data,
                                 float(voxel_size), counts.ctypes.data, None)
        out = np.zeros((T, 3, 3), np.float32)
        self.lib.ref_extract(B, blocks.ctypes.data, tsdf.ctypes.data, weight.ctypes.data, float(min_weight), o.ctypes.data,
                             float(voxel_size), counts.ctypes.data, out.ctypes.data)
        return out, counts[:B].astype(np.int64)


_KEEP = []


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="tsdf_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "tsdf_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libtsdf_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- shared test inputs ----------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    t = np.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def spherical_cam(H, W, hfov_deg, vfov_deg, R, t, near_cut=0.2):
    """The camera dictionary of `project` / `Host.integrate`: u = fx az + cx with az = +hfov/2 at the left image edge
    (fx < 0, as the project's spherical intrinsics), wrap for a 360-degree image."""
    hf, vf = np.radians(hfov_deg), np.radians(vfov_deg)
    return {"fx": np.float32(-W / hf), "fy": np.float32(-H / vf), "cx": np.float32(W / 2.0), "cy": np.float32(H / 2.0),
            "R": np.asarray(R, np.float32), "t": np.asarray(t, np.float32), "wrap": int(hfov_deg >= 359.9), "near_cut": np.float32(near_cut)}


@functools.lru_cache(maxsize=None)
def synthetic_allmap(H, W, seed=0):
    """Alpha in {0, 0.3, 1}, dist on both sides of 0.1, a per-pixel depth around 2 m with a step in the image's right half,
    a median plane 5 cm behind D / alpha.  Read-only."""
    rng = np.random.default_rng(1000 + seed)
    am = np.zeros((7, H, W), np.float32)
    alpha = rng.choice(np.array([0.0, 0.3, 1.0], np.float32), size=(H, W), p=[0.1, 0.1, 0.8])
    depth = (2.0 + 0.15 * rng.uniform(-1, 1, (H, W))).astype(np.float32)
    depth[:, W // 2:] += np.float32(0.6)
    am[0] = depth * alpha
    am[1] = alpha
    am[2:5] = rng.uniform(-1, 1, (3, H, W))
    am[5] = depth + np.float32(0.05)
    am[6] = np.where(rng.uniform(size=(H, W)) < 0.15, 0.15, 0.05)
    am.setflags(write=False)
    return am


# ---- cases and checks shared by the CPU and the GPU tests -------------------------------------------------------------
VS = 0.125
TRUNC = 4 * VS
CENTRE = np.array([0.137, -0.219, 0.071])                    # off the lattice
ORIGIN = (0.05, -0.02, 0.11)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def key_points():
    """Random points, points exactly on block faces (and one margin off them), negative coordinates, duplicates, a point
    beyond 2^20 blocks, non-finite points."""
    rng = np.random.default_rng(5)
    e = 8 * VS
    faces = np.array([[0, 0, 0], [e, 2 * e, -3 * e], [-e, -e, -e], [e + TRUNC + VS, 0, 0], [e - TRUNC - VS, e, e], [-5 * e, 7 * e, 0.5 * e]])
    pts = np.concatenate([rng.normal(0, 3, (300, 3)), faces, faces[:3], -np.abs(rng.normal(0, 20, (50, 3))),
                          [[1.2e6, 0, 0], [0, -1.1e6, 5], [3e38, 0, 0]], [[np.nan, 0, 0], [0, np.inf, 0]], rng.normal(0, 3, (5, 3))])
    return pts.astype(np.float32)


def check_sphere_mesh(tris, centre=CENTRE, radius=1.0, vs=VS):
    """Closed, oriented, of genus 0, normals outwards, every vertex within the linear-interpolation bound of the sphere."""
    rep = manifold_report(tris)
    print(f"V {rep['V']} E {rep['E']} F {rep['F']}: bad edges {rep['bad_edges']}, degenerate faces {rep['degenerate']}")
    assert rep["bad_edges"] == 0 and rep["degenerate"] == 0
    assert rep["V"] - rep["E"] + rep["F"] == 2
    t64 = np.asarray(tris, dtype=np.float64)
    n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    assert (np.einsum("ij,ij->i", n, t64.mean(1) - centre) > 0).all()
    err = np.abs(np.linalg.norm(t64.reshape(-1, 3) - centre, axis=1) - radius).max()
    bound = 3 * vs ** 2 / (8 * (1 - np.sqrt(3) * vs))
    print(f"radius error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def drop_cases(blocks, counts):
    """The block with the most triangles, for the missing-data tests."""
    return int(np.argmax(counts))


def touched_cubes(blocks, k):
    """Global voxel coordinates [lo, hi] per axis of the corners block k owns."""
    return 8 * blocks[k].astype(np.int64), 8 * blocks[k].astype(np.int64) + 7


def check_missing(full, part, blocks, k, vs, origin):
    """`part` (extracted without block k's data) = `full` minus exactly the triangles of cubes with a corner in block k, in
    order and bit for bit.  A triangle's cube: the voxel that holds the minimum corner of its vertices' bounding box."""
    o = np.asarray(origin, np.float64)
    lo, hi = touched_cubes(blocks, k)
    g = np.floor((full.astype(np.float64).min(1) - o) / vs - 0.5 + 1e-6).astype(np.int64)       # the cube of every triangle
    uses = ((g + 1 >= lo) & (g <= hi)).all(1)               # the cube's corners g .. g + 1 reach into block k
    assert 0 < uses.sum() < len(full)
    assert len(part) == int((~uses).sum())
    assert np.array_equal(bits(part), bits(full[~uses]))


H, W = 16, 64
POSES = [(rot([0.3, -0.5, 0.8], 37.0), np.array([0.11, -0.07, 0.05])), (rot([-0.6, 0.2, 0.5], 115.0), np.array([-0.23, 0.18, -0.04]))]


def integration_case(hfov, vfov):
    """(blocks, [camera of keyframe 0, camera of keyframe 1], [allmap 0, allmap 1]): about 60 blocks on a shell around rho = 2."""
    R0, t0 = POSES[0]
    eye = -R0.T @ t0                                         # the first camera's position in the volume's frame
    blocks = shell_blocks(eye, 2.1, VS, 0.2, ORIGIN)
    blocks = blocks[:: max(1, len(blocks) // 60)][:64]
    cams = [spherical_cam(H, W, hfov, vfov, R, t) for R, t in POSES]
    return blocks, cams, [synthetic_allmap(H, W, 0), synthetic_allmap(H, W, 1)]


def compare_with_float64(blocks, cams, maps, depth_ratio, got_t, got_w, what):
    """The float64 restatement of both keyframes in sequence against float32 results, at every voxel whose float64 image
    coordinate is farther than 1e-4 px from a pixel boundary on both axes in both keyframes; at most 1 % may be left out."""
    B = len(blocks)
    t64, w64 = np.ones((B, 512)), np.zeros((B, 512))
    keep = np.ones((B, 512), bool)
    for cam, am in zip(cams, maps):
        t64, w64, edge = integrate(t64, w64, blocks, am, cam, VS, TRUNC, ORIGIN, 0.5, 0.1, depth_ratio)
        keep &= edge > 1e-4
    excluded = 1.0 - keep.mean()
    err = np.abs(got_t.astype(np.float64) - t64)[keep].max()
    wrong_w = int((got_w.astype(np.float64) != w64)[keep].sum())
    print(f"{what}: {B * 512} voxels, {int((w64 > 0).sum())} observed, {int((w64 > 1).sum())} twice, excluded {100 * excluded:.3f} %, "
          f"tsdf error {err:.2e} of trunc, weights that differ {wrong_w}")
    assert excluded <= 0.01
    assert (w64 > 0).sum() > 2000 and (w64 > 1).sum() > 200 and (t64[w64 > 0] < 0).sum() > 200 and (w64 == 0).sum() > 200
    assert wrong_w == 0 and err <= 1e-5
