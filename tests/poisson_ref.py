"""Reference side of the Poisson volume ("Poisson volume"; sls_poisson_splat / _solve / _density) —
shared by tests/test_poisson_math.py (CPU) and tests/test_poisson.py (GPU).  Not a test module.

NumPy restatements written from the rules of include/sls_poisson_math.h, not from the kernels: float64 element-wise
operations on float32 data, each result rounded once, every sum in the header's stated order (np.add.at adds in the order
of its index array; the inner product is the butterfly's tree written with slices).  `host()` compiles the header as plain
C99 with -ffp-contract=off into a small shared library and runs its serial routines: what the device results are compared
with bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import tsdf_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = 1 << 20
FLAG_CONVERGED, FLAG_NOT_PD, FLAG_EMPTY = 1, 2, 4
STATUS_WORDS = 8
REDUCE = 512


# ---- the grid --------------------------------------------------------------------------------------------------------
def sort_blocks(blocks):
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    return np.ascontiguousarray(b[np.argsort(tsdf_ref.block_key(b))], dtype=np.int32)


def lookup(blocks, b):
    """index of every row of b (.., 3) in the sorted block list, -1 when absent"""
    keys = tsdf_ref.block_key(np.asarray(blocks, dtype=np.int64).reshape(-1, 3))
    b = np.asarray(b, dtype=np.int64)
    inside = (np.abs(b) < BIAS).all(-1)
    want = tsdf_ref.block_key(np.where(inside[..., None], b, 0))
    if len(keys) == 0:
        return np.full(want.shape, -1, np.int64)
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return np.where(inside & (keys[pos] == want), pos, -1)


def neighbour_slots(blocks):
    """(6, 512 B) int64: the slot of the voxel next to every voxel in the directions -x, +x, -y, +y, -z, +z; -1: absent"""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    B = len(blocks)
    l = np.arange(512)
    out = np.empty((6, B, 512), np.int64)
    for d in range(6):
        a, sh = d >> 1, 3 * (d >> 1)
        step = np.zeros(3, np.int64)
        step[a] = 1 if d & 1 else -1
        nb = lookup(blocks, blocks + step)                               # (B,)
        c = (l >> sh) & 7
        outside = (c == 7) if d & 1 else (c == 0)
        l2 = np.where(outside, l - (7 << sh) if d & 1 else l + (7 << sh), l + (1 << sh) if d & 1 else l - (1 << sh))
        k2 = np.where(outside[None], nb[:, None], np.arange(B)[:, None])
        out[d] = np.where(k2 >= 0, k2 * 512 + l2[None], -1)
    return out.reshape(6, B * 512)


# ---- 1. splat --------------------------------------------------------------------------------------------------------
def splat(points, normals, blocks, h, origin=(0.0, 0.0, 0.0)):
    """(field (B,512,4) float32, status (4,) uint32)"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    B = len(blocks)
    o, h = np.asarray(origin, dtype=np.float64), np.float64(h)
    finite = np.isfinite(p).all(1) & np.isfinite(n).all(1)
    with np.errstate(all="ignore"):
        u = (p.astype(np.float64) - o) / h - 0.5
        i = np.floor(u)
        ok = (np.abs(np.floor(i / 8.0)) < BIAS) & (np.abs(np.floor((i + 1.0) / 8.0)) < BIAS)
    in_range = finite & ok.all(1)
    i = np.where(in_range[:, None], i, 0.0)
    f = np.where(in_range[:, None], u - i, 0.0)
    cell = i.astype(np.int64)
    have_cell = in_range & (lookup(blocks, cell >> 3) >= 0)
    acc = np.zeros((B * 512, 4), np.float64)
    dropped = in_range & ~have_cell
    n64 = n.astype(np.float64)
    for c in range(8):
        d = np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64)
        node = cell + d
        k = lookup(blocks, node >> 3)
        dropped |= in_range & (k < 0)
        valid = have_cell & (k >= 0)
        slot = (k * 512 + ((node[:, 0] & 7) | (node[:, 1] & 7) << 3 | (node[:, 2] & 7) << 6))[valid]
        w3 = np.where(d[None] == 1, f, 1.0 - f)
        w = ((w3[:, 0] * w3[:, 1]) * w3[:, 2])[valid]
        for a in range(3):
            np.add.at(acc[:, a], slot, w * n64[valid, a])
        np.add.at(acc[:, 3], slot, w)
    status = np.array([(~finite).sum(), (finite & ~in_range).sum(), dropped.sum(), 1], np.uint32)
    return acc.astype(np.float32).reshape(B, 512, 4), status


# ---- 2. system -------------------------------------------------------------------------------------------------------
def system(blocks, field, alpha, nbr=None):
    """(b, diag) (B,512) float32"""
    nbr = neighbour_slots(blocks) if nbr is None else nbr
    F = np.asarray(field, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    s = np.zeros(len(F))
    deg = np.zeros(len(F))
    for d in range(6):
        has = nbr[d] >= 0
        Vn = F[np.maximum(nbr[d], 0), d >> 1]
        g = 0.5 * (Vn + F[:, d >> 1])
        s = np.where(has, s - g if d & 1 else s + g, s)
        deg += has
    diag = (deg + np.float64(alpha) * F[:, 3]).astype(np.float32)
    return s.astype(np.float32).reshape(-1, 512), diag.reshape(-1, 512)


def apply(nbr, diag, p):
    p64 = np.asarray(p, dtype=np.float32).reshape(-1).astype(np.float64)
    s = np.asarray(diag, dtype=np.float32).reshape(-1).astype(np.float64) * p64
    for d in range(6):
        s = np.where(nbr[d] >= 0, s - p64[np.maximum(nbr[d], 0)], s)
    return s.astype(np.float32).reshape(-1, 512)


# ---- the inner product -----------------------------------------------------------------------------------------------
def sum512(v):
    """(.., 512) float64 -> (..): the butterfly's tree over every 64, then the eight wave sums ascending"""
    v = np.asarray(v, dtype=np.float64).reshape(v.shape[:-1] + (8, 64))
    off = 32
    while off:
        v = v[..., :off] + v[..., off:2 * off]
        off >>= 1
    v = v[..., 0]
    s = v[..., 0]
    for w in range(1, 8):
        s = s + v[..., w]
    return s


def dot(a, b=None):
    a = np.asarray(a, dtype=np.float32).reshape(-1, 512).astype(np.float64)
    prod = a * (1.0 if b is None else np.asarray(b, dtype=np.float32).reshape(-1, 512).astype(np.float64))
    partials = sum512(prod)
    rounds = (len(partials) + REDUCE - 1) // REDUCE
    padded = np.zeros(max(rounds, 1) * REDUCE)
    padded[:len(partials)] = partials
    t = np.zeros(REDUCE)
    for row in padded.reshape(-1, REDUCE):
        t = t + row
    return float(sum512(t))


# ---- 3. and 4. solve, iso-level --------------------------------------------------------------------------------------
def bits64(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def solve(blocks, field, alpha=4.0, iterations=300, tol=1e-4):
    """dict(chi (B,512) float32, status (8,) uint64, vectors: b, diag, x, r, z, p, q)"""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    B = len(blocks)
    field = np.asarray(field, dtype=np.float32).reshape(B, 512, 4)
    nbr = neighbour_slots(blocks)
    b, diag = system(blocks, field, alpha, nbr)
    d64 = diag.astype(np.float64)
    x = np.zeros_like(b)
    r = b.copy()
    with np.errstate(all="ignore"):
        z = (r.astype(np.float64) / d64).astype(np.float32)
    p, q = z.copy(), np.zeros_like(b)
    bb = dot(b, b)
    rz, rr = dot(r, z), bb
    thr = (np.float64(tol) * np.float64(tol)) * bb
    flags = iters = 0
    ended = False
    if bb == 0.0:
        flags, ended = FLAG_CONVERGED | FLAG_EMPTY, True
    elif rr <= thr:
        flags, ended = FLAG_CONVERGED, True
    for _ in range(iterations):
        if ended:
            break
        q = apply(nbr, diag, p)
        pq = dot(p, q)
        if not (pq > 0.0 and np.isfinite(pq)):
            flags |= FLAG_NOT_PD
            break
        a = np.float64(rz) / np.float64(pq)
        with np.errstate(all="ignore"):
            x = (x.astype(np.float64) + a * p.astype(np.float64)).astype(np.float32)
            r = (r.astype(np.float64) - a * q.astype(np.float64)).astype(np.float32)
            z = (r.astype(np.float64) / d64).astype(np.float32)
        rr, rz2 = dot(r, r), dot(r, z)
        iters += 1
        if rr <= thr:
            flags |= FLAG_CONVERGED
            break
        beta = np.float64(rz2) / np.float64(rz)
        p = (z.astype(np.float64) + beta * p.astype(np.float64)).astype(np.float32)
        rz = rz2
    W = field[..., 3]
    wx, w1 = dot(W, x), dot(W)
    iso = 0.0 if w1 == 0.0 else float(np.float64(wx) / np.float64(w1))
    chi = (x.astype(np.float64) - iso).astype(np.float32)
    status = np.array([iters, flags, B, bits64(rr), bits64(bb), bits64(iso), bits64(w1), 0], np.uint64)
    return {"chi": chi, "status": status, "vectors": dict(b=b, diag=diag, x=x, r=r, z=z, p=p, q=q)}


def status_dict(words):
    w = np.asarray(words, dtype=np.uint64)
    f = w[3:7].view(np.float64)
    return {"iterations": int(w[0]), "flags": int(w[1]), "B": int(w[2]), "rr": float(f[0]), "bb": float(f[1]), "iso": float(f[2]),
            "w1": float(f[3])}


# ---- 5. density ------------------------------------------------------------------------------------------------------
def density(blocks, field, sweeps=2):
    nbr = neighbour_slots(blocks)
    D = np.asarray(field, dtype=np.float32).reshape(-1, 4)[:, 3].copy()
    for _ in range(sweeps):
        s = D.astype(np.float64)
        deg = np.zeros(len(D))
        d64 = D.astype(np.float64)
        for d in range(6):
            has = nbr[d] >= 0
            s = np.where(has, s + d64[np.maximum(nbr[d], 0)], s)
            deg += has
        D = (s / (1.0 + deg)).astype(np.float32)
    return D.reshape(-1, 512)


def operator_matrix(blocks, field, alpha):
    """The dense float64 matrix L + alpha diag(W) (deg and W exact, not the float32 diag) and b in float64"""
    nbr = neighbour_slots(blocks)
    F = np.asarray(field, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    n = len(F)
    A = np.zeros((n, n))
    b = np.zeros(n)
    for d in range(6):
        has = np.flatnonzero(nbr[d] >= 0)
        A[has, has] += 1.0
        A[has, nbr[d][has]] -= 1.0
        g = 0.5 * (F[nbr[d][has], d >> 1] + F[has, d >> 1])
        b[has] += -g if d & 1 else g
    A[np.arange(n), np.arange(n)] += alpha * F[:, 3]
    return A, b


# ---- the header on the host ------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <stdlib.h>
#include "sls_poisson_math.h"

int ref_splat(int M, const float *xyz, const float *normals, int B, const int32_t *blocks, double h, const double *origin,
              float *field, uint32_t *status)
{
    uint32_t *keys = malloc(4 * (size_t)M + 4), *order = malloc(4 * (size_t)M + 4), *first = malloc(4 * ((size_t)B * 512 + 1));
    if (!keys || !order || !first) return 1;
    sls_poisson_splat_host(M, xyz, normals, B, blocks, h, origin, field, status, keys, order, first);
    free(keys); free(order); free(first);
    return 0;
}

/* vec: 7 * 512 B floats (b, diag, x, r, z, p, q) */
int ref_solve(int B, const int32_t *blocks, const float *field, double alpha, int iterations, double tol, float *chi,
              uint64_t *status, float *vec)
{
    int32_t *nb6 = malloc(24 * (size_t)B + 4);
    if (!nb6) return 1;
    sls_poisson_solve_host(B, blocks, field, alpha, iterations, tol, chi, status, nb6, vec);
    free(nb6);
    return 0;
}

int ref_density(int B, const int32_t *blocks, const float *field, int sweeps, float *density)
{
    int32_t *nb6 = malloc(24 * (size_t)B + 4);
    float *tmp = malloc(2048 * (size_t)B + 4);
    if (!nb6 || !tmp) return 1;
    sls_poisson_density_host(B, blocks, field, sweeps, density, nb6, tmp);
    free(nb6); free(tmp);
    return 0;
}

double ref_dot(int B, const float *a, const float *b) { return sls_poisson_dot_host(B, a, 1, b, 1); }
void ref_neighbours(int B, const int32_t *blocks, int32_t *nb6) { sls_poisson_neighbours_host(B, blocks, nb6); }
int ref_consts(int *out)
{
    out[0] = SLS_POISSON_FLAG_CONVERGED; out[1] = SLS_POISSON_FLAG_NOT_PD; out[2] = SLS_POISSON_FLAG_EMPTY;
    out[3] = SLS_POISSON_STATUS_WORDS; out[4] = SLS_POISSON_REDUCE;
    return 5;
}
'''


class Host:
    """include/sls_poisson_math.h compiled as plain C and called through ctypes."""

    def __init__(self, lib):
        self.lib = lib
        V = C.c_void_p
        lib.ref_splat.argtypes = [C.c_int, V, V, C.c_int, V, C.c_double, V, V, V]
        lib.ref_solve.argtypes = [C.c_int, V, V, C.c_double, C.c_int, C.c_double, V, V, V]
        lib.ref_density.argtypes = [C.c_int, V, V, C.c_int, V]
        lib.ref_dot.restype = C.c_double
        lib.ref_dot.argtypes = [C.c_int, V, V]
        lib.ref_neighbours.argtypes = [C.c_int, V, V]
        lib.ref_consts.argtypes = [V]

    def consts(self):
        out = np.zeros(8, np.int32)
        n = self.lib.ref_consts(out.ctypes.data)
        return out[:n].tolist()

    def splat(self, points, normals, blocks, h, origin=(0.0, 0.0, 0.0)):
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        field = np.zeros((len(blocks), 512, 4), np.float32)
        status = np.zeros(4, np.uint32)
        assert self.lib.ref_splat(len(p), p.ctypes.data, n.ctypes.data, len(blocks), blocks.ctypes.data, float(h), o.ctypes.data,
                                  field.ctypes.data, status.ctypes.data) == 0
        return field, status

    def solve(self, blocks, field, alpha=4.0, iterations=300, tol=1e-4):
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 3)
        B = len(blocks)
        field = np.ascontiguousarray(field, dtype=np.float32)
        chi = np.zeros((B, 512), np.float32)
        status = np.zeros(STATUS_WORDS, np.uint64)
        vec = np.zeros((7, B, 512), np.float32)
        assert self.lib.ref_solve(B, blocks.ctypes.data, field.ctypes.data, float(alpha), int(iterations), float(tol), chi.ctypes.data,
                                  status.ctypes.data, vec.ctypes.data) == 0
        return {"chi": chi, "status": status, "vectors": dict(zip(("b", "diag", "x", "r", "z", "p", "q"), vec))}

    def density(self, blocks, field, sweeps=2):
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 3)
        field = np.ascontiguousarray(field, dtype=np.float32)
        out = np.zeros((len(blocks), 512), np.float32)
        assert self.lib.ref_density(len(blocks), blocks.ctypes.data, field.ctypes.data, int(sweeps), out.ctypes.data) == 0
        return out

    def dot(self, a, b):
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        return float(self.lib.ref_dot(a.size // 512, a.ctypes.data, b.ctypes.data))

    def neighbours(self, blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 3)
        nb = np.zeros((len(blocks), 6), np.int32)
        self.lib.ref_neighbours(len(blocks), blocks.ctypes.data, nb.ctypes.data)
        return nb


_KEEP = []


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="poisson_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "poisson_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libpoisson_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           src, "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- shared test inputs ----------------------------------------------------------------------------------------------
VS = 0.1
MARGIN = 3 * VS
CENTRE = np.array([0.137, -0.219, 0.071])                   # off the lattice
ORIGIN = (0.05, -0.02, 0.11)
CAP = 0.43                                                   # chord radius of the cap cut out of the unit sphere, around +z


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    same = a.view(np.uint8) == b.view(np.uint8)
    assert same.all(), f"{what}: {int((~same).sum())} bytes differ"


def blocks_around(points, h=VS, margin=MARGIN, origin=ORIGIN):
    """what tsdf.allocate_blocks(points, h, trunc=margin) returns (the NumPy rule of tsdf_ref)"""
    return tsdf_ref.blocks_of_points(points, h, margin, origin)[0]


@functools.lru_cache(maxsize=None)
def capped_sphere(n=19000):
    """(points, normals) float32: a Fibonacci lattice on the unit sphere around CENTRE without the cap around +z"""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    nrm = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    keep = ~((nrm[:, 2] > 0) & (np.hypot(nrm[:, 0], nrm[:, 1]) < CAP))
    pts, nrm = (nrm[keep] + CENTRE).astype(np.float32), nrm[keep].astype(np.float32)
    pts.setflags(write=False); nrm.setflags(write=False)
    return pts, nrm


@functools.lru_cache(maxsize=None)
def holed_plane(n=20000, size=6.0, noise=0.02, hole=0.3, seed=3):
    """(points, normals) float32: the plane z = 0.033 over [-size/2, size/2]^2 with noise along z and a round hole at (0.4, -0.3)"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-size / 2, size / 2, (n, 2))
    keep = np.hypot(xy[:, 0] - 0.4, xy[:, 1] + 0.3) >= hole
    pts = np.concatenate([xy, 0.033 + noise * rng.normal(size=(n, 1))], 1)[keep].astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(pts), 1))
    pts.setflags(write=False); nrm.setflags(write=False)
    return pts, nrm


def sphere_report(tris, centre=CENTRE):
    """dict(closed, euler, outward, mean_error over the vertices whose direction has samples, cap_error over the others)"""
    rep = tsdf_ref.manifold_report(tris)
    t64 = np.asarray(tris, dtype=np.float64)
    n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    v = np.unique(t64.reshape(-1, 3), axis=0) - centre
    r = np.linalg.norm(v, axis=1)
    u = v / r[:, None]
    cap = (u[:, 2] > 0) & (np.hypot(u[:, 0], u[:, 1]) < CAP)
    return {"closed": rep["bad_edges"] == 0 and rep["degenerate"] == 0, "euler": rep["V"] - rep["E"] + rep["F"],
            "outward": bool((np.einsum("ij,ij->i", n, t64.mean(1) - centre) > 0).all()),
            "mean_error": float(np.abs(r[~cap] - 1.0).mean()), "cap_error": float(np.abs(r[cap] - 1.0).max()) if cap.any() else 0.0,
            "cap_vertices": int(cap.sum()), "triangles": len(t64)}
