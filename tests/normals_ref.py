"""NumPy restatement of the PCA normal estimate (include/sls_normals_math.h, sls_cloud_normals,
splat_loam_amd/evaluation.py: estimate_normals): brute-force neighbour lists as outlier_ref.py builds them, the prefix
within the radius, the float64 mean and covariance in list order, the header's cyclic Jacobi, the choice of the smallest
eigenvalue's column, the orientation and the fallback.

The eigen-solve is written twice.  `jacobi_scalar` is the header line by line with Python floats and math.sqrt: IEEE
float64 with one rounding per operation, no fused multiply-add, so it gives the bits of the header compiled with
-ffp-contract=off.  `normals` runs the same operations in the same order on NumPy float64 arrays, a point per element (a
skipped rotation is an element left as it was); tests/test_normals_math.py holds the two equal bit for bit.

Open3D is not installed where this project is developed: the rule is Open3D's estimate_normals + orientation as RESTATED in
the header, and the device code is pinned against this file, not against Open3D.
"""
from __future__ import annotations

import math

import numpy as np

import outlier_ref

SWEEPS = 6          # SLS_NORMALS_SWEEPS
NN_MAX = 64         # SLS_NORMALS_NN_MAX


def lists(points, k):
    """(d2 float32 (M,k), index int32 (M,k)) of the cloud's self-query: +inf and -1 beyond M."""
    return outlier_ref.split(outlier_ref.keys_k(points, points, k))


def counts(d2, index, radius):
    """n_i: the length of the list's prefix that is real and has d2 <= radius * radius (one float32 product)."""
    r = np.float32(np.inf if radius is None else radius)
    with np.errstate(over="ignore"):
        r2 = np.float32(r * r)
    ok = (index >= 0) & (d2 <= r2)
    return np.where(ok.all(1), ok.shape[1], np.argmin(ok, axis=1)).astype(np.int32)


def _rotate_scalar(app, aqq, apq, arp, arq, vp, vq):
    """sls_normals_rotate: returns the new (app, aqq, apq, arp, arq, vp, vq); vp, vq: the three rows' entries."""
    if apq == 0.0:
        return app, aqq, apq, arp, arq, vp, vq
    theta = 0.5 * (aqq - app) / apq
    abs_theta = -theta if theta < 0.0 else theta
    den = abs_theta + math.sqrt(theta * theta + 1.0)
    t = -1.0 / den if theta < 0.0 else 1.0 / den
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    tau = s / (1.0 + c)
    h = t * apq
    rot = lambda g, f: (g - s * (f + g * tau), f + s * (g - f * tau))
    arp, arq = rot(arp, arq)
    new = [rot(g, f) for g, f in zip(vp, vq)]
    return app - h, aqq + h, 0.0, arp, arq, [n[0] for n in new], [n[1] for n in new]


def jacobi_scalar(cov):
    """sls_normals_jacobi on six Python floats (xx, xy, xz, yy, yz, zz): (d [3], v [3][3] row-major, columns = vectors)."""
    a00, a01, a02, a11, a12, a22 = (float(c) for c in cov)
    col = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]          # col[j]: column j of V
    for _ in range(SWEEPS):
        a00, a11, a01, a02, a12, col[0], col[1] = _rotate_scalar(a00, a11, a01, a02, a12, col[0], col[1])
        a00, a22, a02, a01, a12, col[0], col[2] = _rotate_scalar(a00, a22, a02, a01, a12, col[0], col[2])
        a11, a22, a12, a01, a02, col[1], col[2] = _rotate_scalar(a11, a22, a12, a01, a02, col[1], col[2])
    return [a00, a11, a22], [[col[j][r] for j in range(3)] for r in range(3)]


def _rotate(a, pp, qq, pq, rp, rq, cp, cq, V):
    """The same on arrays: a maps an element's name to an (M,) float64 array, V[row][column] likewise; cp, cq: V's columns."""
    apq = a[pq]
    go = apq != 0.0
    safe = np.where(go, apq, 1.0)
    with np.errstate(over="ignore"):                                    # (an infinite theta gives t = 0, as in the header)
        theta = 0.5 * (a[qq] - a[pp]) / safe
        neg = theta < 0.0
        abs_theta = np.where(neg, -theta, theta)
        den = abs_theta + np.sqrt(theta * theta + 1.0)
    t = np.where(neg, -1.0 / den, 1.0 / den)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    tau = s / (1.0 + c)
    h = t * safe

    def rot(g, f):
        return np.where(go, g - s * (f + g * tau), g), np.where(go, f + s * (g - f * tau), f)
    a[pp], a[qq] = np.where(go, a[pp] - h, a[pp]), np.where(go, a[qq] + h, a[qq])
    a[pq] = np.where(go, 0.0, apq)
    a[rp], a[rq] = rot(a[rp], a[rq])
    for row in range(3):
        V[row][cp], V[row][cq] = rot(V[row][cp], V[row][cq])


def jacobi(cov, sweeps=SWEEPS):
    """cov (M,6) float64 -> d (M,3), V (M,3,3): the header's solve, a matrix per row."""
    cov = np.asarray(cov, np.float64)
    M = len(cov)
    a = {"00": cov[:, 0].copy(), "01": cov[:, 1].copy(), "02": cov[:, 2].copy(), "11": cov[:, 3].copy(), "12": cov[:, 4].copy(),
         "22": cov[:, 5].copy()}
    V = [[np.full(M, 1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    for _ in range(sweeps):
        _rotate(a, "00", "11", "01", "02", "12", 0, 1, V)
        _rotate(a, "00", "22", "02", "01", "12", 0, 2, V)
        _rotate(a, "11", "22", "12", "01", "02", 1, 2, V)
    d = np.stack([a["00"], a["11"], a["22"]], 1)
    return d, np.stack([np.stack(V[r], 1) for r in range(3)], 1)


def covariance(points, index, n):
    """(M,6) float64: the header's mean and six sums, in list order, over the first n_i entries of every row."""
    P = np.asarray(points, np.float32).astype(np.float64)
    M, k = index.shape
    safe = np.where(index >= 0, index, 0)
    dn = np.maximum(n, 1).astype(np.float64)
    s = np.zeros((M, 3))
    for j in range(k):
        use = (j < n)[:, None]
        s = np.where(use, s + P[safe[:, j]], s)
    mean = s / dn[:, None]
    acc = np.zeros((M, 6))
    for j in range(k):
        use = (j < n)[:, None]
        d = P[safe[:, j]] - mean
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                         d[:, 2] * d[:, 2]], 1)
        acc = np.where(use, acc + prod, acc)
    return acc / dn[:, None]


def fallback(points, viewpoint):
    """unit(viewpoint - p) in float64, rounded; (0, 0, 1) for the zero vector."""
    v = np.asarray(viewpoint, np.float32).astype(np.float64)[None, :] - np.asarray(points, np.float32).astype(np.float64)
    len2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    zero = len2 == 0.0
    out = v / np.sqrt(np.where(zero, 1.0, len2))[:, None]
    out[zero] = (0.0, 0.0, 1.0)
    return out.astype(np.float32)


def select(d, V, points, viewpoint):
    """(normal float32 (M,3), eigenvalues float32 (M,3)) from the solve: sls_normals_select."""
    dm, n = d[:, 0].copy(), V[:, :, 0].copy()
    for j in (1, 2):
        less = d[:, j] < dm
        dm = np.where(less, d[:, j], dm)
        n = np.where(less[:, None], V[:, :, j], n)
    length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    n = n / length[:, None]
    v = np.asarray(viewpoint, np.float32).astype(np.float64)[None, :] - np.asarray(points, np.float32).astype(np.float64)
    flip = n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1] + n[:, 2] * v[:, 2] < 0.0
    n = np.where(flip[:, None], -n, n)
    e = [d[:, 0], d[:, 1], d[:, 2]]
    for lo, hi in ((0, 1), (1, 2), (0, 1)):                             # the header's three exchanges
        swap = e[hi] < e[lo]
        e[lo], e[hi] = np.where(swap, e[hi], e[lo]), np.where(swap, e[lo], e[hi])
    return n.astype(np.float32), np.stack(e, 1).astype(np.float32)


def normals_from_lists(points, d2, index, radius, viewpoint=(0.0, 0.0, 0.0)):
    """dict(normals (M,3) float32, count (M,) int32, eigenvalues (M,3) float32, cov (M,6) float64) from list rows."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = counts(d2, index, radius)
    cov = covariance(points, index, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        d, V = jacobi(cov)
        nrm, eig = select(d, V, points, viewpoint)
    few = n < 3
    nrm[few] = fallback(points[few], viewpoint)
    eig[few] = 0.0
    return {"normals": nrm, "count": n, "eigenvalues": eig, "cov": cov}


def normals(points, k, radius, viewpoint=(0.0, 0.0, 0.0), full=None):
    """The whole rule.  full: (d2, index) of a longer self-query list, whose first k columns are the k-list."""
    d2, index = lists(points, k) if full is None else (full[0][:, :k], full[1][:, :k])
    return normals_from_lists(points, d2, index, radius, viewpoint)


def normal_scalar(points, d2_row, index_row, i, radius, viewpoint):
    """One point by the header's own loops, Python floats only: (normal [3] float32, n, eigenvalues [3] float32)."""
    P = np.asarray(points, np.float32)
    r = np.float32(np.inf if radius is None else radius)
    with np.errstate(over="ignore"):
        r2 = np.float32(r * r)
    n = 0
    for j in range(len(index_row)):
        if index_row[j] < 0 or not d2_row[j] <= r2:
            break
        n += 1
    view = [float(np.float32(c)) for c in viewpoint]
    p = [float(c) for c in P[i]]
    v = [view[a] - p[a] for a in range(3)]
    if n < 3:
        len2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        if len2 == 0.0:
            return np.array([0, 0, 1], np.float32), n, np.zeros(3, np.float32)
        length = math.sqrt(len2)
        return np.array([c / length for c in v], np.float64).astype(np.float32), n, np.zeros(3, np.float32)
    s = [0.0, 0.0, 0.0]
    for j in range(n):
        q = P[index_row[j]]
        s = [s[a] + float(q[a]) for a in range(3)]
    mean = [c / float(n) for c in s]
    acc = [0.0] * 6
    for j in range(n):
        q = P[index_row[j]]
        dx, dy, dz = (float(q[a]) - mean[a] for a in range(3))
        for t, prod in enumerate((dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)):
            acc[t] += prod
    d, V = jacobi_scalar([c / float(n) for c in acc])
    m = 0
    for j in (1, 2):
        if d[j] < d[m]:
            m = j
    nx, ny, nz = V[0][m], V[1][m], V[2][m]
    length = math.sqrt(nx * nx + ny * ny + nz * nz)
    nx, ny, nz = nx / length, ny / length, nz / length
    if nx * v[0] + ny * v[1] + nz * v[2] < 0.0:
        nx, ny, nz = -nx, -ny, -nz
    return np.array([nx, ny, nz], np.float64).astype(np.float32), n, np.array(sorted(d), np.float64).astype(np.float32)
