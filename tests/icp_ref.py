"""include/sls_icp_math.h restated in NumPy: float64, the header's order of operations, a brute-force association.

Everything per point is an array expression written in the header's order (NumPy never contracts a * b + c into an fma),
the sum over the cloud follows the header's four steps, and the solve runs on Python floats with math.sqrt — IEEE doubles,
one operation at a time.  So the results equal the header compiled for the host, and the device, bit for bit, wherever
the association is the same: where the float32 search of the device and a float64 search cannot disagree (`icp` records
the margins that decide this)."""
import math

import numpy as np

PLANE, POINT = 0, 1
TERMS, BLOCK = 29, 256
FLAG_CONVERGED, FLAG_FEW, FLAG_NOT_PD = 1, 2, 4
STATUS_WORDS = 20
DEFAULTS = dict(damping=1e-9, eps_rot=1e-7, eps_trans=1e-7, min_inliers=6)
IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


def gate2(max_distance):
    d = np.float32(max_distance)
    return np.float32(d * d)


def transform(T, p):
    """p' (M,3) float32 of the source rows p (M,3) float32 under the pose T (12,) float64."""
    T = np.asarray(T, np.float64)
    x, y, z = (np.asarray(p, np.float32)[:, k].astype(np.float64) for k in range(3))
    out = np.empty((len(x), 3), np.float32)
    for a in range(3):
        out[:, a] = (((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3]).astype(np.float32)
    return out


def _fma32(a, b):
    """fmaf(a, a, b) for float32 arrays, exactly: the float64 sum a*a + b rounded to odd, then to float32 (a*a is exact in
    float64; rounding a 53-bit round-to-odd value to 24 bits equals one rounding of the exact sum)."""
    sq = a.astype(np.float64) * a.astype(np.float64)
    b = b.astype(np.float64)
    s = sq + b
    bb = s - sq
    err = (sq - (s - bb)) + (b - bb)                    # TwoSum: sq + b == s + err exactly
    bits = s.view(np.int64).copy()                      # (all values >= +0: the bit pattern grows with the value)
    bits -= (err < 0).astype(np.int64)                  # towards zero
    bits |= (err != 0).astype(np.int64)                 # sticky
    return bits.view(np.float64).astype(np.float32)


def dist2_f32(q, t):
    """sls_nn_dist2 of every query row against every target row: (Mq, Mt) float32."""
    d = t[None, :, :] - q[:, None, :]
    return _fma32(d[..., 2], _fma32(d[..., 1], d[..., 0] * d[..., 0]))


def associate(moved, target, g2, chunk=1024, margins=False):
    """The rule of sls_nn_query by brute force: (index (M,) int32, dist2 (M,) float32, inlier (M,) bool); np.argmin returns
    the lowest index among equals.  margins=True adds, from float64 distances of the same float32 coordinates, the relative
    gap between the best and the second-best target ((d_second - d_best) / d_second; 1 where there is one target, 0 where
    two targets are at distance 0) and the relative gap between the best d2 and the gate."""
    M = len(moved)
    index = np.empty(M, np.int32)
    d2 = np.empty(M, np.float32)
    gap_nn = np.ones(M)
    gap_gate = np.ones(M)
    for a in range(0, M, chunk):
        d = dist2_f32(moved[a:a + chunk], target)
        idx = d.argmin(1)
        index[a:a + chunk] = idx
        d2[a:a + chunk] = d[np.arange(len(idx)), idx]
        if margins:
            diff = target[None, :, :].astype(np.float64) - moved[a:a + chunk, None, :].astype(np.float64)
            e = (diff * diff).sum(2)
            best = e.min(1)
            if target.shape[0] > 1:
                second = np.partition(e, 1, axis=1)[:, 1]
                gap_nn[a:a + chunk] = np.where(second > 0, (second - best) / np.where(second > 0, second, 1.0), 0.0)
            gap_gate[a:a + chunk] = np.abs(best - float(g2)) / float(g2)
    out = (index, d2, d2 <= g2)
    return out + ((gap_nn, gap_gate),) if margins else out


def _row(acc, J, r):
    k = 0
    for a in range(6):
        for c in range(a, 6):
            acc[:, k] += J[a] * J[c]
            k += 1
    for a in range(6):
        acc[:, 21 + a] += J[a] * r
    acc[:, 27] += r * r


def terms(method, inlier, moved, q, n):
    """sls_icp_terms for every point: (M, 29) float64.  q, n: the associated target rows (n ignored for POINT)."""
    M = len(moved)
    acc = np.zeros((M, TERMS))
    px, py, pz = (moved[:, k].astype(np.float64) for k in range(3))
    dx, dy, dz = px - q[:, 0].astype(np.float64), py - q[:, 1].astype(np.float64), pz - q[:, 2].astype(np.float64)
    one, zero = np.ones(M), np.zeros(M)
    if method == PLANE:
        nx, ny, nz = (n[:, k].astype(np.float64) for k in range(3))
        r = (nx * dx + ny * dy) + nz * dz
        _row(acc, (nx, ny, nz, py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx), r)
    else:
        _row(acc, (one, zero, zero, zero, pz, -py), dx)
        _row(acc, (zero, one, zero, -pz, zero, px), dy)
        _row(acc, (zero, zero, one, py, -px, zero), dz)
    acc[:, 28] += 1.0
    acc[~np.asarray(inlier, bool)] = 0.0
    return acc


def _block_sums(rows):
    """steps 2 and 3 of the header's sum: rows (B * 256, 29) -> (B, 29)"""
    x = rows.reshape(-1, 4, 64, TERMS)
    for off in (32, 16, 8, 4, 2, 1):
        x = x[:, :, :off] + x[:, :, off:2 * off]
    w = x[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def reduce_terms(rows):
    """The header's sum of the (M, 29) terms: (29,) float64."""
    M = len(rows)
    nblocks = (M + BLOCK - 1) // BLOCK
    padded = np.zeros((nblocks * BLOCK, TERMS))
    padded[:M] = rows
    partials = _block_sums(padded)
    rounds = (nblocks + BLOCK - 1) // BLOCK
    grid = np.zeros((rounds * BLOCK, TERMS))
    grid[:nblocks] = partials
    acc = np.zeros((BLOCK, TERMS))
    for r in range(rounds):                             # thread t: rows t, t + 256, ... in this order, from zeros
        acc = acc + grid[r * BLOCK:(r + 1) * BLOCK]
    return _block_sums(acc)[0]


def solve(S, T, damping, eps_rot, eps_trans, min_inliers):
    """sls_icp_solve on Python floats: (flags, new T (12,) float64, xi (6,))."""
    S = [float(v) for v in S]
    T = [float(v) for v in T]
    H = [[0.0] * 6 for _ in range(6)]
    t = 0
    for a in range(6):
        for c in range(a, 6):
            H[a][c] = H[c][a] = S[t]
            t += 1
    zero6 = [0.0] * 6
    if S[28] < float(min_inliers):
        return FLAG_FEW, np.array(T), np.array(zero6)
    for a in range(6):
        H[a][a] = H[a][a] + damping
    L = [[0.0] * 6 for _ in range(6)]
    for a in range(6):
        for c in range(a + 1):
            s = H[a][c]
            for k in range(c):
                s = s - L[a][k] * L[c][k]
            if a == c:
                if not s > 0.0:
                    return FLAG_NOT_PD, np.array(T), np.array(zero6)
                L[a][a] = math.sqrt(s)
            else:
                L[a][c] = s / L[c][c]
    yv, xi = [0.0] * 6, [0.0] * 6
    for a in range(6):
        s = -S[21 + a]
        for k in range(a):
            s = s - L[a][k] * yv[k]
        yv[a] = s / L[a][a]
    for a in range(5, -1, -1):
        s = yv[a]
        for k in range(a + 1, 6):
            s = s - L[k][a] * xi[k]
        xi[a] = s / L[a][a]
    if not all(math.isfinite(v) for v in xi):
        return FLAG_NOT_PD, np.array(T), np.array(zero6)
    ax, ay, az = 0.5 * xi[3], 0.5 * xi[4], 0.5 * xi[5]
    s = (ax * ax + ay * ay) + az * az
    den, c = 1.0 + s, 1.0 - s
    dR = [(c + 2.0 * (ax * ax)) / den, 2.0 * (ax * ay - az) / den, 2.0 * (ax * az + ay) / den,
          2.0 * (ax * ay + az) / den, (c + 2.0 * (ay * ay)) / den, 2.0 * (ay * az - ax) / den,
          2.0 * (ax * az - ay) / den, 2.0 * (ay * az + ax) / den, (c + 2.0 * (az * az)) / den]
    N = [0.0] * 12
    for a in range(3):
        for j in range(3):
            N[4 * a + j] = (dR[3 * a] * T[j] + dR[3 * a + 1] * T[4 + j]) + dR[3 * a + 2] * T[8 + j]
        N[4 * a + 3] = ((dR[3 * a] * T[3] + dR[3 * a + 1] * T[7]) + dR[3 * a + 2] * T[11]) + xi[a]
    nw = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
    nv = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
    return (FLAG_CONVERGED if (nw < eps_rot and nv < eps_trans) else 0), np.array(N), np.array(xi)


def linearize(source, target, normals, T, method, max_distance, margins=False):
    """One pass at the pose T: dict(system (29,), index, dist2, inlier, moved[, gap_nn, gap_gate])."""
    moved = transform(T, source)
    res = associate(moved, target, gate2(max_distance), margins=margins)
    index, d2, inlier = res[:3]
    q = target[index]
    n = normals[index] if method == PLANE else None
    out = dict(system=reduce_terms(terms(method, inlier, moved, q, n)), index=index, dist2=d2, inlier=inlier, moved=moved)
    if margins:
        out["gap_nn"], out["gap_gate"] = res[3]
    return out


def icp(source, target, normals, init=None, method=PLANE, max_distance=1.0, iterations=30, margins=False, **params):
    """The loop of sls_cloud_icp.  Returns dict(pose (12,), updates, flags, inliers, sum_r2, system, index, dist2, passes):
    `passes` holds every pass's linearisation (with the margins where asked for) and the pose it was taken at."""
    p = dict(DEFAULTS, **params)
    source, target = np.ascontiguousarray(source, np.float32), np.ascontiguousarray(target, np.float32)
    T = np.array(IDENTITY if init is None else np.asarray(init, np.float64).reshape(-1)[:12], np.float64)
    updates, flags, done, passes = 0, 0, False, []
    if len(source) == 0:
        return dict(pose=T, updates=0, flags=FLAG_FEW, inliers=0, sum_r2=0.0, system=np.zeros(TERMS), index=np.zeros(0, np.int32),
                    dist2=np.zeros(0, np.float32), passes=[])
    for it in range(iterations + 1):
        lin = linearize(source, target, normals, T, method, max_distance, margins)
        lin["pose"] = T.copy()
        passes.append(lin)
        if done or it == iterations:
            break
        f, T2, _ = solve(lin["system"], T, p["damping"], p["eps_rot"], p["eps_trans"], p["min_inliers"])
        if f & (FLAG_FEW | FLAG_NOT_PD):
            flags |= f
            break                                       # the pose is kept: this pass evaluated it
        T = T2
        updates += 1
        if f & FLAG_CONVERGED:
            flags |= FLAG_CONVERGED
            done = True
    S = passes[-1]["system"]
    return dict(pose=T, updates=updates, flags=flags, inliers=int(S[28]), sum_r2=float(S[27]), system=S, index=passes[-1]["index"],
                dist2=passes[-1]["dist2"], passes=passes)


def status_words(res, Ms, Mt):
    """sls_cloud_icp's out_status for a result of `icp`: (20,) int64."""
    w = np.zeros(STATUS_WORDS, np.int64)
    w[0], w[1], w[2], w[3], w[4] = res["updates"], res["inliers"], Ms, Mt, res["flags"]
    w[5] = np.array([res["sum_r2"]], np.float64).view(np.int64)[0]
    w[6:18] = np.asarray(res["pose"], np.float64).view(np.int64)
    w[18] = 2
    return w


def pose_error(T, truth):
    """(rotation angle in radians, translation distance) between two poses (12,)"""
    A, B = np.asarray(T, np.float64).reshape(3, 4), np.asarray(truth, np.float64).reshape(3, 4)
    dR = A[:, :3] @ B[:, :3].T
    return float(np.linalg.norm(dR - dR.T) / (2 * math.sqrt(2))), float(np.linalg.norm(A[:, 3] - B[:, 3]))


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).reshape(-1)


def walls(n=9, spacing=0.25):
    """Three mutually orthogonal lattice walls (x = 0, y = 0, z = 0) of n x n points each, with their axis normals; every
    seventh row's normal is tilted (still a unit vector in float64, rounded to float32)."""
    g = np.arange(1, n + 1) * spacing
    a, b = (v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij"))
    z = np.zeros_like(a)
    pts = np.concatenate([np.stack([z, a, b], 1), np.stack([a, z, b], 1), np.stack([a, b, z], 1)]).astype(np.float32)
    nrm = np.concatenate([np.tile([1.0, 0, 0], (n * n, 1)), np.tile([0, 1.0, 0], (n * n, 1)), np.tile([0, 0, 1.0], (n * n, 1))])
    tilt = np.arange(len(pts)) % 7 == 3
    nrm[tilt] += 0.05 * np.roll(nrm[tilt], 1, axis=1) - 0.03 * np.roll(nrm[tilt], 2, axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, nrm.astype(np.float32)
