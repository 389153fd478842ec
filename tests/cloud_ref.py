"""NumPy restatement of the voxel down-sampling and of the mesh sampling (splat_loam_amd/evaluation.py,
sls_voxel_downsample / sls_mesh_sample), float64, in the operation sequence of include/sls_cloud_math.h.

Open3D is not installed where this project is built and tested: both operations are restated from its documented
behaviour (voxel_down_sample: voxel index floor((p - (min - size / 2)) / size), the mean of a voxel's points;
sample_points_uniformly: a face in proportion to its area, the point (1 - sqrt(u1)) v0 + sqrt(u1) (1 - u2) v1 +
sqrt(u1) u2 v2), and what Open3D leaves open — the order of the rows, the random stream — is what the header defines.

On inputs whose coordinates are multiples of 1/16 with magnitude <= 64 every float64 sum of a voxel is exact in any
order, so rows, counts and centroids here ARE the kernel's bits.
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
INDEX_LIMIT = 1 << 21


def voxel_keys(points, voxel_size):
    """uint64 key ix | iy << 21 | iz << 42 of every point; ValueError as evaluation.voxel_down_sample raises it."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if not np.isfinite(p).all():
        raise ValueError("non-finite coordinate")
    vs = np.float64(voxel_size)
    origin = p.min(0).astype(np.float64) - np.float64(0.5) * vs
    idx = np.floor((p.astype(np.float64) - origin) / vs)
    if not ((idx >= 0) & (idx < INDEX_LIMIT)).all():
        raise ValueError("an index of 2^21 or more")
    i = idx.astype(np.uint64)
    return i[:, 0] | (i[:, 1] << np.uint64(21)) | (i[:, 2] << np.uint64(42))


def voxel_down_sample(points, voxel_size):
    """(rows (n_voxels,3) float32, counts (n_voxels,) int32), rows in ascending key order; the float64 sum of a voxel
    adds its points in ascending input index (np.add.at works through its indices in order)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0,), np.int32)
    keys = voxel_keys(p, voxel_size)
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    sums = np.zeros((len(counts), 3), np.float64)
    np.add.at(sums, inverse.reshape(-1), p.astype(np.float64))
    return (sums / counts[:, None].astype(np.float64)).astype(np.float32), counts.astype(np.int32)


def face_areas(vertices, faces):
    """float64 area of every face in the header's operation order; a face with an index outside the vertices gets NaN."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    bad = ((f < 0) | (f >= len(v))).any(1)
    g = np.where(bad[:, None], 0, f) if len(v) else np.zeros_like(f)
    if len(v) == 0:
        return np.full(len(f), np.nan), bad
    v0, v1, v2 = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    area[bad] = np.nan
    return area, bad


def mesh_weights(vertices, faces, crop_box=None):
    """(w uint64 (F,), number of faces with a bad index): w = floor(A / A_max 2^32), 0 for a dropped face."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    area, bad = face_areas(v32, f)
    area = np.where(np.isfinite(area), area, 0.0)
    if crop_box is not None and len(f):
        box = np.asarray(crop_box, np.float32).reshape(6)
        with np.errstate(invalid="ignore"):
            inside = ((v32 >= box[:3]) & (v32 <= box[3:])).all(1)
        g = np.where(bad[:, None], 0, f)
        keep = inside[g].all(1) if len(v32) else np.zeros(len(f), bool)
        area = np.where(keep & ~bad, area, 0.0)
    amax = area.max() if len(area) else 0.0
    if not amax > 0:
        return np.zeros(len(f), np.uint64), int(bad.sum())
    return np.floor(area / amax * 4294967296.0).astype(np.uint64), int(bad.sum())


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (uint64 arithmetic on 32-bit values)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def mulhi64(a, b):
    """High 64 bits of a * b for uint64 arrays, in 32-bit pieces (no overflow anywhere)."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    s32 = np.uint64(32)
    a0, a1, b0, b1 = a & M32, a >> s32, b & M32, b >> s32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s32) + (p01 & M32) + (p10 & M32)
    return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)


def sample_mesh(vertices, faces, n, seed=0, crop_box=None, float32=False):
    """(points (n,3) float64, face (n,) int32) of the seeded draw; ValueError for a bad index or a mesh without area.
    float32=True: the point in the header's own float32 arithmetic (NumPy's float32 + - * and sqrt are the IEEE
    operations the kernel is compiled to, without contraction): the kernel's bits."""
    ft = np.float32 if float32 else np.float64
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(ft)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    w, n_bad = mesh_weights(vertices, f, crop_box)
    if n_bad:
        raise ValueError("vertex index outside the vertices")
    C = np.cumsum(w, dtype=np.uint64)
    if len(C) == 0 or C[-1] == 0:
        raise ValueError("no area")
    i = np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r0, r1, r2, r3 = philox4x32_10(i, zero + np.uint64(2), zero, zero, seed & 0xFFFFFFFF, seed >> 32)
    t = mulhi64(r0 | (r1 << np.uint64(32)), C[-1])
    face = np.searchsorted(C, t, side="right")             # the first f with C[f] > t
    u1 = (2 * (r2 >> np.uint64(9)) + 1).astype(ft) * ft(2.0 ** -24)      # (an odd 24-bit integer: exact in float32)
    u2 = (2 * (r3 >> np.uint64(9)) + 1).astype(ft) * ft(2.0 ** -24)
    s = np.sqrt(u1)
    a, b, c = ft(1.0) - s, s * (ft(1.0) - u2), s * u2
    g = f[face]
    points = (a[:, None] * v[g[:, 0]] + b[:, None] * v[g[:, 1]]) + c[:, None] * v[g[:, 2]]
    assert points.dtype == ft
    return points, face.astype(np.int32)


def evaluate_recon(reference, vertices, faces, nn_ref, down_sample_res=0.02, threshold=0.2, truncation_acc=0.5,
                   truncation_com=0.5, crop_to_reference=False, mesh_sample_point=10_000_000, seed=0):
    """The all-NumPy chain with the reference's keys; `nn_ref` is tests/nn_ref.py.  The sample points are taken in the
    header's float32 arithmetic (a last bit can move a point into the next voxel)."""
    reference = np.asarray(reference, np.float32)
    box = None
    if crop_to_reference:
        pad = np.array([0, 0, down_sample_res], np.float32)
        box = np.concatenate([reference.min(0) - pad, reference.max(0) + pad])
    estimate = sample_mesh(vertices, faces, mesh_sample_point, seed, box, float32=True)[0]
    if down_sample_res > 0:
        estimate = voxel_down_sample(estimate, down_sample_res)[0]
        reference = voxel_down_sample(reference, down_sample_res)[0]
    m = nn_ref.cloud_metrics(reference, estimate, threshold, truncation_acc, truncation_com)
    return {
        "MAE_accuracy (cm)": m["accuracy_m"] * 100, "MAE_completeness (cm)": m["completeness_m"] * 100,
        "Chamfer_L1 (cm)": m["chamfer_l1_m"] * 100, "Precision [Accuracy] (%)": m["precision"] * 100.0,
        "Recall [Completeness] (%)": m["recall"] * 100.0, "F-score (%)": m["fscore"] * 100.0,
        "Inlier_threshold (m)": float(threshold), "Outlier_truncation_acc (m)": float(truncation_acc),
        "Outlier_truncation_com (m)": float(truncation_com),
    }


# ---- inputs the host and the device tests share ----------------------------------------------------------------------
def grid_mesh(nx=8, ny=8):
    """An nx x ny grid of unit quads in the plane z = 0 (two triangles each), a few faces collapsed to zero area and a
    few repeated: (vertices (V,3) float32 on the lattice, faces (F,3) int32, the zero-area faces)."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    vertices = np.stack([xs.ravel() - nx / 2, ys.ravel() - ny / 2, np.zeros(xs.size)], 1).astype(np.float32)
    vertices[:, 2] = ((xs.ravel() * 3 + ys.ravel() * 5) % 4) / 16.0            # a little relief: the faces differ in area
    vid = lambda i, j: i * (ny + 1) + j
    faces = []
    for i in range(nx):
        for j in range(ny):
            faces.append([vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)])
            faces.append([vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)])
    faces = np.array(faces, np.int32)
    zero = np.array([5, 40, 77, 127])
    faces[zero, 2] = faces[zero, 1]                                            # two equal vertices: no area
    faces[[9, 10, 11]] = faces[[60, 60, 3]]                                    # duplicated faces
    return vertices, faces, zero


ONE_TO_THREE = (np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, -3, 0]], np.float32), np.array([[0, 1, 2], [0, 3, 1]], np.int32))
PROPORTION_N, PROPORTION_SEED = 200_000, 7
