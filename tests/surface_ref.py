"""Reference side of the surface sampler ("Surface samples"; sls_surface_samples) — shared by
tests/test_surface_math.py (CPU) and tests/test_surface_samples.py (GPU).  Not a test module.

A NumPy restatement: the random words through densify_draw_ref.philox4x32_10, the validity mask from float32
comparisons, the rank floor(r n_valid / 2^32) in uint64, the rank-th valid pixel through np.flatnonzero — all integers,
compared without tolerance — and the point and the normal in float64, written from the formulas of
renderer.pixel_rays / renderer.postprocess and the transform the reference's pcd.transform applies, not from the kernel.
"""
import numpy as np

from densify_draw_ref import philox4x32_10


def sample_words(n_samples, seed, frame_id):
    """r_j, j = 0 .. n_samples - 1: first word of Philox4x32-10, counter (j, 1, frame_id, 0), key (seed lo, seed hi)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    j = np.arange(n_samples, dtype=np.uint64)
    zero = np.zeros_like(j)
    return philox4x32_10((j, zero + np.uint64(1), zero + np.uint64(int(frame_id) & 0xFFFFFFFF), zero),
                         (seed & 0xFFFFFFFF, seed >> 32))[0]


def sample_indices(words, n_valid):
    """(uint32)(((uint64) r * n_valid) >> 32)"""
    return ((np.asarray(words, dtype=np.uint32).astype(np.uint64) * np.uint64(n_valid)) >> np.uint64(32)).astype(np.uint32)


def valid_mask(allmap, min_opacity, max_depth_dist):
    """!(alpha < (float) min_opacity) && !(dist > (float) max_depth_dist), flat, row-major; float32 comparisons."""
    am = np.asarray(allmap, dtype=np.float32)
    alpha, dist = am[1].reshape(-1), am[6].reshape(-1)
    with np.errstate(invalid="ignore"):
        return ~(alpha < np.float32(min_opacity)) & ~(dist > np.float32(max_depth_dist))


def select_pixels(allmap, min_opacity, max_depth_dist, n_samples, seed, frame_id):
    """(n_valid, the selected row-major pixels (int64, n_samples) — empty where n_valid == 0)."""
    where = np.flatnonzero(valid_mask(allmap, min_opacity, max_depth_dist))
    if where.size == 0:
        return 0, np.zeros((0,), np.int64)
    idx = sample_indices(sample_words(n_samples, seed, frame_id), where.size)
    assert int(idx.max()) < where.size
    return int(where.size), where[idx.astype(np.int64)].astype(np.int64)


def points_normals(allmap, pixels, K, view32, world_T_model, depth_ratio):
    """float64 (points (n,3), normals (n,3)) of the given pixels.
    K: the 3x3 intrinsics (u = fx az + cx, v = fy el + cy); view32: the float32 world_view_transform^T the keyframe was
    rendered with (inv(model_T_frame) rounded, as scene.Camera stores it); world_T_model: 4x4."""
    am = np.asarray(allmap, dtype=np.float32).astype(np.float64)
    _, H, W = am.shape
    flat = am.reshape(7, -1)[:, pixels]
    r, c = np.divmod(np.asarray(pixels, dtype=np.int64), W)
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float32).astype(np.float64))
    gx, gy = c - 0.5, r - 0.5                                           # utils/graphic_utils.py:46-49
    az = Kinv[0, 0] * gx + Kinv[0, 1] * gy + Kinv[0, 2]
    el = Kinv[1, 0] * gx + Kinv[1, 1] * gy + Kinv[1, 2]
    rays = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=1)
    alpha = flat[1]
    hit = alpha > 0.0
    safe = np.where(hit, alpha, 1.0)
    expected = np.where(hit, flat[0] / safe, flat[0])                   # gaussian_renderer/__init__.py:69-79
    depth = expected * (1.0 - depth_ratio) + flat[5] * depth_ratio
    n_view = np.where(hit, flat[2:5] / safe, flat[2:5]).T               # (n,3)
    c2w = np.linalg.inv(np.asarray(view32, dtype=np.float32).astype(np.float64).reshape(4, 4))
    M = np.asarray(world_T_model, dtype=np.float64).reshape(4, 4) @ c2w
    points = (depth[:, None] * rays) @ M[:3, :3].T + M[:3, 3]
    normals = n_view @ M[:3, :3].T
    return points, normals
