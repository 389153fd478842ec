"""Reconstruction metrics between a reference cloud and an estimated mesh or cloud, on the device.

The reference answers "how good is the map" in utils/eval_utils.py (`evaluate_recon`, `nn_correspondance`,
`crop_union`) with Open3D: it samples the estimated mesh, voxel-down-samples both clouds and queries a KD-tree one
point at a time from Python.  Here the whole of `evaluate_recon` runs on the device: the mesh is sampled by one native
call (sls_mesh_sample: area-weighted, seeded), both clouds are down-sampled by one each (sls_voxel_downsample), the
nearest-neighbour search is one call (sls_nn_query: the spatial index of `distCUDA2`, queried by a second cloud) and
the metric block (eval_utils.py:122-153) two more (sls_nn_stats).  `evaluate_recon` reads the host twice: the status
words of the sampling and of both down-samples together, then the eight metric words.  Device tensors only; there is
no CPU path.

Open3D is not a dependency: voxel_down_sample and sample_points_uniformly are restated from their documented behaviour
(include/sls_cloud_math.h) with the two things Open3D leaves open — the order of the voxels, the random stream — defined
here, and pinned against NumPy restatements (tests/cloud_ref.py), not against Open3D itself.

`point_to_mesh` is the exact distance of points to a triangle mesh (sls_mesh_distance: the same box sweep over an index
of triangles, include/sls_meshdist_math.h) — unsigned, no BVH, not compared against Open3D's RaycastingScene;
`signed_distance` gives it a sign from the mesh's angle-weighted pseudo-normals (`mesh_pseudonormals`,
include/sls_signdist_math.h), and `evaluate_recon(signed=True)` reports the signed mean: bias, not only error.  With it
`evaluate_recon(completeness="exact")` measures every reference point against the mesh itself, not against samples
of it, and `error_map=True` returns where the mesh is wrong: the error map the reference's `evaluate_recon` announces
and raises NotImplementedError for (eval_utils.py:93-94, 131-133) — per-vertex distances to the reference cloud and
per-reference-point distances to the mesh, coloured by `error_colors` (sls_error_colors: green, yellow at half the
truncation, red at or beyond it).  The defaults of both are off and change nothing.

`cast_rays` is the other geometric query: the FIRST face a ray hits (sls_mesh_raycast: a second traversal of that same
index of triangles, ray against box; include/sls_raycast_math.h: the watertight test of Woop, Benthin and Wald, so no
ray passes between two faces that share an edge), `mesh_ray_index` the index built once for many casts, and
`render_mesh` the range image of a mesh from a camera in the pixel convention of `renderer.depth_to_points`.  No BVH,
rays cast in the caller's order; not compared against Open3D's `RaycastingScene.cast_rays`.

Not done here: reading files (splat_loam_amd/ply_io.py: load_point_cloud, load_mesh; tools/eval_recon.py puts the two
together).
"""
from __future__ import annotations

import ctypes
import math
import struct

import torch

from . import _abi


def _cloud(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    t = t.detach()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be (M,3)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _scratch(nbytes: int, device) -> tuple[torch.Tensor, int, int]:
    """A scratch buffer for a native call: (the tensor that owns it, its 256-byte aligned address, nbytes)."""
    buf = torch.empty((int(nbytes) + 256,), dtype=torch.uint8, device=device)
    return buf, (buf.data_ptr() + 255) & ~255, int(nbytes)


def _query(lib, target, query, want_index, scratch, st):
    Mt, Mq = int(target.shape[0]), int(query.shape[0])
    dist2 = torch.empty((Mq,), dtype=torch.float32, device=target.device)
    index = torch.empty((Mq,), dtype=torch.int32, device=target.device) if want_index else None
    if Mq:
        _, aligned, nbytes = scratch
        _abi.check(lib.sls_nn_query(Mt, target.data_ptr(), Mq, query.data_ptr(), dist2.data_ptr(),
                                    index.data_ptr() if want_index else None, aligned, nbytes, st), "sls_nn_query")
    return dist2, index


def nearest(target: torch.Tensor, query: torch.Tensor, return_index: bool = True):
    """For every row of `query` (Mq,3) its nearest row of `target` (Mt,3): `(dist2 (Mq,) float32, index (Mq,) int32)`,
    or `(dist2, None)` with `return_index=False`.  dist2 is fmaf(dz,dz,fmaf(dy,dy,dx*dx)) of the float32 differences
    (include/sls_nn_math.h) and index the lowest target row attaining it, bit for bit."""
    target, query = _cloud(target, "target"), _cloud(query, "query")
    if query.device != target.device:
        raise ValueError("target and query must live on the same device")
    if target.shape[0] == 0:
        raise ValueError("the target cloud is empty")
    lib = _abi.lib()
    with torch.cuda.device(target.device):
        st = torch.cuda.current_stream(target.device).cuda_stream
        scratch = _scratch(lib.sls_nn_scratch_bytes(int(target.shape[0]), int(query.shape[0])), target.device)
        return _query(lib, target, query, return_index, scratch, st)


NN_K_MAX = 32      # SLS_NN_K_MAX (include/sls_abi.h)


def _check_k(k, name: str, lo: int = 1, hi: int = NN_K_MAX) -> int:
    if isinstance(k, bool) or int(k) != k or not lo <= int(k) <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}]")
    return int(k)


def nearest_k(target: torch.Tensor, query: torch.Tensor, k: int, return_index: bool = True):
    """For every row of `query` (Mq,3) its `k` nearest rows of `target` (Mt,3), 1 <= k <= 32:
    `(dist2 (Mq,k) float32, index (Mq,k) int32)`, or `(dist2, None)` with `return_index=False`.  Row q is sorted by
    (dist2, index): nearer first, the lower target row first among equal distances, bit for bit
    (include/sls_outlier_math.h); with Mt < k the slots from Mt on hold +inf and -1.  A target that is the query's own
    copy is a target like any other: querying a cloud by itself gives every point itself first, at distance 0.
    `nearest_k(k=1)` equals `nearest`.  As for `nearest`, the coordinates must be finite: they are not checked, and what
    a row with a NaN or an infinity gets, or gives to others, is unspecified (every access stays inside the buffers)."""
    target, query = _cloud(target, "target"), _cloud(query, "query")
    k = _check_k(k, "k")
    if query.device != target.device:
        raise ValueError("target and query must live on the same device")
    if target.shape[0] == 0:
        raise ValueError("the target cloud is empty")
    Mt, Mq = int(target.shape[0]), int(query.shape[0])
    lib = _abi.lib()
    dev = target.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        dist2 = torch.empty((Mq, k), dtype=torch.float32, device=dev)
        index = torch.empty((Mq, k), dtype=torch.int32, device=dev) if return_index else None
        if Mq:
            _, aligned, nbytes = _scratch(lib.sls_nn_k_scratch_bytes(Mt, Mq, k), dev)
            _abi.check(lib.sls_nn_query_k(Mt, target.data_ptr(), Mq, query.data_ptr(), k, dist2.data_ptr(),
                                          index.data_ptr() if return_index else None, None, aligned, nbytes, st), "sls_nn_query_k")
    return dist2, index


NORMALS_NN_MAX = 64     # SLS_NORMALS_NN_MAX (include/sls_abi.h)


def _check_normals_args(radius, max_nn, viewpoint) -> tuple[float, int, tuple[float, float, float]]:
    k = _check_k(max_nn, "max_nn", 1, NORMALS_NN_MAX)
    radius = math.inf if radius is None else float(radius)
    if not radius > 0.0 or (radius > 3.0e38 and radius != math.inf):
        raise ValueError("radius must be a number > 0 that float32 holds, or None for the max_nn nearest at any distance")
    view = tuple(float(v) for v in viewpoint)
    if len(view) != 3 or not all(math.isfinite(v) for v in view):
        raise ValueError("viewpoint must be three finite numbers")
    return radius, k, view


def estimate_normals(points: torch.Tensor, radius=0.5, max_nn: int = 30, viewpoint=(0.0, 0.0, 0.0), return_details: bool = False):
    """Open3D's `estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))` followed by
    `orient_normals_towards_camera_location(viewpoint)`, restated (include/sls_normals_math.h; Open3D is not a dependency
    and the rule is pinned against a NumPy restatement, tests/normals_ref.py, not against Open3D itself).  The
    neighbourhood of point i is the part of its `max_nn` nearest points, ITSELF INCLUDED, with d2 <= radius * radius (one
    float32 product; `radius=None`: the `max_nn` nearest whatever their distance), n_i points from the exact list of
    `nearest_k`.  With n_i >= 3 the normal is the eigenvector of the smallest eigenvalue of the float64 covariance (cyclic
    Jacobi, + - * / and sqrt only, fixed order), flipped towards `viewpoint`; with n_i < 3 it is unit(viewpoint - p) — the
    reference's default -unit(point) for a viewpoint at the origin — or (0, 0, 1) for a point at the viewpoint.

    Returns `normals` (M,3) float32; with `return_details=True` `(normals, count (M,) int32 = n_i, eigenvalues (M,3)
    float32, ascending, zeros where n_i < 3)`.  1 <= max_nn <= 64.  One native call (sls_cloud_normals), no host read, no
    float atomics: the same cloud gives the same bits on every run, and the bits of the header compiled for the host.
    Device float32 (M,3) only; the coordinates must be finite (not checked; every access stays inside the buffers)."""
    res = _estimate_normals(points, radius, max_nn, viewpoint, return_details, False)
    return res if return_details else res[0]


def _estimate_normals(points, radius, max_nn, viewpoint, details: bool, lists: bool):
    """estimate_normals' call: (normals,), + (count, eigenvalues) with `details`, + (dist2 (M,k), index (M,k)) with `lists`
    — every point's neighbour list as `nearest_k` returns it, for max_nn up to 64, copied out of the scratch, where
    sls_cloud_normals leaves the rows (include/sls_abi.h).  For tests and tools/normals_bench.py."""
    points = _cloud(points, "points")
    radius, k, view = _check_normals_args(radius, max_nn, viewpoint)
    M = int(points.shape[0])
    lib = _abi.lib()
    dev = points.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        normals = torch.empty((M, 3), dtype=torch.float32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev) if details else None
        eig = torch.empty((M, 3), dtype=torch.float32, device=dev) if details else None
        rows = (torch.empty((M, k), dtype=torch.float32, device=dev), torch.empty((M, k), dtype=torch.int32, device=dev)) if lists else ()
        if M:
            buf, aligned, nbytes = _scratch(lib.sls_cloud_normals_scratch_bytes(M, k), dev)
            view3 = (ctypes.c_float * 3)(*view)                   # host memory, read before the call returns
            _abi.check(lib.sls_cloud_normals(M, points.data_ptr(), k, radius, ctypes.addressof(view3), normals.data_ptr(),
                                             count.data_ptr() if details else None, eig.data_ptr() if details else None,
                                             aligned, nbytes, st), "sls_cloud_normals")
            if lists:
                up = lambda v: (v + 255) & ~255
                a = aligned - buf.data_ptr() + up(int(lib.sls_nn_scratch_bytes(M, M)))
                b = a + up(4 * M * k)
                rows = (buf[a:a + 4 * M * k].view(torch.float32).view(M, k).clone(),
                        buf[b:b + 4 * M * k].view(torch.int32).view(M, k).clone())
    return (normals,) + ((count, eig) if details else ()) + tuple(rows)


GROUND_BINS = 504       # SLS_GROUND_BINS (include/sls_abi.h)
GROUND_STATES = ("EMPTY", "FEW", "DEGENERATE", "NOT_UPRIGHT", "ELEVATED_ROUGH", "GROUND")
GROUND_DEFAULTS = dict(min_range=2.7, max_range=80.0, th_seeds=0.5, th_dist=0.125, uprightness_thr=0.707, noise_margin=1.1,
                       elevation_thr=(0.523, 0.746, 0.879, 1.125), flatness_thr=(5e-4, 7.25e-4, 1e-3, 1e-3), num_lpr=20,
                       num_iter=3, num_min_pts=10)


def _check_ground_args(sensor_height, params) -> _abi.SlsGroundParams:
    """The parameters of segment_ground as the C struct, checked as sls_ground_segment checks them (before any work)."""
    unknown = sorted(set(params) - set(GROUND_DEFAULTS))
    if unknown:
        raise ValueError(f"unknown ground parameter {unknown[0]!r}; the parameters are {sorted(GROUND_DEFAULTS)}")
    p = dict(GROUND_DEFAULTS, sensor_height=sensor_height, **params)
    prm = _abi.SlsGroundParams()
    for name, value in p.items():
        if name.startswith("num_"):
            try:
                whole = not isinstance(value, bool) and int(value) == value and -2**31 <= int(value) < 2**31
            except (OverflowError, ValueError, TypeError):
                whole = False
            if not whole:
                raise ValueError(f"{name} must be an integer")
            setattr(prm, name, int(value))
            continue
        try:
            values = tuple(value) if name in ("elevation_thr", "flatness_thr") else (value,)
            values = tuple(ctypes.c_float(float(v)).value for v in values)      # what the C struct will hold ...
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be {'four numbers' if name in ('elevation_thr', 'flatness_thr') else 'a number'}") from None
        if name in ("elevation_thr", "flatness_thr") and len(values) != 4:
            raise ValueError(f"{name} must be four numbers")
        if not all(0.0 < v < math.inf for v in values):                         # ... is what sls_ground_segment checks
            raise ValueError(f"{name} must be finite and > 0 as a float32")
        setattr(prm, name, (ctypes.c_float * 4)(*values) if len(values) == 4 else values[0])
    if not prm.min_range < prm.max_range:
        raise ValueError("min_range must be below max_range")
    if not 1 <= prm.num_iter <= 8:
        raise ValueError("num_iter must be in [1, 8]")
    if prm.num_lpr < 1:
        raise ValueError("num_lpr must be >= 1")
    if prm.num_min_pts < 3:
        raise ValueError("num_min_pts must be >= 3")
    return prm


def _ground_enqueue(points: torch.Tensor, prm: _abi.SlsGroundParams, details: bool):
    """sls_ground_segment without a host read: (label (M,) uint8, bin (M,) int32, planes (BINS,8) float64, info (BINS,4)
    int32 | None, status (8,) int32)."""
    M = int(points.shape[0])
    lib = _abi.lib()
    dev = points.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        label = torch.empty((M,), dtype=torch.uint8, device=dev)
        bins = torch.empty((M,), dtype=torch.int32, device=dev)
        planes = torch.zeros((GROUND_BINS, 8), dtype=torch.float64, device=dev)
        info = torch.zeros((GROUND_BINS, 4), dtype=torch.int32, device=dev) if details else None
        status = torch.empty((8,), dtype=torch.int32, device=dev)
        _, aligned, nbytes = _scratch(lib.sls_ground_scratch_bytes(M), dev)
        _abi.check(lib.sls_ground_segment(M, points.data_ptr() if M else None, ctypes.byref(prm), label.data_ptr() if M else None,
                                          bins.data_ptr() if M else None, planes.data_ptr(),
                                          info.data_ptr() if details else None, status.data_ptr(), aligned if M else None,
                                          nbytes, st), "sls_ground_segment")
    return label, bins, planes, info, status


def segment_ground(points: torch.Tensor, sensor_height: float = 1.723, *, return_details: bool = False, **params):
    """The ground of a LiDAR scan (sensor frame, z up, the sensor `sensor_height` above the ground): a bool mask (M,).

    A region-wise ground-plane fit in the manner of Patchwork (Lim et al., RA-L 2021), RESTATED from the paper
    (include/sls_ground_math.h; patchwork / patchwork++ are not dependencies, no parity with them is claimed, and the rule is
    pinned against a NumPy restatement, tests/ground_ref.py): 504 bins of a concentric zone model whose sectors are cut in
    the diamond angle y / (|x| + |y|), not in azimuth; per bin the lowest points seed an iterated PCA plane fit (float64,
    Jacobi), and the bin's candidates are ground if its plane is upright and, near the sensor, not an elevated rough patch.
    `params`: min_range, max_range, th_seeds, th_dist, uprightness_thr, noise_margin, elevation_thr (4), flatness_thr (4),
    num_lpr, num_iter (1 ... 8), num_min_pts (>= 3); the defaults (GROUND_DEFAULTS) are a judgement, not verified values.
    Not here: Patchwork++'s reflected-noise removal, vertical plane fitting, adaptive thresholds, temporal revert,
    sensor-height estimation.

    With `return_details=True`: `(mask, bin (M,) int32, -1 = none, planes (504, 8) float64 = nx ny nz d mean_z and the
    eigenvalues ascending, info (504, 4) int32 = n, seeds, candidates, state (GROUND_STATES), status (8,) int32 = points
    with a bin, ground points, non-finite rows, GROUND bins, 0, 0, 0, 1)`.  One native call (sls_ground_segment), no host
    read, no float atomics: the same scan gives the same bits on every run, and the bits of the header compiled for the
    host.  Device float32 (M,3) only; rows with a non-finite coordinate are legal and never ground."""
    points = _cloud(points, "points")
    label, bins, planes, info, status = _ground_enqueue(points, _check_ground_args(sensor_height, params), return_details)
    mask = label.view(torch.bool)
    return (mask, bins, planes, info, status) if return_details else mask


def plane_normals(mask: torch.Tensor, bins: torch.Tensor, planes: torch.Tensor) -> torch.Tensor:
    """(M,3) float32 from `segment_ground`'s details: the bin's plane normal where `mask` is set, zeros elsewhere."""
    normals = planes[:, :3].to(torch.float32)[bins.long().clamp_(min=0)]
    return torch.where(mask.unsqueeze(1), normals, torch.zeros_like(normals))


def ground_normals(points: torch.Tensor, sensor_height: float = 1.723, *, return_mask: bool = False, **params):
    """Per-point normals (M,3) float32 from `segment_ground`: a ground point gets its bin's plane normal (unit, nz >= 0:
    up, towards the sensor), every other point zeros.  `return_mask=True`: `(normals, mask)`.  No host read."""
    points = _cloud(points, "points")
    label, bins, planes, _, _ = _ground_enqueue(points, _check_ground_args(sensor_height, params), False)
    mask = label.view(torch.bool)
    normals = plane_normals(mask, bins, planes)
    return (normals, mask) if return_mask else normals


def _normals(normals, points: torch.Tensor):
    if normals is None:
        return None
    normals = _cloud(normals, "normals")
    if normals.shape != points.shape or normals.device != points.device:
        raise ValueError("normals must have the shape and the device of points")
    return normals


def _outlier_enqueue(lib, call, name: str, points, normals, k: int, args: tuple, st):
    """One filter call without a host read: (rows (M,3), normals (M,3) | None, index (M,) int32, status (8,) int64)."""
    M = int(points.shape[0])
    dev = points.device
    out = torch.empty((M, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((M, 3), dtype=torch.float32, device=dev) if normals is not None else None
    index = torch.empty((M,), dtype=torch.int32, device=dev)
    status = torch.empty((8,), dtype=torch.int64, device=dev)
    _, aligned, nbytes = _scratch(lib.sls_outlier_scratch_bytes(M, k), dev)
    _abi.check(call(M, points.data_ptr() if M else None, normals.data_ptr() if (normals is not None and M) else None, *args,
                    out.data_ptr() if M else None, out_n.data_ptr() if (out_n is not None and M) else None,
                    index.data_ptr() if M else None, status.data_ptr(), aligned if M else None, nbytes, st), name)
    return out, out_n, index, status


def _kept_result(kept: int, out, out_n, index, details):
    """What the filters of a cloud return: the first `kept` rows of out, then — each where it is not None — of out_n and of
    index, then details; the rows alone without any of these."""
    res = [out[:kept]] + [t[:kept] for t in (out_n, index) if t is not None] + ([details] if details is not None else [])
    return res[0] if len(res) == 1 else tuple(res)


def _outlier_result(out, out_n, index, words, has_normals: bool, return_index: bool, details: bool):
    bits = lambda v: struct.unpack("<d", struct.pack("<q", v))[0]
    kept = int(words[0])
    det = {"kept": kept, "removed": int(words[5]) - kept, "zero_mean": int(words[1]), "cloud_mean": bits(words[2]),
           "std": bits(words[3]), "threshold": bits(words[4])} if details else None
    return _kept_result(kept, out, out_n if has_normals else None, index if return_index else None, det)


def _check_stat_args(nb_neighbors, std_ratio) -> tuple[int, float]:
    k = _check_k(nb_neighbors, "nb_neighbors")
    std_ratio = float(std_ratio)
    if not (std_ratio > 0.0 and math.isfinite(std_ratio)):
        raise ValueError("std_ratio must be a finite number > 0")
    return k, std_ratio


def remove_statistical_outlier(points: torch.Tensor, nb_neighbors: int = 20, std_ratio: float = 2.0, normals=None,
                               return_index: bool = False, details: bool = False):
    """Open3D's `remove_statistical_outlier`, restated (include/sls_outlier_math.h; Open3D is not a dependency and the
    rule is pinned against a NumPy restatement, tests/outlier_ref.py, not against Open3D itself).  mean_i is the mean
    distance of point i to its `nb_neighbors` nearest points, ITSELF INCLUDED (at distance 0: the cloud is queried
    by itself): float32 roots of the exact neighbour list of `nearest_k`, summed in float64.
    With n = M: cloud_mean = sum{mean_i > 0} mean_i / n, std = sqrt(sum{mean_i > 0} (mean_i - cloud_mean)^2 / (n - 1)),
    and point i is kept iff mean_i > 0 and mean_i < cloud_mean + std_ratio * std.  Three consequences: a point whose
    nb_neighbors - 1 nearest others are exact copies of it is removed; nb_neighbors = 1 removes everything; a cloud of
    one point loses it.  One native call (sls_outlier_statistical), fixed-order float64 sums — the same cloud gives the
    same bits on every run — and one host read (the status words).

    Returns the kept rows in their original order, (kept,3) float32; then, in this order, the kept rows of `normals`
    where given, with `return_index=True` their original row numbers (kept,) int32, with `details=True` a dict: kept,
    removed, zero_mean (points with mean 0), cloud_mean, std, threshold.  1 <= nb_neighbors <= 32, std_ratio > 0.
    As for `nearest`, the coordinates must be finite: they are not checked, and a NaN or an infinity makes the result
    unspecified (every access stays inside the buffers)."""
    points = _cloud(points, "points")
    k, std_ratio = _check_stat_args(nb_neighbors, std_ratio)
    normals = _normals(normals, points)
    lib = _abi.lib()
    with torch.cuda.device(points.device):
        st = torch.cuda.current_stream(points.device).cuda_stream
        out, out_n, index, status = _outlier_enqueue(lib, lib.sls_outlier_statistical, "sls_outlier_statistical", points, normals,
                                                     k, (k, std_ratio), st)
        words = status.cpu().tolist()                                       # the one host read
    return _outlier_result(out, out_n, index, words, normals is not None, return_index, details)


def remove_radius_outlier(points: torch.Tensor, nb_points: int, radius: float, normals=None, return_index: bool = False,
                          details: bool = False):
    """Keep the points with MORE than `nb_points` points, themselves included, within `radius`: d2 <= radius * radius,
    one float32 product, d2 the exact float32 expression of `nearest`.  This is the project's rule; whether Open3D's
    `remove_radius_outlier` puts its boundary at < or <= was not verified.  0 <= nb_points <= 31, radius > 0.  One
    native call (sls_outlier_radius), one host read.  Returns as `remove_statistical_outlier`; the details hold kept
    and removed.  Coordinates must be finite, as there."""
    points = _cloud(points, "points")
    nb = _check_k(nb_points, "nb_points", 0, NN_K_MAX - 1)
    radius = float(radius)
    if not (radius > 0.0 and math.isfinite(radius) and radius <= 3.0e38):
        raise ValueError("radius must be a finite number > 0")
    normals = _normals(normals, points)
    lib = _abi.lib()
    with torch.cuda.device(points.device):
        st = torch.cuda.current_stream(points.device).cuda_stream
        out, out_n, index, status = _outlier_enqueue(lib, lib.sls_outlier_radius, "sls_outlier_radius", points, normals, nb + 1,
                                                     (nb, radius), st)
        words = status.cpu().tolist()                                       # the one host read
    res = _outlier_result(out, out_n, index, words, normals is not None, return_index, details)
    if details:
        for key in ("zero_mean", "cloud_mean", "std", "threshold"):
            res[-1].pop(key)                                                # (the statistical filter's words)
    return res


CLUSTER_STATUS_WORDS = 8        # SLS_CLUSTER_STATUS_WORDS, and behind them the SLS_CLUSTER_SELECT_STATUS_WORDS = 4 of the selection
INT32_MAX = 2 ** 31 - 1


def _check_cluster_args(eps, min_points) -> tuple[float, int]:
    """(eps, min_points) as sls_cloud_dbscan accepts them — before any launch."""
    eps = float(eps)
    f32 = struct.unpack("<f", struct.pack("<f", eps))[0] if math.isfinite(eps) and abs(eps) <= 3.4028234663852886e38 else math.inf
    if not (eps > 0.0 and math.isfinite(f32) and f32 > 0.0 and f32 * f32 <= 3.4028234663852886e38):
        raise ValueError("eps must be a finite number > 0 whose square is a finite float32")
    if isinstance(min_points, bool) or int(min_points) != min_points or not 1 <= int(min_points) <= INT32_MAX:
        raise ValueError("min_points must be an integer >= 1")
    return f32, int(min_points)


def _check_select_args(keep, min_cluster_points) -> tuple[int, int]:
    for name, v in (("keep", keep), ("min_cluster_points", min_cluster_points)):
        if isinstance(v, bool) or int(v) != v or not -INT32_MAX <= int(v) <= INT32_MAX:
            raise ValueError(f"{name} must be an integer")
    return int(keep), int(min_cluster_points)


def _dbscan_enqueue(lib, points, eps: float, min_points: int, status: torch.Tensor, st):
    """sls_cloud_dbscan without a host read: (labels (M,) int32, counts (M,) int32: the first C entries); status: 8 int32."""
    M = int(points.shape[0])
    dev = points.device
    labels = torch.empty((M,), dtype=torch.int32, device=dev)
    counts = torch.empty((M,), dtype=torch.int32, device=dev)
    _, aligned, nbytes = _scratch(lib.sls_cloud_dbscan_scratch_bytes(M), dev)
    _abi.check(lib.sls_cloud_dbscan(M, points.data_ptr() if M else None, eps, min_points, labels.data_ptr() if M else None,
                                    counts.data_ptr() if M else None, status.data_ptr(), aligned if M else None, nbytes, st),
               "sls_cloud_dbscan")
    return labels, counts


def _cluster_details(words) -> dict:
    return {"clusters": int(words[0]), "core": int(words[1]), "border": int(words[2]), "noise": int(words[3]),
            "largest": int(words[4])}


def cluster_dbscan(points: torch.Tensor, eps: float, min_points: int = 10, return_counts: bool = False, details: bool = False):
    """DBSCAN over exact radius neighbours (include/sls_cluster_math.h), with the border rule of Open3D's `cluster_dbscan`
    as restated there — Open3D is not a dependency and no parity is claimed; the rule is pinned against a NumPy
    restatement (tests/cluster_ref.py) and the header's all-pairs routine.  t is a neighbour of q iff
    d2 <= eps * eps (one float32 product, d2 the exact float32 expression of `nearest`), itself and exact copies
    included; a point is core iff at least `min_points` points are its neighbours; the clusters are the connected
    components of the cores, numbered in ascending order of their lowest core index; a non-core point with a core
    neighbour takes the lowest cluster number among its core neighbours' clusters and connects nothing; the rest is
    noise, -1.  Integers and one comparison: the same cloud gives the same bytes on every run.

    The cost grows with the number of pairs within eps — eps is meant to be a few point spacings; many spacings on
    millions of points is quadratic, as it is anywhere.  min_points = 10 is a judgement.

    Returns labels (M,) int32; with `return_counts=True` then counts (C,) int32, the points of every cluster; with
    `details=True` then a dict: clusters, core, border, noise, largest.  One native call (sls_cloud_dbscan), one host
    read (the status words).  Coordinates must be finite, as for `nearest`."""
    points = _cloud(points, "points")
    eps, min_points = _check_cluster_args(eps, min_points)
    lib = _abi.lib()
    dev = points.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        status = torch.empty((CLUSTER_STATUS_WORDS,), dtype=torch.int32, device=dev)
        labels, counts = _dbscan_enqueue(lib, points, eps, min_points, status, st)
        words = status.cpu().tolist()                                       # the one host read
    res = [labels]
    if return_counts:
        res.append(counts[:int(words[0])])
    if details:
        res.append(_cluster_details(words))
    return res[0] if len(res) == 1 else tuple(res)


def keep_clusters(points: torch.Tensor, eps: float, min_points: int = 10, keep: int = 1, min_cluster_points: int = 0, normals=None,
                  return_index: bool = False, details: bool = False):
    """The large pieces of a cloud: `cluster_dbscan(eps, min_points)`, then the rule of `mesh_ops`' cluster filter over
    its clusters — n_min = max(max(min_cluster_points, 0), the min(keep, C)-th largest count), the second term 0 for
    keep <= 0; a point stays iff it has a cluster and that cluster holds at least n_min points (clusters that tie at the
    keep-th place all stay; noise always goes).  Two native calls back to back (sls_cloud_dbscan, sls_cloud_select), ONE
    host read in total.  keep = 1 is a judgement.

    Returns as `remove_statistical_outlier`: the kept rows in their original order, (kept,3) float32; then the kept rows
    of `normals` where given, with `return_index=True` their original row numbers (kept,) int32, with `details=True` a
    dict: kept, removed, n_min and the words of `cluster_dbscan`."""
    points = _cloud(points, "points")
    eps, min_points = _check_cluster_args(eps, min_points)
    keep, min_cluster_points = _check_select_args(keep, min_cluster_points)
    normals = _normals(normals, points)
    lib = _abi.lib()
    dev = points.device
    M = int(points.shape[0])
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        status = torch.empty((CLUSTER_STATUS_WORDS + 4,), dtype=torch.int32, device=dev)
        labels, counts = _dbscan_enqueue(lib, points, eps, min_points, status, st)
        out = torch.empty((M, 3), dtype=torch.float32, device=dev)
        out_n = torch.empty((M, 3), dtype=torch.float32, device=dev) if normals is not None else None
        index = torch.empty((M,), dtype=torch.int32, device=dev) if return_index else None
        _, aligned, nbytes = _scratch(lib.sls_cloud_select_scratch_bytes(M), dev)
        ptr = lambda t: t.data_ptr() if (t is not None and M) else None
        _abi.check(lib.sls_cloud_select(M, ptr(points), ptr(normals), ptr(labels), ptr(counts), status.data_ptr() if M else None, keep,
                                        min_cluster_points, ptr(out), ptr(out_n), ptr(index), status[CLUSTER_STATUS_WORDS:].data_ptr(),
                                        aligned if M else None, nbytes, st), "sls_cloud_select")
        words = status.cpu().tolist()                                       # the one host read
    kept = int(words[CLUSTER_STATUS_WORDS])
    det = {"kept": kept, "removed": M - kept, "n_min": int(words[CLUSTER_STATUS_WORDS + 1]), **_cluster_details(words)} if details else None
    return _kept_result(kept, out, out_n, index, det)


ICP_METHODS = {"plane": 0, "point": 1}                # SLS_ICP_PLANE, SLS_ICP_POINT (include/sls_abi.h)
ICP_STATUS_WORDS = 20                                   # SLS_ICP_STATUS_WORDS
ICP_MAX_ITERATIONS = 1000                               # SLS_ICP_MAX_ITERATIONS
ICP_FLAG_CONVERGED, ICP_FLAG_FEW, ICP_FLAG_NOT_PD = 1, 2, 4
# a judgement, as in include/sls_icp_math.h (sls_icp_defaults), where the reasons are given
ICP_DEFAULTS = dict(damping=1e-9, eps_rot=1e-7, eps_trans=1e-7, min_inliers=6)


def _check_icp_args(max_distance, iterations, method, init, params) -> tuple[_abi.SlsIcpParams, list]:
    """The parameters of register_icp as the C struct and the initial pose as 12 floats, checked as sls_cloud_icp checks
    them (before any work)."""
    unknown = sorted(set(params) - set(ICP_DEFAULTS))
    if unknown:
        raise ValueError(f"unknown ICP parameter {unknown[0]!r}; the parameters are {sorted(ICP_DEFAULTS)}")
    if method not in ICP_METHODS:
        raise ValueError(f"method must be one of {sorted(ICP_METHODS)}")
    p = dict(ICP_DEFAULTS, **params)
    prm = _abi.SlsIcpParams()
    prm.method = ICP_METHODS[method]
    prm.iterations = _check_k(iterations, "iterations", 0, ICP_MAX_ITERATIONS)
    prm.min_inliers = _check_k(p["min_inliers"], "min_inliers", 0, 2**31 - 1)
    try:
        gate = ctypes.c_float(float(max_distance)).value                    # what the C struct will hold
    except (TypeError, ValueError):
        raise ValueError("max_distance must be a number") from None
    if not 0.0 < gate < math.inf:
        raise ValueError("max_distance must be finite and > 0 as a float32")
    prm.max_distance = gate
    for name in ("damping", "eps_rot", "eps_trans"):
        try:
            v = float(p[name])
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number") from None
        if not 0.0 <= v < math.inf:
            raise ValueError(f"{name} must be a finite number >= 0")
        setattr(prm, name, v)
    if init is None:
        pose = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    else:
        t = (init.detach() if isinstance(init, torch.Tensor) else torch.as_tensor(init, dtype=torch.float64)).to("cpu", torch.float64)
        if tuple(t.shape) == (4, 4):
            t = t[:3]
        if t.numel() != 12 or tuple(t.shape) not in ((3, 4), (12,)):
            raise ValueError("init must be a 4x4 or 3x4 matrix, or 12 numbers (row-major 3x4 target_T_source)")
        pose = [float(v) for v in t.reshape(-1).tolist()]
        if not all(math.isfinite(v) for v in pose):
            raise ValueError("init must be finite")
    return prm, pose


def _icp_enqueue(lib, source, target, normals, prm: _abi.SlsIcpParams, pose12, details: bool, st):
    """sls_cloud_icp without a host read: (status (20,) int64, system (32,) float64 | None, index (Ms,) int32 | None,
    dist2 (Ms,) float32 | None)."""
    Ms, Mt = int(source.shape[0]), int(target.shape[0])
    dev = target.device
    status = torch.empty((ICP_STATUS_WORDS,), dtype=torch.int64, device=dev)
    system = torch.empty((32,), dtype=torch.float64, device=dev) if details else None
    index = torch.empty((Ms,), dtype=torch.int32, device=dev) if details else None
    dist2 = torch.empty((Ms,), dtype=torch.float32, device=dev) if details else None
    _, aligned, nbytes = _scratch(lib.sls_cloud_icp_scratch_bytes(Ms, Mt), dev)
    init = (ctypes.c_double * 12)(*pose12)                                  # host memory, read before the call returns
    _abi.check(lib.sls_cloud_icp(Ms, source.data_ptr() if Ms else None, Mt, target.data_ptr(),
                                 normals.data_ptr() if normals is not None else None, ctypes.byref(prm), ctypes.addressof(init),
                                 status.data_ptr(), system.data_ptr() if details else None,
                                 index.data_ptr() if (details and Ms) else None, dist2.data_ptr() if (details and Ms) else None,
                                 aligned, nbytes, st), "sls_cloud_icp")
    return status, system, index, dist2


def _icp_result(words) -> dict:
    """The status words of sls_cloud_icp as register_icp returns them."""
    bits = lambda v: struct.unpack("<d", struct.pack("<q", v))[0]
    inliers, Ms, flags, sum_r2 = int(words[1]), int(words[2]), int(words[4]), bits(words[5])
    pose = torch.eye(4, dtype=torch.float64)
    pose[:3] = torch.tensor([bits(w) for w in words[6:18]], dtype=torch.float64).view(3, 4)
    return {"target_T_source": pose, "fitness": inliers / Ms if Ms else 0.0,
            "inlier_rmse": math.sqrt(sum_r2 / inliers) if inliers else 0.0, "inliers": inliers, "sum_r2": sum_r2,
            "updates": int(words[0]), "converged": bool(flags & ICP_FLAG_CONVERGED), "too_few_inliers": bool(flags & ICP_FLAG_FEW),
            "not_positive_definite": bool(flags & ICP_FLAG_NOT_PD), "flags": flags}


def register_icp(source: torch.Tensor, target: torch.Tensor, target_normals=None, init=None, max_distance: float = 1.0,
                 iterations: int = 30, method: str = "plane", return_details: bool = False, **params):
    """Register `source` (Ms,3) onto `target` (Mt,3): Gauss-Newton ICP on the EXACT nearest neighbours of `nearest`, with
    a hard distance gate (a pair counts iff d2 <= max_distance * max_distance, one float32 product) and NO robust weight
    (include/sls_icp_math.h; pinned against a NumPy restatement, tests/icp_ref.py).  `method="plane"` minimises
    n . (R p + t - q) over the target's normals, `"point"` the distances themselves.  It is NOT a global registration:
    `init` (4x4, 3x4 or 12 numbers, default the identity) must bring the clouds within the gate.  No multi-scale, no
    robust kernel; not Open3D's `registration_icp`, which is not a dependency, and no parity with it is claimed.

    `iterations` (0 ... 1000) updates at most, then one evaluation pass at the final pose; the updates end early once a
    step is below `eps_rot` / `eps_trans` (converged), or when fewer than `min_inliers` pairs pass the gate or the damped
    system is not positive definite (the pose is then kept).  `params`: damping, eps_rot, eps_trans, min_inliers; the
    defaults (ICP_DEFAULTS) are a judgement.

    Returns a dict: `target_T_source` (4x4 float64, CPU), `fitness` = inliers / Ms, `inlier_rmse` = sqrt(sum r^2 /
    inliers) of the final pose (r: the plane distance, or the point distance), `inliers`, `sum_r2`, `updates`,
    `converged`, `too_few_inliers`, `not_positive_definite`, `flags`.  With `return_details=True` also `system` (32,)
    float64 — the 29 sums of the last linearisation — and the last association, `index` (Ms,) int32 and `dist2` (Ms,)
    float32, all on the device.  ONE native call (sls_cloud_icp) and ONE host read, of the status words; with
    `method="plane"` and no `target_normals` it first calls `estimate_normals(target)` — a second native call, still no
    further host read.  Fixed-order float64 sums, no float atomics: the same input gives the same bits on every run.
    Device float32 (M,3) only; coordinates and normals must be finite (not checked)."""
    source, target = _cloud(source, "source"), _cloud(target, "target")
    if source.device != target.device:
        raise ValueError("source and target must live on the same device")
    if target.shape[0] == 0:
        raise ValueError("the target cloud is empty")
    prm, pose12 = _check_icp_args(max_distance, iterations, method, init, params)
    normals = _normals(target_normals, target) if method == "plane" else None
    if method == "plane" and normals is None:
        normals = estimate_normals(target)
    lib = _abi.lib()
    with torch.cuda.device(target.device):
        st = torch.cuda.current_stream(target.device).cuda_stream
        status, system, index, dist2 = _icp_enqueue(lib, source, target, normals, prm, pose12, return_details, st)
        res = _icp_result(status.cpu().tolist())                            # the one host read
    if return_details:
        res.update(system=system, index=index, dist2=dist2)
    return res


def transform_points(points: torch.Tensor, pose: torch.Tensor) -> torch.Tensor:
    """(M,3) float32: R p + t for a 4x4 (or 3x4) pose, computed in float64 on the points' device and rounded once."""
    pose = torch.as_tensor(pose, dtype=torch.float64).to(points.device)
    return (points.double() @ pose[:3, :3].T + pose[:3, 3]).float()


def crop_union_mask(reference: torch.Tensor, estimate: torch.Tensor, threshold_dist: float = 1.2) -> torch.Tensor:
    """bool (Mref,): the reference points with an estimate point nearer than `threshold_dist` — `crop_union`
    (eval_utils.py:202-250) after its mesh sampling; `estimate` is the merged cloud of all methods.  The comparison is
    dist2 < threshold_dist² in float32, on the device."""
    dist2, _ = nearest(estimate, reference, return_index=False)
    t = torch.tensor(float(threshold_dist), dtype=torch.float32)
    return dist2 < float(t * t)


def cloud_metrics(reference: torch.Tensor, estimate: torch.Tensor, threshold: float = 0.2, truncation_acc: float = 0.5,
                  truncation_com: float = 0.5) -> dict:
    """The metric block of `evaluate_recon` (eval_utils.py:122-153) for two point clouds, in metres and fractions.

    Accuracy: every estimate point against the reference cloud, points farther than `truncation_acc` dropped.
    Completeness: every reference point against the estimate cloud, points farther than `truncation_com` counted as
    `truncation_com`.  precision / recall: the fraction of either set below `threshold`.  An empty accuracy set gives
    NaN for `accuracy_m` and `precision` (the reference's mean of an empty array); `fscore` is 0.0 when
    precision + recall is 0."""
    reference, estimate = _cloud(reference, "reference"), _cloud(estimate, "estimate")
    if reference.device != estimate.device:
        raise ValueError("reference and estimate must live on the same device")
    Mr, Me = int(reference.shape[0]), int(estimate.shape[0])
    if Mr == 0 or Me == 0:
        raise ValueError("both clouds need at least one point")
    lib = _abi.lib()
    dev = reference.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        scratch = _scratch(lib.sls_nn_scratch_bytes(max(Mr, Me), max(Mr, Me)), dev)
        _, aligned, nbytes = scratch
        words = torch.empty((8,), dtype=torch.int64, device=dev)
        d_acc, _ = _query(lib, reference, estimate, False, scratch, st)
        _abi.check(lib.sls_nn_stats(Me, d_acc.data_ptr(), float(truncation_acc), float(threshold), 0, words.data_ptr(),
                                    aligned, nbytes, st), "sls_nn_stats")
        d_com, _ = _query(lib, estimate, reference, False, scratch, st)
        _abi.check(lib.sls_nn_stats(Mr, d_com.data_ptr(), float(truncation_com), float(threshold), 1,
                                    words.data_ptr() + 32, aligned, nbytes, st), "sls_nn_stats")
        w = words.cpu().tolist()                                  # the one host read
    return _metrics(w, threshold, truncation_acc, truncation_com)


def _metrics(w, threshold, truncation_acc, truncation_com) -> dict:
    """cloud_metrics' dict from the eight words of its two sls_nn_stats calls."""
    bits = lambda v: struct.unpack("<d", struct.pack("<q", v))[0]
    n_acc, below_acc, sum_acc = w[0], w[1], bits(w[2])
    n_com, below_com, sum_com = w[4], w[5], bits(w[6])
    accuracy = sum_acc / n_acc if n_acc else math.nan
    precision = below_acc / n_acc if n_acc else math.nan
    completeness = sum_com / n_com
    recall = below_com / n_com
    pr = precision + recall
    fscore = 2.0 * precision * recall / pr if pr != 0 else 0.0
    return {
        "accuracy_m": accuracy, "completeness_m": completeness, "chamfer_l1_m": 0.5 * (accuracy + completeness),
        "precision": precision, "recall": recall, "fscore": fscore,
        "n_accuracy": int(n_acc), "n_completeness": int(n_com),
        "threshold": float(threshold), "truncation_acc": float(truncation_acc), "truncation_com": float(truncation_com),
    }


def _voxel_enqueue(lib, points: torch.Tensor, voxel_size: float, want_counts: bool, st):
    """sls_voxel_downsample without a host read: (rows (M,3), counts (M,) | None, status (4,) int32)."""
    M = int(points.shape[0])
    dev = points.device
    out = torch.empty((M, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((M,), dtype=torch.int32, device=dev) if want_counts else None
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    scratch, aligned, nbytes = _scratch(lib.sls_voxel_scratch_bytes(M), dev)
    _abi.check(lib.sls_voxel_downsample(M, points.data_ptr() if M else None, float(voxel_size), out.data_ptr() if M else None,
                                        counts.data_ptr() if (want_counts and M) else None, status.data_ptr(),
                                        aligned if M else None, nbytes, st), "sls_voxel_downsample")
    return out, counts, status


def _voxel_status(words, what: str) -> int:
    """n_voxels from the three status words of one down-sample; ValueError where the cloud could not be served."""
    n_voxels, n_nonfinite, n_big = (int(w) & 0xFFFFFFFF for w in words[:3])
    if n_nonfinite:
        raise ValueError(f"{what}: {n_nonfinite} points have a non-finite coordinate")
    if n_big:
        raise ValueError(f"{what}: {n_big} points lie more than 2^21 voxels from the cloud's minimum; the voxel size is too "
                         "small for the cloud's extent")
    return n_voxels


def _check_voxel_size(voxel_size) -> float:
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
        raise ValueError("voxel_size must be a finite number > 0")
    return voxel_size


def voxel_down_sample(points: torch.Tensor, voxel_size: float, return_counts: bool = False):
    """Open3D's `voxel_down_sample` for points: one row per occupied voxel, the mean of the voxel's points — float64
    sums, rounded to float32 once.  Voxel (ix, iy, iz) of a point is floor((p - (min - voxel_size / 2)) / voxel_size) per
    axis in float64 (include/sls_cloud_math.h); the rows come in ascending order of ix | iy << 21 | iz << 42 (Open3D's
    order is that of a hash map: unspecified).  The same cloud gives the same bits on every run.  `return_counts=True`
    adds the number of points of every voxel, (n_voxels,) int32.  One host read (the status words).
    ValueError: a non-finite coordinate, or a cloud wider than 2^21 voxels along an axis."""
    points = _cloud(points, "points")
    voxel_size = _check_voxel_size(voxel_size)
    lib = _abi.lib()
    with torch.cuda.device(points.device):
        st = torch.cuda.current_stream(points.device).cuda_stream
        out, counts, status = _voxel_enqueue(lib, points, voxel_size, return_counts, st)
        n = _voxel_status(status.cpu().tolist(), "voxel_down_sample")      # the one host read
    return (out[:n], counts[:n]) if return_counts else out[:n]


def _mesh(vertices: torch.Tensor, faces: torch.Tensor):
    vertices = _cloud(vertices, "vertices")
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise RuntimeError("faces must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise ValueError("faces must be an integer tensor of shape (F,3)")
    if faces.device != vertices.device:
        raise ValueError("vertices and faces must live on the same device")
    faces = faces.detach()
    if faces.dtype != torch.int32:
        faces = faces.to(torch.int32)
    return vertices, faces.contiguous()


def _mesh_enqueue(lib, vertices, faces, n: int, seed: int, crop_box, want_faces: bool, st):
    """sls_mesh_sample without a host read: (points (n,3), face (n,) | None, status (4,) int32)."""
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev) if want_faces else None
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    scratch, aligned, nbytes = _scratch(lib.sls_mesh_sample_scratch_bytes(V, F, n), dev)
    _abi.check(lib.sls_mesh_sample(V, vertices.data_ptr() if V else None, F, faces.data_ptr() if F else None,
                                   crop_box.data_ptr() if crop_box is not None else None, n, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   out.data_ptr() if n else None, face.data_ptr() if (want_faces and n) else None,
                                   status.data_ptr(), aligned, nbytes, st), "sls_mesh_sample")
    return out, face, status


def _mesh_status(words, n: int) -> None:
    written, n_bad, no_area = (int(w) & 0xFFFFFFFF for w in words[:3])
    if n_bad:
        raise ValueError(f"sample_mesh: {n_bad} faces have a vertex index outside the vertices")
    if n and (no_area or written != n):
        raise ValueError("sample_mesh: the mesh has no area to sample (no face, or every face is degenerate or cropped away)")


def _crop_box(crop_box, device):
    if crop_box is None:
        return None
    box = torch.as_tensor(crop_box, dtype=torch.float32).to(device).reshape(-1).contiguous()
    if box.numel() != 6:
        raise ValueError("crop_box must hold six numbers: min xyz, max xyz")
    return box


def sample_mesh(vertices: torch.Tensor, faces: torch.Tensor, n: int, seed: int = 0, crop_box=None, return_faces: bool = False):
    """`n` points drawn uniformly from the surface of a triangle mesh — Open3D's `sample_points_uniformly` with a seeded,
    defined random stream: sample i is a pure function of (mesh, crop box, seed, i), so a rerun gives the same cloud and
    a longer draw starts with the shorter one.  A face is drawn in proportion to its float64 area, quantised to 2^-32 of
    the largest area (smaller faces are never drawn); `crop_box` (six numbers or a device tensor: min xyz, max xyz)
    keeps only the faces whose three vertices lie inside the closed box, as Open3D's `crop` does.  (n,3) float32, with
    `return_faces=True` also the face of every point, (n,) int32.  One host read (the status words).
    ValueError: a vertex index outside the vertices, or no face with area left."""
    vertices, faces = _mesh(vertices, faces)
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    lib = _abi.lib()
    dev = vertices.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        out, face, status = _mesh_enqueue(lib, vertices, faces, n, seed, _crop_box(crop_box, dev), return_faces, st)
        _mesh_status(status.cpu().tolist(), n)                              # the one host read
    return (out, face) if return_faces else out


def _mesh_distance_enqueue(lib, points, vertices, faces, want_face: bool, want_closest: bool, st):
    """sls_mesh_distance without a host read: (dist2 (M,), face (M,) | None, closest (M,3) | None, status (4,) int32,
    scratch) — the scratch serves a following sls_nn_stats."""
    dev = vertices.device
    V, F, M = int(vertices.shape[0]), int(faces.shape[0]), int(points.shape[0])
    if V < 1 or F < 1:
        raise ValueError("the mesh needs at least one vertex and one face")
    dist2 = torch.empty((M,), dtype=torch.float32, device=dev)
    face = torch.empty((M,), dtype=torch.int32, device=dev) if want_face else None
    closest = torch.empty((M, 3), dtype=torch.float32, device=dev) if want_closest else None
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    scratch = _scratch(lib.sls_mesh_distance_scratch_bytes(V, F, M), dev)
    _abi.check(lib.sls_mesh_distance(V, vertices.data_ptr(), F, faces.data_ptr(), M, points.data_ptr() if M else None,
                                     dist2.data_ptr() if M else None, face.data_ptr() if (want_face and M) else None,
                                     closest.data_ptr() if (want_closest and M) else None, status.data_ptr(), scratch[1],
                                     scratch[2], st), "sls_mesh_distance")
    return dist2, face, closest, status, scratch


def _mesh_distance_status(words, what: str) -> None:
    _, n_index, n_nonfinite = (int(w) & 0xFFFFFFFF for w in words[:3])
    if n_index:
        raise ValueError(f"{what}: {n_index} faces have a vertex index outside the vertices")
    if n_nonfinite:
        raise ValueError(f"{what}: {n_nonfinite} faces have a vertex with a non-finite coordinate")


def point_to_mesh(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, return_face: bool = True,
                  return_closest: bool = False):
    """The exact, UNSIGNED distance of every row of `points` (M,3) to the triangle mesh (`vertices` (V,3), `faces` (F,3)
    integers): `dist2` (M,) float32, the squared distance to the nearest face as include/sls_meshdist_math.h defines it
    (the minimum over points that lie on the triangle: its three edge segments and the plane's foot point where that
    falls inside; a zero-area face is its segment or its point); with `return_face` (the default) also `face` (M,)
    int32, the lowest face index among those of equal dist2 bits; with `return_closest` also `closest` (M,3) float32,
    the nearest point of that face.  Returned as `dist2`, `(dist2, face)`, `(dist2, closest)` or `(dist2, face, closest)`.

    dist2 and closest are the bits of the header compiled for the host for (point, returned face); the float64
    distance to the returned face exceeds the true minimum over all faces by no more than 1e-5 of the scale (the
    largest distance from the point to that face's vertices; measured: DESIGN.md section 7).  Outside a convex mesh a
    point nearest to a shared edge or vertex has several faces at the same true distance: which of them is named is
    decided by float32 bits, then by the lower index.  One native call (sls_mesh_distance), one host read (the status
    words), no float atomics: the same input gives the same bits on every run.

    The signed twin is `signed_distance`.  There is no BVH: the faces are
    indexed in the curve order of their centroids, in runs of 32 whose boxes bound all three vertices, so a few huge
    triangles among many small ones make their runs' boxes loose — that costs time, never exactness.  Device tensors
    only; the points must be finite (not checked; every access stays inside the buffers).
    ValueError: a face with a vertex index outside the vertices or with a non-finite vertex; an empty mesh."""
    points = _cloud(points, "points")
    vertices, faces = _mesh(vertices, faces)
    if points.device != vertices.device:
        raise ValueError("the points and the mesh must live on the same device")
    lib = _abi.lib()
    dev = vertices.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        dist2, face, closest, status, _ = _mesh_distance_enqueue(lib, points, vertices, faces, bool(return_face),
                                                                 bool(return_closest), st)
        _mesh_distance_status(status.cpu().tolist(), "point_to_mesh")          # the one host read
    res = (dist2,) + ((face,) if return_face else ()) + ((closest,) if return_closest else ())
    return res[0] if len(res) == 1 else res


def _check_truncation(truncation) -> float:
    try:
        t = ctypes.c_float(float(truncation)).value                             # what the native call will see
    except (TypeError, ValueError):
        raise ValueError("truncation must be a number") from None
    if not 0.0 < t < math.inf:
        raise ValueError("truncation must be finite and > 0 as a float32")
    return t


def error_colors(dist2: torch.Tensor, truncation: float) -> torch.Tensor:
    """(M,3) uint8 RGB of squared distances (M,) at `truncation` metres (include/sls_meshdist_math.h): with
    t = sqrt(dist2) / truncation in float32 and L = 255 for t >= 1, else int(t * 256): (2 L, 255, 0) up to L = 127, then
    (255, 2 (255 - L), 0) — green is good, yellow is at half the truncation, red at or beyond it; a NaN gives blue
    (0, 0, 255).  One native call (sls_error_colors), no host read."""
    if not isinstance(dist2, torch.Tensor) or not dist2.is_cuda:
        raise RuntimeError("dist2 must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    if dist2.dim() != 1:
        raise ValueError("dist2 must be (M,)")
    t = _check_truncation(truncation)
    dist2 = dist2.detach().float().contiguous()
    M = int(dist2.shape[0])
    lib = _abi.lib()
    with torch.cuda.device(dist2.device):
        st = torch.cuda.current_stream(dist2.device).cuda_stream
        rgb = torch.empty((M, 3), dtype=torch.uint8, device=dist2.device)
        _abi.check(lib.sls_error_colors(M, dist2.data_ptr() if M else None, t, rgb.data_ptr() if M else None, st),
                   "sls_error_colors")
    return rgb


class MeshPseudoNormals:
    """What `mesh_pseudonormals` returns: the mesh as the native call reads it (`vertices` (V,3) float32, `faces` (F,3)
    int32, contiguous device tensors), the three tables of include/sls_signdist_math.h — `face_normals` (F,3) the unit
    normals, `edge_normals` (F,3,3) the sum of the unit normals of the faces sharing the edge of every corner,
    `vertex_normals` (V,3) the angle-weighted sum over the corners at every vertex, all float32 — and the device tensor
    `status` (8,) int32.  Valid for exactly these two tensors' contents: do not write to them."""
    __slots__ = ("vertices", "faces", "face_normals", "edge_normals", "vertex_normals", "status")

    def __init__(self, vertices, faces, face_normals, edge_normals, vertex_normals, status):
        self.vertices, self.faces, self.status = vertices, faces, status
        self.face_normals, self.edge_normals, self.vertex_normals = face_normals, edge_normals, vertex_normals


def _pseudonormals_enqueue(lib, vertices, faces, st) -> MeshPseudoNormals:
    """sls_mesh_pseudonormals without a host read; `status` (8,) int32 stays on the device."""
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if V < 1 or F < 1:
        raise ValueError("the mesh needs at least one vertex and one face")
    face_n = torch.empty((F, 3), dtype=torch.float32, device=dev)
    edge_n = torch.empty((F, 3, 3), dtype=torch.float32, device=dev)
    vertex_n = torch.empty((V, 3), dtype=torch.float32, device=dev)
    status = torch.empty((8,), dtype=torch.int32, device=dev)
    _, aligned, nbytes = scratch = _scratch(lib.sls_mesh_pseudonormals_scratch_bytes(V, F), dev)
    _abi.check(lib.sls_mesh_pseudonormals(V, vertices.data_ptr(), F, faces.data_ptr(), face_n.data_ptr(), edge_n.data_ptr(),
                                          vertex_n.data_ptr(), status.data_ptr(), aligned, nbytes, st), "sls_mesh_pseudonormals")
    del scratch
    return MeshPseudoNormals(vertices, faces, face_n, edge_n, vertex_n, status)


def _pseudonormals_status(words, what: str) -> dict:
    """The details of the eight status words; ValueError for the two kinds of face no distance is defined for."""
    w = [int(x) & 0xFFFFFFFF for x in words[:8]]
    if w[1]:
        raise ValueError(f"{what}: {w[1]} faces have a vertex index outside the vertices")
    if w[2]:
        raise ValueError(f"{what}: {w[2]} faces have a vertex with a non-finite coordinate")
    return {"degenerate_faces": w[0], "zero_area_faces": w[3], "boundary_edges": w[4], "nonmanifold_edges": w[5],
            "inconsistent_edges": w[6]}


def mesh_pseudonormals(vertices: torch.Tensor, faces: torch.Tensor, return_details: bool = False):
    """The pseudo-normal tables of a mesh for `signed_distance(pseudonormals=)`: built once (one native call,
    sls_mesh_pseudonormals: a thread per face, one stable sort of the corners by edge, the corner-by-vertex sort of
    `mesh_ops.vertex_normals`, float64 sums in ascending corner id — no float atomics, the same bytes on every run), used
    any number of times.  One host read (the status words).  With `return_details` also a dict of facts about the mesh,
    none of them an error: `degenerate_faces` (two equal indices), `zero_area_faces`, `boundary_edges` (one owner),
    `nonmanifold_edges` (three or more), `inconsistent_edges` (two owners that run the same way: a flipped face).
    Nothing is repaired: a mesh with flipped faces gets the sign its faces say.
    ValueError: a face with a vertex index outside the vertices or with a non-finite vertex; an empty mesh."""
    vertices, faces = _mesh(vertices, faces)
    lib = _abi.lib()
    dev = vertices.device
    with torch.cuda.device(dev):
        pn = _pseudonormals_enqueue(lib, vertices, faces, torch.cuda.current_stream(dev).cuda_stream)
        details = _pseudonormals_status(pn.status.cpu().tolist(), "mesh_pseudonormals")      # the one host read
    return (pn, details) if return_details else pn


def _use_pseudonormals(pn, vertices, faces) -> MeshPseudoNormals:
    if not isinstance(pn, MeshPseudoNormals):
        raise TypeError("pseudonormals must come from mesh_pseudonormals")
    if pn.vertices.shape != vertices.shape or pn.faces.shape != faces.shape or pn.vertices.device != vertices.device:
        raise ValueError("the pseudo-normals were built for another mesh")
    return pn


def _signed_enqueue(lib, pn: MeshPseudoNormals, points, want_face: bool, want_closest: bool, want_feature: bool, st):
    """sls_mesh_signed_distance without a host read: (sdist (M,), face (M,) | None, closest (M,3) | None, feature (M,) uint8
    | None, status (4,) int32, scratch) — the scratch serves a following sls_signed_stats."""
    dev = pn.vertices.device
    V, F, M = int(pn.vertices.shape[0]), int(pn.faces.shape[0]), int(points.shape[0])
    sdist = torch.empty((M,), dtype=torch.float32, device=dev)
    face = torch.empty((M,), dtype=torch.int32, device=dev) if want_face else None
    closest = torch.empty((M, 3), dtype=torch.float32, device=dev) if want_closest else None
    feature = torch.empty((M,), dtype=torch.uint8, device=dev) if want_feature else None
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    scratch = _scratch(lib.sls_mesh_signed_distance_scratch_bytes(V, F, M), dev)
    _abi.check(lib.sls_mesh_signed_distance(V, pn.vertices.data_ptr(), F, pn.faces.data_ptr(), pn.face_normals.data_ptr(),
                                            pn.edge_normals.data_ptr(), pn.vertex_normals.data_ptr(), M,
                                            points.data_ptr() if M else None, sdist.data_ptr() if M else None,
                                            face.data_ptr() if (want_face and M) else None,
                                            closest.data_ptr() if (want_closest and M) else None,
                                            feature.data_ptr() if (want_feature and M) else None, status.data_ptr(), scratch[1],
                                            scratch[2], st), "sls_mesh_signed_distance")
    return sdist, face, closest, feature, status, scratch


def signed_distance(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, return_face: bool = False,
                    return_closest: bool = False, return_feature: bool = False, pseudonormals: MeshPseudoNormals = None):
    """The exact SIGNED distance of every row of `points` (M,3) to the triangle mesh: `sdist` (M,) float32, whose magnitude is
    sqrt of `point_to_mesh`'s dist2, bit for bit, and which is negative iff the point lies BEHIND the mesh: behind the
    angle-weighted pseudo-normal (Baerentzen and Aanaes 2005) of the part of the nearest face the closest point lies on —
    the face, one of its edges, one of its vertices (include/sls_signdist_math.h).  With `return_face` also `face` (M,)
    int32 and with `return_closest` `closest` (M,3), both `point_to_mesh`'s; with `return_feature` `feature` (M,) uint8:
    0 the face, 1-3 its edge AB, BC, CA, 4-6 its vertex a, b, c.  Returned as `sdist` or a tuple in that order.

    Positive means the point lies on the side the faces look to (counter-clockwise vertices seen from there).  The sign
    is right for every closed, consistently oriented mesh and locally for an open oriented one, which the sign of the
    nearest face's own normal is not: around a thin wedge that is wrong for one query in eight.  A point on the surface,
    or on a feature whose faces cancel, gets the non-negative value.  `mesh_tsdf` and `mesh_poisson` emit oriented meshes
    whose faces look to the observed, free-space side.

    `pseudonormals=mesh_pseudonormals(vertices, faces)` uses tables built before; without it they are built by this call.
    One host read either way (the two status tensors are read together), no float atomics: the same input gives the same
    bits on every run.

    It is not an inside / outside test by ray parity and no occupancy query, nothing repairs the orientation (a flipped
    face gives the sign it says; `mesh_pseudonormals(return_details=True)` counts the evidence), it samples no volume,
    and it is not compared against Open3D's `compute_signed_distance`, which signs by ray counting and is undefined on
    the open meshes a LiDAR gives.  Device tensors only; the points must be finite.
    ValueError: a face with a vertex index outside the vertices or with a non-finite vertex; an empty mesh."""
    points = _cloud(points, "points")
    vertices, faces = _mesh(vertices, faces)
    if points.device != vertices.device:
        raise ValueError("the points and the mesh must live on the same device")
    lib = _abi.lib()
    dev = vertices.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        pn = _pseudonormals_enqueue(lib, vertices, faces, st) if pseudonormals is None else _use_pseudonormals(pseudonormals, vertices, faces)
        sdist, face, closest, feature, status, _ = _signed_enqueue(lib, pn, points, bool(return_face), bool(return_closest),
                                                                   bool(return_feature), st)
        w = torch.cat([pn.status, status]).cpu().tolist()                      # the one host read
    _pseudonormals_status(w[:8], "signed_distance")
    _mesh_distance_status(w[8:12], "signed_distance")
    res = (sdist,) + ((face,) if return_face else ()) + ((closest,) if return_closest else ()) + ((feature,) if return_feature else ())
    return res[0] if len(res) == 1 else res


def signed_error_colors(sdist: torch.Tensor, truncation: float) -> torch.Tensor:
    """(M,3) uint8 RGB of signed distances (M,) at `truncation` metres (include/sls_signdist_math.h): L = 255 for
    |sd| >= truncation, else int(|sd| / truncation * 256); positive (in front of the faces) (255, 255 - L, 255 - L), white
    to red; negative (behind them) (255 - L, 255 - L, 255), white to blue; a NaN gives black.  One native call
    (sls_signed_error_colors), no host read."""
    if not isinstance(sdist, torch.Tensor) or not sdist.is_cuda:
        raise RuntimeError("sdist must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    if sdist.dim() != 1:
        raise ValueError("sdist must be (M,)")
    t = _check_truncation(truncation)
    sdist = sdist.detach().float().contiguous()
    M = int(sdist.shape[0])
    lib = _abi.lib()
    with torch.cuda.device(sdist.device):
        st = torch.cuda.current_stream(sdist.device).cuda_stream
        rgb = torch.empty((M, 3), dtype=torch.uint8, device=sdist.device)
        _abi.check(lib.sls_signed_error_colors(M, sdist.data_ptr() if M else None, t, rgb.data_ptr() if M else None, st),
                   "sls_signed_error_colors")
    return rgb


class MeshRayIndex:
    """What `mesh_ray_index` returns: the mesh as the native call reads it (`vertices` (V,3) float32, `faces` (F,3) int32,
    contiguous device tensors) and the device buffer that holds the index of its triangles.  Valid for exactly these two
    tensors' contents: cast against it, do not write to them."""
    __slots__ = ("vertices", "faces", "buffer", "address", "nbytes", "status")

    def __init__(self, vertices, faces, buffer, address, nbytes, status):
        self.vertices, self.faces, self.buffer, self.address, self.nbytes, self.status = vertices, faces, buffer, address, nbytes, status


def _ray_index_enqueue(lib, vertices, faces, st) -> MeshRayIndex:
    """sls_mesh_rayindex_build without a host read; `status` (4,) int32 stays on the device."""
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if V < 1 or F < 1:
        raise ValueError("the mesh needs at least one vertex and one face")
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    buffer, address, nbytes = _scratch(lib.sls_mesh_rayindex_bytes(V, F), dev)
    _abi.check(lib.sls_mesh_rayindex_build(V, vertices.data_ptr(), F, faces.data_ptr(), address, nbytes, status.data_ptr(), st),
               "sls_mesh_rayindex_build")
    return MeshRayIndex(vertices, faces, buffer, address, nbytes, status)


def mesh_ray_index(vertices: torch.Tensor, faces: torch.Tensor) -> MeshRayIndex:
    """The index of a mesh's triangles for `cast_rays(index=)` and `render_mesh(index=)`: built once (one native call,
    sls_mesh_rayindex_build: the index `point_to_mesh` sweeps), cast against any number of times.  One host read (the
    status words).  ValueError: a face with a vertex index outside the vertices or with a non-finite vertex; an empty
    mesh."""
    vertices, faces = _mesh(vertices, faces)
    lib = _abi.lib()
    dev = vertices.device
    with torch.cuda.device(dev):
        index = _ray_index_enqueue(lib, vertices, faces, torch.cuda.current_stream(dev).cuda_stream)
        _mesh_distance_status(index.status.cpu().tolist(), "mesh_ray_index")    # the one host read
    return index


def _check_t_range(t_min, t_max):
    try:
        lo, hi = ctypes.c_float(float(t_min)).value, ctypes.c_float(float(t_max)).value   # what the native call will see
    except (TypeError, ValueError):
        raise ValueError("t_min and t_max must be numbers") from None
    if not lo >= 0.0:
        raise ValueError("t_min must not be negative or NaN")
    if not hi >= lo:
        raise ValueError("t_max must not be below t_min or NaN")
    return lo, hi


def _use_index(index, vertices, faces) -> MeshRayIndex:
    if not isinstance(index, MeshRayIndex):
        raise TypeError("index must come from mesh_ray_index")
    if index.vertices.shape != vertices.shape or index.faces.shape != faces.shape or index.vertices.device != vertices.device:
        raise ValueError("the index was built for another mesh")
    return index


def _cast_enqueue(lib, index: MeshRayIndex, origins, directions, t_min: float, t_max: float, want_face: bool, want_uv: bool, st):
    """sls_mesh_raycast without a host read: (t (M,), face (M,) | None, uv (M,2) | None, status (4,) int32)."""
    dev = index.vertices.device
    V, F, M = int(index.vertices.shape[0]), int(index.faces.shape[0]), int(origins.shape[0])
    t = torch.empty((M,), dtype=torch.float32, device=dev)
    face = torch.empty((M,), dtype=torch.int32, device=dev) if want_face else None
    uv = torch.empty((M, 2), dtype=torch.float32, device=dev) if want_uv else None
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    _abi.check(lib.sls_mesh_raycast(V, index.vertices.data_ptr(), F, index.faces.data_ptr(), index.address, index.nbytes, M,
                                    origins.data_ptr() if M else None, directions.data_ptr() if M else None, t_min, t_max,
                                    t.data_ptr() if M else None, face.data_ptr() if (want_face and M) else None,
                                    uv.data_ptr() if (want_uv and M) else None, status.data_ptr(), st), "sls_mesh_raycast")
    return t, face, uv, status


def cast_rays(origins: torch.Tensor, directions: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, t_min: float = 0.0,
              t_max: float = math.inf, return_face: bool = True, return_uv: bool = False, index: MeshRayIndex = None):
    """The first hit of every ray `origins[i] + t directions[i]` (both (M,3); a direction need not be unit) on the triangle
    mesh within `t_min <= t <= t_max`: `t` (M,) float32, +inf on a miss; with `return_face` (the default) also `face` (M,)
    int32, the lowest face index among hits of equal t bits, -1 on a miss; with `return_uv` also `uv` (M,2) float32, the
    barycentric weights of that face's second and third vertex.  Returned as `t`, `(t, face)`, `(t, uv)` or
    `(t, face, uv)`.  Both sides of a face hit.

    The values are the bits of include/sls_raycast_math.h compiled for the host for (ray, returned face): the watertight
    test of Woop, Benthin and Wald, under which no ray passes between two faces that share an edge or a vertex, and a
    ray exactly through one hits every face that shares it.  A ray with a non-finite component or a zero direction (the
    largest |component| below 2^-100) misses.  `index=mesh_ray_index(vertices, faces)` casts against an index built
    before; without it the index is built by this call.  One host read (the status words), no float atomics: the same
    input gives the same bits on every run.

    It is not a BVH: the faces are indexed in the curve order of their centroids, in runs of 32 whose boxes bound all
    three vertices, and 64 consecutive rays share one walk over the boxes — coherent rays (a range image) share most of
    what they visit, incoherent ones list many boxes per wave and are slow, though exact.  Rays are cast in the caller's
    order, not sorted.  t on a sliver is as good as float32 edge functions make it
    (DESIGN.md section 7).  Device tensors only.
    ValueError: a face with a vertex index outside the vertices or with a non-finite vertex; an empty mesh; a bad range."""
    origins, directions = _cloud(origins, "origins"), _cloud(directions, "directions")
    vertices, faces = _mesh(vertices, faces)
    if origins.shape != directions.shape:
        raise ValueError("origins and directions must have the same shape")
    if origins.device != vertices.device or directions.device != vertices.device:
        raise ValueError("the rays and the mesh must live on the same device")
    lo, hi = _check_t_range(t_min, t_max)
    lib = _abi.lib()
    dev = vertices.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        index = _ray_index_enqueue(lib, vertices, faces, st) if index is None else _use_index(index, vertices, faces)
        t, face, uv, status = _cast_enqueue(lib, index, origins, directions, lo, hi, bool(return_face), bool(return_uv), st)
        _mesh_distance_status(status.cpu().tolist(), "cast_rays")               # the one host read
    res = (t,) + ((face,) if return_face else ()) + ((uv,) if return_uv else ())
    return res[0] if len(res) == 1 else res


def _render_mesh_enqueue(lib, index: MeshRayIndex, col_half, row_half, cam_to_world, t_max: float, st):
    """The range image of the indexed mesh without a host read.  col_half (W,2) / row_half (H,2): the half-pixel ray tables
    (cos, sin of azimuth / elevation); cam_to_world: (4,4) float32 device tensor, sensor frame -> the mesh's frame.
    (range (H,W), face (H,W) int32, normal (3,H,W) in the sensor frame, status (4,) int32)."""
    W, H = int(col_half.shape[0]), int(row_half.shape[0])
    ce, se = row_half[:, 0:1], row_half[:, 1:2]
    rays = torch.stack([col_half[None, :, 0] * ce, col_half[None, :, 1] * ce, se.expand(H, W)], dim=-1).reshape(-1, 3)
    R = cam_to_world[:3, :3]
    directions = (rays @ R.T).contiguous()
    origins = cam_to_world[:3, 3].expand(H * W, 3).contiguous()
    t, face, _, status = _cast_enqueue(lib, index, origins, directions, 0.0, t_max, True, False, st)
    hit = face >= 0
    tri = index.vertices[index.faces[face.clamp(min=0).long()].long()]          # (HW, 3, 3)
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n = torch.nn.functional.normalize(n, dim=1)
    n = torch.where(((n * directions).sum(1, keepdim=True) > 0), -n, n)         # towards the sensor
    n = torch.where(hit[:, None], n @ R, torch.zeros_like(n))                   # R^T n: back to the sensor frame
    rng = torch.where(hit, t, torch.zeros_like(t))
    return rng.view(H, W), face.view(H, W), n.T.reshape(3, H, W).contiguous(), status


def render_mesh(vertices: torch.Tensor, faces: torch.Tensor, camera, t_max: float = math.inf, index: MeshRayIndex = None) -> dict:
    """What a spherical sensor at `camera` (a `scene.Camera`: world_view_transform, projection_matrix, image size) sees of
    the mesh: `{"range": (H,W) float32, "face": (H,W) int32, "normal": (3,H,W) float32}`.  The rays are the half-pixel rays
    of the surface sampler and of `renderer.pixel_rays` — pixel (c, r) looks along image coordinate (c - 0.5, r - 0.5) —
    built from `rasterizer.half_pixel_tables`, so `renderer.depth_to_points(camera, range[None])` puts every pixel back
    on the face it hit.  `range` is the distance along the unit ray (0 on a miss, as in `surf_depth`), `face` the face
    hit (-1), `normal` the unit geometric normal of that face in the SENSOR frame, turned towards the sensor (0).  One
    `cast_rays` over H W rays (`index=`: against an index built before); one host read (the status words)."""
    from .rasterizer import GaussianRasterizationSettings, get_camera, half_pixel_tables
    vertices, faces = _mesh(vertices, faces)
    _, hi = _check_t_range(0.0, t_max)
    lib = _abi.lib()
    dev = vertices.device
    H, W = int(camera.image_height), int(camera.image_width)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        ce = get_camera(GaussianRasterizationSettings(H, W, 1.0, camera.world_view_transform, camera.projection_matrix), dev)
        col_half, row_half = half_pixel_tables(ce, dev)
        cam_to_world = torch.linalg.inv_ex(camera.world_view_transform.detach().to(dev, torch.float32).T).inverse
        index = _ray_index_enqueue(lib, vertices, faces, st) if index is None else _use_index(index, vertices, faces)
        rng, face, normal, status = _render_mesh_enqueue(lib, index, col_half, row_half, cam_to_world, hi, st)
        _mesh_distance_status(status.cpu().tolist(), "render_mesh")             # the one host read
    return {"range": rng, "face": face, "normal": normal}


def _recon_metrics(reference, estimate, vertices, faces, exact: bool, error_map: bool, threshold, truncation_acc,
                   truncation_com, signed: bool = False):
    """evaluate_recon's metric block where the completeness is exact or the error map is wanted: cloud_metrics' calls with
    sls_mesh_distance (reference points against the mesh, then the unchanged sls_nn_stats) and, for the map, one more
    sls_nn_query (the mesh's vertices against the reference cloud) and two sls_error_colors.  One host read: the eight
    metric words and the four status words of sls_mesh_distance together.  With `signed` the reference points are measured
    once more with the sign (sls_mesh_pseudonormals, sls_mesh_signed_distance, sls_signed_stats: the unsigned calls and
    their bits stay as they are) and the four signed words and twelve more status words ride on that same read.
    (metrics, error map | None, signed block | None)"""
    Mr, Me = int(reference.shape[0]), int(estimate.shape[0])
    lib = _abi.lib()
    dev = reference.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        scratch = _scratch(lib.sls_nn_scratch_bytes(max(Mr, Me), max(Mr, Me)), dev)
        _, aligned, nbytes = scratch
        words = torch.empty((8,), dtype=torch.int64, device=dev)
        d_acc, _ = _query(lib, reference, estimate, False, scratch, st)
        _abi.check(lib.sls_nn_stats(Me, d_acc.data_ptr(), float(truncation_acc), float(threshold), 0, words.data_ptr(),
                                    aligned, nbytes, st), "sls_nn_stats")
        d_mesh, _, _, status, (_, m_aligned, m_nbytes) = _mesh_distance_enqueue(lib, reference, vertices, faces, False, False, st)
        if exact:
            _abi.check(lib.sls_nn_stats(Mr, d_mesh.data_ptr(), float(truncation_com), float(threshold), 1,
                                        words.data_ptr() + 32, m_aligned, m_nbytes, st), "sls_nn_stats")
        else:
            d_com, _ = _query(lib, estimate, reference, False, scratch, st)
            _abi.check(lib.sls_nn_stats(Mr, d_com.data_ptr(), float(truncation_com), float(threshold), 1,
                                        words.data_ptr() + 32, aligned, nbytes, st), "sls_nn_stats")
        emap = None
        if error_map:
            d_vert, _ = nearest(reference, vertices, return_index=False)
            emap = {"vertices": vertices, "vertex_dist2": d_vert, "vertex_colors": error_colors(d_vert, truncation_acc),
                    "points": reference, "point_dist2": d_mesh, "point_colors": error_colors(d_mesh, truncation_com)}
        read = [words, status.to(torch.int64)]
        if signed:
            t_com = _check_truncation(truncation_com)
            pn = _pseudonormals_enqueue(lib, vertices, faces, st)
            sdist, _, _, _, s_status, (_, s_aligned, s_nbytes) = _signed_enqueue(lib, pn, reference, False, False, False, st)
            s_words = torch.empty((4,), dtype=torch.int64, device=dev)
            _abi.check(lib.sls_signed_stats(Mr, sdist.data_ptr(), t_com, s_words.data_ptr(), s_aligned, s_nbytes, st),
                       "sls_signed_stats")
            if emap is not None:
                emap["point_signed"] = sdist
                emap["point_colors_signed"] = signed_error_colors(sdist, t_com)
            read += [s_words, pn.status.to(torch.int64), s_status.to(torch.int64)]
        w = torch.cat(read).cpu().tolist()                                     # the one host read
    _mesh_distance_status(w[8:12], "evaluate_recon")
    sblock = None
    if signed:
        details = _pseudonormals_status(w[16:24], "evaluate_recon")
        _mesh_distance_status(w[24:28], "evaluate_recon")
        n_s, behind = int(w[12]), int(w[13])
        total = struct.unpack("<d", struct.pack("<q", w[14]))[0]
        sblock = {"mean_m": total / n_s if n_s else math.nan, "share_behind": behind / n_s if n_s else math.nan, "n": n_s, **details}
    return _metrics(w[:8], threshold, truncation_acc, truncation_com), emap, sblock


ALIGN_MAX_POINTS = 200_000


def _align_vertices(reference: torch.Tensor, vertices: torch.Tensor, align) -> dict:
    """evaluate_recon's `align`: register_icp of a bounded subset of the vertices onto the reference cloud."""
    if not isinstance(align, dict) or "max_distance" not in align:
        raise ValueError("align must be a dict with at least max_distance (the arguments of register_icp)")
    args = dict(align)
    max_points = _check_k(args.pop("max_points", ALIGN_MAX_POINTS), "max_points", 1, 2**31 - 1)
    draw_seed = int(args.pop("seed", 0))
    if "return_details" in args:
        raise ValueError("align takes no return_details")
    source = vertices
    if vertices.shape[0] > max_points:
        g = torch.Generator(device=vertices.device)
        g.manual_seed(draw_seed)
        source = vertices[torch.randint(0, int(vertices.shape[0]), (max_points,), generator=g, device=vertices.device)]
    return register_icp(source, reference, **args)


def evaluate_recon(reference_points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, down_sample_res: float = 0.02,
                   threshold: float = 0.2, truncation_acc: float = 0.5, truncation_com: float = 0.5,
                   crop_to_reference: bool = False, mesh_sample_point: int = 10_000_000, seed: int = 0, align=None,
                   completeness: str = "sampled", error_map: bool = False, signed: bool = False) -> dict:
    """The reference's `evaluate_recon` (utils/eval_utils.py:67-154) for a reference cloud and an estimated mesh already
    on the device, with its dictionary keys and units: sample `mesh_sample_point` points from the mesh, voxel-down-sample
    both clouds at `down_sample_res` (skipped where that is <= 0, as in the reference), then the metric block of
    `cloud_metrics`.  Two host reads in all: the status words of the sampling and of both down-samples together, then the
    metric words.

    `crop_to_reference` defaults to False ON PURPOSE: the reference calls `estimate_mesh.crop(reference_bbox)` and
    discards what it returns (eval_utils.py:109; Open3D's crop does not work in place), so the numbers it publishes
    are those of the UNCROPPED mesh.  True does what it intended: only the faces whose vertices all lie inside the
    reference cloud's bounding box, padded by `down_sample_res` along z, are sampled (the box is computed on the device).
    The sampling is seeded (`seed`), where the reference's is not: a rerun gives the same numbers.

    `align` (default None: nothing of what follows happens, no extra call, no extra host read): a dict of `register_icp`
    arguments — `max_distance` is required; `iterations`, `method`, `init`, `target_normals` (of the reference cloud) and
    its `params` are optional — plus `max_points` (default 200 000) and `seed`.  The mesh's VERTICES are then registered
    onto the reference cloud before anything is sampled: on at most `max_points` of them, a seeded device draw with
    replacement where there are more; every vertex is moved by the pose found, and the metrics are those of the moved
    mesh.  The result gets one more key, "Alignment": what `register_icp` returns.  One more host read (its status
    words), and with the plane method and no normals the `estimate_normals` call on the reference cloud.

    `completeness` (default "sampled": nothing of what follows happens, the same calls, the same two host reads, the
    same bits): "exact" measures every reference point, after its voxel down-sampling, against the MESH ITSELF
    (`point_to_mesh`: sls_mesh_distance, then the unchanged sls_nn_stats) instead of against its nearest sample.  The
    sampled value depends on `seed` and on `mesh_sample_point` and is biased upwards by the sample spacing; the exact value
    depends on neither.  (A sample lies ON the surface, so with `down_sample_res <= 0` no exact distance exceeds its
    sampled one; voxel-averaged samples leave a curved surface a little, and there that holds for the means.)  The
    accuracy side stays sampled: it is points of the surface against a cloud.  With `crop_to_reference` the distance is
    to the faces the sampler keeps, selected with torch on the device: one more host synchronisation (the boolean
    index), none otherwise.  Still two host reads: the status words of sls_mesh_distance ride with the metric words.

    `error_map=True` adds the key "ErrorMap", a dict of device tensors: `vertices` (V,3) (moved, with `align`; all of
    them, also with `crop_to_reference`), `vertex_dist2` (V,) their squared distances to the evaluated reference cloud
    (`nearest`), `vertex_colors` (V,3) uint8 = `error_colors(vertex_dist2, truncation_acc)`; `points` (the evaluated
    reference points), `point_dist2` their EXACT squared distances to the mesh, whatever `completeness` is, and
    `point_colors` = `error_colors(point_dist2, truncation_com)`.  No further host read.

    `signed` (default False: nothing of what follows happens, the same calls, the same host reads, the same bits): True
    measures the evaluated reference points against the mesh with `signed_distance` as well, whatever `completeness`
    is, and adds the key "Signed": `mean_m`, the mean SIGNED distance over the points within `truncation_com` of the
    mesh; `share_behind`, the fraction of them with a negative distance; `n`, their number; and the details of
    `mesh_pseudonormals` (`degenerate_faces`, `zero_area_faces`, `boundary_edges`, `nonmanifold_edges`,
    `inconsistent_edges`).  With `error_map=True` "ErrorMap" also gets `point_signed` (the signed distances) and
    `point_colors_signed` = `signed_error_colors(point_signed, truncation_com)`.  No further host read: the new words
    ride on the second one.  The unsigned search is not replaced, so the search runs twice.
    What the sign means here: positive means the reference point lies on the side the faces look to.  For the output of
    `mesh_tsdf` / `mesh_poisson` that is the observed, free-space side, so a POSITIVE mean says the mesh sits BEHIND the
    true surface as the sensor saw it (a shrunk mesh), a negative one that it sits in front of it (an inflated one): bias
    where the unsigned numbers only show error."""
    if completeness not in ("sampled", "exact"):
        raise ValueError('completeness must be "sampled" or "exact"')
    if not isinstance(error_map, bool):
        raise ValueError("error_map must be True or False")
    if not isinstance(signed, bool):
        raise ValueError("signed must be True or False")
    reference = _cloud(reference_points, "reference_points")
    vertices, faces = _mesh(vertices, faces)
    if reference.device != vertices.device:
        raise ValueError("the reference cloud and the mesh must live on the same device")
    if reference.shape[0] == 0:
        raise ValueError("the reference cloud is empty")
    alignment = None
    if align is not None:
        alignment = _align_vertices(reference, vertices, align)
        vertices = transform_points(vertices, alignment["target_T_source"])
    n = int(mesh_sample_point)
    if n < 1:
        raise ValueError("mesh_sample_point must be at least 1")
    res = float(down_sample_res)
    down = res > 0.0
    if down:
        _check_voxel_size(res)
    lib = _abi.lib()
    dev = reference.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        box = None
        if crop_to_reference:
            pad = torch.tensor([0.0, 0.0, res], dtype=torch.float32, device=dev)
            box = torch.cat([reference.amin(0) - pad, reference.amax(0) + pad]).contiguous()
        estimate, _, status = _mesh_enqueue(lib, vertices, faces, n, seed, box, False, st)
        if down:
            estimate, _, status_e = _voxel_enqueue(lib, estimate, res, False, st)
            reference, _, status_r = _voxel_enqueue(lib, reference, res, False, st)
            status = torch.cat([status, status_e, status_r])
        w = status.cpu().tolist()                                           # host read 1 of 2
        _mesh_status(w[0:4], n)
        if down:
            estimate = estimate[:_voxel_status(w[4:8], "evaluate_recon: the sampled mesh")]
            reference = reference[:_voxel_status(w[8:12], "evaluate_recon: the reference cloud")]
    emap = sblock = None
    if completeness == "sampled" and not error_map and not signed:
        m = cloud_metrics(reference, estimate, threshold=threshold, truncation_acc=truncation_acc,
                          truncation_com=truncation_com)                    # host read 2 of 2
    else:
        if reference.shape[0] == 0 or estimate.shape[0] == 0:
            raise ValueError("both clouds need at least one point")
        kept = faces
        if box is not None:                                                 # the faces the sampler keeps (closed box)
            inside = ((vertices >= box[:3]) & (vertices <= box[3:])).all(1)
            kept = faces[inside[faces.long()].all(1)].contiguous()          # (a host synchronisation: the boolean index)
        m, emap, sblock = _recon_metrics(reference, estimate, vertices, kept, completeness == "exact", error_map, threshold,
                                         truncation_acc, truncation_com, signed)   # host read 2 of 2
    out = {
        "MAE_accuracy (cm)": m["accuracy_m"] * 100, "MAE_completeness (cm)": m["completeness_m"] * 100,
        "Chamfer_L1 (cm)": m["chamfer_l1_m"] * 100, "Precision [Accuracy] (%)": m["precision"] * 100.0,
        "Recall [Completeness] (%)": m["recall"] * 100.0, "F-score (%)": m["fscore"] * 100.0,
        "Inlier_threshold (m)": float(threshold), "Outlier_truncation_acc (m)": float(truncation_acc),
        "Outlier_truncation_com (m)": float(truncation_com),
    }
    if alignment is not None:
        out["Alignment"] = alignment
    if emap is not None:
        out["ErrorMap"] = emap
    if sblock is not None:
        out["Signed"] = sblock
    return out
