"""Spherical projection of a LiDAR scan to range / normal / valid images — the
CPU plumbing of scene/preprocessing.py:24-83 (BASELINE config 1).

The reference does this with `pyprojections` 0.0.3 (C++/pybind, PyPI sdist, not
installed and not vendored — "unpinned").  What the tree pins is the output
contract (`range_image (H,W) f32`, `normals_image (H,W,3)`, `valid (H,W) bool`,
`lut (H,W)` with -1 for empty pixels, the depth window `(depth_min, depth_max]`,
normals = -unit(point) by default, scene/preprocessing.py:42-64,112) and the
back-projection it must agree with: pixel (c, r) <-> (az, el) = K^-1 [c-0.5, r-0.5, 1]
(utils/graphic_utils.py:41-59).  This module defines K so that
`depth_to_points(project(cloud)) == cloud` for points at bin centres:

    fx = -W/hfov, cx = W*az_max/hfov - 1     (az decreases with the column index)
    fy = -H/vfov, cy = H*el_max/vfov - 1     (row 0 is the top beam)
    pixel index of image coordinate u:  floor(u + 1)   (centre of pixel c is u = c - 0.5)

NumPy only; nearest return wins (z-buffer on range).
"""
from __future__ import annotations

import math

import numpy as np


def calculate_spherical_intrinsics(cloud: np.ndarray, H: int, W: int, full_azimuth_threshold_deg: float = 300.0):
    """(K, vfov, hfov, az_max, el_max) for a (N,3) cloud.  A scan spanning more than
    `full_azimuth_threshold_deg` of azimuth is treated as a 360-degree sensor."""
    pts = np.asarray(cloud, dtype=np.float64)
    rng = np.linalg.norm(pts, axis=1)
    ok = rng > 0
    az = np.arctan2(pts[ok, 1], pts[ok, 0])
    el = np.arcsin(np.clip(pts[ok, 2] / rng[ok], -1.0, 1.0))
    el_min, el_max = float(el.min()), float(el.max())
    span = float(az.max() - az.min())
    if math.degrees(span) >= full_azimuth_threshold_deg:
        az_max, hfov = math.pi, 2.0 * math.pi
    else:
        pad = span / max(W - 1, 1) * 0.5
        az_max, hfov = float(az.max()) + pad, span + 2 * pad
    pad = (el_max - el_min) / max(H - 1, 1) * 0.5
    el_max, vfov = el_max + pad, (el_max - el_min) + 2 * pad
    fx, fy = -W / hfov, -H / vfov
    K = np.array([[fx, 0.0, W * az_max / hfov - 1.0], [0.0, fy, H * el_max / vfov - 1.0], [0.0, 0.0, 1.0]],
                 dtype=np.float32)
    return K, vfov, hfov, az_max, el_max


def project(cloud: np.ndarray, K: np.ndarray, H: int, W: int, depth_min: float, depth_max: float):
    """lut (H,W) int64: index of the nearest point falling into each pixel, -1 if none."""
    pts = np.asarray(cloud, dtype=np.float64)
    rng = np.linalg.norm(pts, axis=1)
    keep = (rng > depth_min) & (rng <= depth_max)
    az = np.arctan2(pts[:, 1], pts[:, 0])
    el = np.arcsin(np.clip(pts[:, 2] / np.maximum(rng, 1e-30), -1.0, 1.0))
    K = np.asarray(K, dtype=np.float64)
    u = K[0, 0] * az + K[0, 2]
    v = K[1, 1] * el + K[1, 2]
    c = np.floor(u + 1.0).astype(np.int64)
    r = np.floor(v + 1.0).astype(np.int64)
    hfov_px = abs(K[0, 0]) * 2.0 * math.pi
    if abs(hfov_px - W) <= 1.0:
        c = np.mod(c, W)                      # 360-degree image: az = +-pi are the same column
    keep &= (c >= 0) & (c < W) & (r >= 0) & (r < H)
    lut = np.full((H, W), -1, dtype=np.int64)
    idx = np.nonzero(keep)[0]
    order = idx[np.argsort(-rng[idx], kind="stable")]      # far first, so the nearest write lands last
    lut[r[order], c[order]] = order
    return lut


def scan_to_images(cloud: np.ndarray, H: int, W: int, depth_min: float = 0.5, depth_max: float = 100.0):
    """The image triple the reference's Preprocessor builds (scene/preprocessing.py:42-64):
    returns dict(K, range_image (H,W), normals_image (H,W,3), valid (H,W) bool, lut)."""
    cloud = np.asarray(cloud, dtype=np.float32)
    K, vfov, hfov, _, _ = calculate_spherical_intrinsics(cloud, H, W)
    lut = project(cloud, K, H, W, depth_min, depth_max)
    invalid = lut == -1
    ranges = np.linalg.norm(cloud, axis=1).astype(np.float32)
    range_image = ranges[lut]
    range_image[invalid] = 0.0
    normals = np.zeros_like(cloud, dtype=np.float32)
    ok = (ranges > depth_min) & (ranges <= depth_max)
    normals[ok] = -cloud[ok] / ranges[ok, None]                          # scene/preprocessing.py:112
    normals_image = normals[lut]
    normals_image[invalid] = 0.0
    return dict(K=K, vfov=vfov, hfov=hfov, range_image=range_image, normals_image=normals_image,
                valid=~invalid, lut=lut)


class DeviceProjector:
    """The same projection on the MI355X (csrc/sls_projector.hip through the C ABI): the scan never
    leaves the device, K is computed and consumed there, no host synchronisation.  One instance per
    image size; images are freshly allocated per scan (they become the keyframe's targets).

        proj = DeviceProjector(H, W, depth_min, depth_max)
        out = proj.scan_to_images(cloud_cuda)     # dict like scan_to_images(), device tensors; K (3,3) on device

    normals="radial" (the default) writes the reference's default normals, -unit(point).  normals="pca" is the
    reference's `preprocessing.enable_normal_estimation` (scene/preprocessing.py:85-118): the points inside the depth
    window (depth_min, depth_max] alone form a cloud, `evaluation.estimate_normals(radius=normal_radius,
    max_nn=normal_max_nn, viewpoint=origin)` gives them normals (a point with fewer than three neighbours within the
    radius keeps -unit(point)), and the normals image is gathered from those through `lut`; empty pixels stay 0.  lut,
    range_image and valid are the "radial" ones.  Selecting the in-window points is a boolean selection whose size the
    host must learn before the next launch can be sized, so "pca" costs ONE host synchronisation per scan and gives up
    the "no host synchronisation" property above; everything else stays on the device.

    ground=True is the reference's `preprocessing.enable_ground_segmentation` ("segment and assign up-facing normals to the
    ground", not implemented there): after the normals image of either option is made, `evaluation.segment_ground(cloud,
    sensor_height, **ground_params)` labels the WHOLE scan — every point gets a key, nothing is selected, so there is no
    host synchronisation — and every pixel whose lut point is ground takes its bin's plane normal (unit, nz >= 0).  The
    dict gains "ground", (H, W) bool.  lut, range_image and valid do not change.  The scan must be in the sensor frame,
    z up.  A Patchwork-style restatement, not Patchwork itself: see `evaluation.segment_ground`.
    """

    def __init__(self, H: int, W: int, depth_min: float = 0.5, depth_max: float = 100.0,
                 full_azimuth_threshold_deg: float = 300.0, device="cuda:0", normals: str = "radial",
                 normal_radius: float = 0.5, normal_max_nn: int = 50, ground: bool = False, sensor_height: float = 1.723,
                 ground_params=None):
        import torch
        from . import _abi, evaluation
        if normals not in ("radial", "pca"):
            raise ValueError('normals must be "radial" or "pca"')
        self.normals = normals
        if normals == "pca":                                    # checked before any work
            self.normal_radius, self.normal_max_nn, _ = evaluation._check_normals_args(normal_radius, normal_max_nn, (0.0, 0.0, 0.0))
        self.ground = bool(ground)
        if self.ground:                                         # likewise
            self._ground_prm = evaluation._check_ground_args(sensor_height, dict(ground_params or {}))
        self.H, self.W = int(H), int(W)
        self.depth_min, self.depth_max = float(depth_min), float(depth_max)
        self.thr = float(full_azimuth_threshold_deg)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("DeviceProjector runs on the GPU only (no CPU fallback); use scan_to_images() on the host")
        lib = _abi.lib()
        self._bytes = int(lib.sls_projector_scratch_bytes(self.H, self.W))
        self._scratch = torch.empty((self._bytes + 7) // 8, dtype=torch.int64, device=self.dev)
        _abi.check(lib.sls_projector_prepare(self.H, self.W, self._scratch.data_ptr(), self._bytes, self._stream()),
                   "sls_projector_prepare")

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _cloud(self, cloud):
        import torch
        if not (isinstance(cloud, torch.Tensor) and cloud.is_cuda):
            raise RuntimeError("cloud must be a CUDA tensor (no CPU fallback)")
        if cloud.dtype != torch.float32 or cloud.dim() != 2 or cloud.shape[1] != 3:
            raise RuntimeError("cloud must be (N,3) float32")
        return cloud.contiguous()

    def intrinsics(self, cloud):
        """12 device floats: K row-major, vfov, hfov, any-point flag (calculate_spherical_intrinsics)."""
        import torch
        from . import _abi
        cloud = self._cloud(cloud)
        out = torch.empty(12, dtype=torch.float32, device=self.dev)
        _abi.check(_abi.lib().sls_projector_intrinsics(cloud.shape[0], cloud.data_ptr(), self.H, self.W, self.thr,
                                                       out.data_ptr(), self._scratch.data_ptr(), self._bytes,
                                                       self._stream()), "sls_projector_intrinsics")
        return out

    def project(self, cloud, K):
        """(lut int32 (H,W), range_image (H,W), normals_image (H,W,3), valid bool (H,W)) for K: 9+ device floats."""
        import torch
        from . import _abi
        cloud = self._cloud(cloud)
        if not (isinstance(K, torch.Tensor) and K.is_cuda and K.dtype == torch.float32 and K.numel() >= 9):
            raise RuntimeError("K must be a CUDA float32 tensor with the 9 row-major entries first")
        K = K.contiguous()
        H, W = self.H, self.W
        lut = torch.empty((H, W), dtype=torch.int32, device=self.dev)
        rng = torch.empty((H, W), dtype=torch.float32, device=self.dev)
        nrm = torch.empty((H, W, 3), dtype=torch.float32, device=self.dev)
        valid = torch.empty((H, W), dtype=torch.uint8, device=self.dev)
        _abi.check(_abi.lib().sls_projector_project(cloud.shape[0], cloud.data_ptr(), K.data_ptr(), H, W, self.depth_min,
                                                    self.depth_max, lut.data_ptr(), rng.data_ptr(), nrm.data_ptr(),
                                                    valid.data_ptr(), self._scratch.data_ptr(), self._bytes,
                                                    self._stream()), "sls_projector_project")
        return lut, rng, nrm, valid.view(torch.bool)

    def pca_normals_image(self, cloud, lut, valid):
        """normals_image (H,W,3) of normals="pca" for a projected scan: estimate_normals over the in-window points,
        scattered back to the scan's rows and gathered through lut; 0 at empty pixels.  One host synchronisation."""
        import torch
        from . import evaluation
        cloud = self._cloud(cloud)
        x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
        rng = (x * x + y * y + z * z).sqrt()                    # float32, the projection kernel's own expression
        lo, hi = torch.tensor([self.depth_min, self.depth_max], dtype=torch.float32, device=cloud.device)
        inside = (rng > lo) & (rng <= hi)                       # (float32 against float32, as there)
        rows = torch.nonzero(inside).squeeze(1)                 # the host synchronisation: the selection's size
        radius = None if math.isinf(self.normal_radius) else self.normal_radius
        est = evaluation.estimate_normals(cloud[rows], radius, self.normal_max_nn, (0.0, 0.0, 0.0))
        per_point = torch.zeros_like(cloud)
        per_point[rows] = est
        image = per_point[lut.long().clamp_(min=0).view(-1)].view(self.H, self.W, 3)
        return torch.where(valid.unsqueeze(-1), image, torch.zeros_like(image))

    def ground_image(self, cloud, lut, valid, normals_image):
        """(normals_image with the bin's plane normal at every pixel whose lut point is ground, ground (H,W) bool) of
        ground=True for a projected scan.  No host synchronisation."""
        import torch
        from . import evaluation
        cloud = self._cloud(cloud)
        label, bins, planes, _, _ = evaluation._ground_enqueue(cloud, self._ground_prm, False)
        rows = lut.long().clamp_(min=0).view(-1)
        ground = (label.view(torch.bool)[rows].view(self.H, self.W) & valid) if cloud.shape[0] else torch.zeros_like(valid)
        if not cloud.shape[0]:
            return normals_image, ground
        plane = planes[:, :3].to(torch.float32)[bins.long().clamp_(min=0)[rows]].view(self.H, self.W, 3)
        return torch.where(ground.unsqueeze(-1), plane, normals_image), ground

    def scan_to_images(self, cloud):
        intr = self.intrinsics(cloud)
        lut, rng, nrm, valid = self.project(cloud, intr)
        if self.normals == "pca":
            nrm = self.pca_normals_image(cloud, lut, valid)
        out = dict(K=intr[:9].view(3, 3), vfov=intr[9], hfov=intr[10], range_image=rng, normals_image=nrm,
                   valid=valid, lut=lut)
        if self.ground:
            out["normals_image"], out["ground"] = self.ground_image(cloud, lut, valid, nrm)
        return out
