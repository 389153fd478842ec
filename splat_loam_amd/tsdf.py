"""A sparse truncated signed distance volume on the device: from rendered keyframes to a triangle mesh.

The mesher of the 2DGS lineage, restated for the spherical camera: the rendered depth of every keyframe is fused into a
volume of 8x8x8-voxel blocks (sls_tsdf_integrate), allocated around a point set (sls_tsdf_blocks: the surface samples
`meshing.sample_surface` produces are the intended source), and the zero surface leaves as a triangle soup by marching
tetrahedra (sls_tsdf_extract_count / _emit).  include/sls_tsdf_math.h states every rule, DESIGN.md section 2
("TSDF volume") the contract, tests/tsdf_ref.py restates it in NumPy.  Device tensors only; there is no CPU path.

Host reads: `allocate_blocks` one (the status words, for B), `TsdfVolume.integrate` none, `TsdfVolume.extract` one (T).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi

BLOCK_VOXELS = 512
MAX_BLOCKS = 1 << 19                 # SLS_TSDF_MAX_BLOCKS


def _grid(voxel_size, trunc, origin):
    voxel_size, trunc = float(voxel_size), float(trunc)
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    return voxel_size, trunc, origin


def _device_points(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    t = t.detach()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be (M,3)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@torch.no_grad()
def allocate_blocks(points: torch.Tensor, voxel_size: float, trunc: float, origin=(0.0, 0.0, 0.0), details: bool = False):
    """The blocks the (M,3) device points name: every block the box [p - m, p + m] touches, m = trunc + voxel_size,
    as a (B,3) int32 device tensor in ascending key order — the same array for the same cloud on every run.  Points with
    a non-finite coordinate, or farther than 2^20 blocks from the origin, name nothing; `details=True` adds
    dict(n_nonfinite, n_out_of_range).  One host read (the status words)."""
    points = _device_points(points, "points")
    voxel_size, trunc, origin = _grid(voxel_size, trunc, origin)
    lib = _abi.lib()
    dev = points.device
    M = int(points.shape[0])
    with torch.cuda.device(dev):
        capacity = min(27 * M, MAX_BLOCKS)
        out = torch.empty((capacity, 3), dtype=torch.int32, device=dev)
        status = torch.empty((4,), dtype=torch.int32, device=dev)
        nbytes = int(lib.sls_tsdf_blocks_scratch_bytes(M))
        scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=dev)
        _abi.check(lib.sls_tsdf_blocks(M, points.data_ptr(), voxel_size, trunc, origin.ctypes.data, capacity, out.data_ptr(),
                                       status.data_ptr(), (scratch.data_ptr() + 255) & ~255, nbytes, _stream(dev)), "sls_tsdf_blocks")
        words = status.cpu().numpy().view(np.uint32)                # the one host read
    B = int(words[0])
    if B > capacity:
        raise RuntimeError(f"the points name {B} blocks, more than a volume holds ({MAX_BLOCKS}): use a larger voxel_size")
    blocks = out[:B].clone()
    if details:
        return blocks, {"n_nonfinite": int(words[1]), "n_out_of_range": int(words[2])}
    return blocks


def weld_soup(vertices: torch.Tensor):
    """A triangle soup (3T,3) with its bit-equal vertices merged: `(vertices (V,3) float32, faces (T,3) int32)`.  Rows are
    compared as integers (-0.0 and 0.0 stay apart); plumbing, `torch.unique`, not on the hot path."""
    if vertices.shape[0] == 0:
        return vertices, torch.zeros((0, 3), dtype=torch.int32, device=vertices.device)
    uniq, inverse = torch.unique(vertices.contiguous().view(torch.int32), dim=0, return_inverse=True)
    return uniq.view(torch.float32), inverse.to(torch.int32).view(-1, 3)


def compose_volume_to_view(world_T_model, view32) -> np.ndarray:
    """inv(world_T_model) followed by the keyframe's view, as 12 float32 (3x4 row-major): composed in float64 from the
    float32 view matrix the rasterizer renders with (model frame -> view frame), rounded once — the other direction of
    `meshing.compose_cam_to_world`."""
    from .meshing import _pose44
    view = np.asarray(view32, dtype=np.float32).astype(np.float64).reshape(4, 4)
    return np.ascontiguousarray((view @ np.linalg.inv(_pose44(world_T_model)))[:3].reshape(12), dtype=np.float32)


class TsdfVolume:
    """`blocks` (B,3) int32 device tensor in ascending key order (what `allocate_blocks` returns), voxels of edge
    `voxel_size`, truncation `trunc` (`trunc + voxel_size <= 8 voxel_size`), `origin` of block (0,0,0) in the volume's
    (world) frame.  `.tsdf` / `.weight`: (B,512) float32, voxel l = x | y << 3 | z << 6 of block k at [k, l]; a new volume
    holds tsdf = 1 (free space) and weight = 0 (unobserved)."""

    def __init__(self, blocks: torch.Tensor, voxel_size: float, trunc: float, origin=(0.0, 0.0, 0.0)):
        if not isinstance(blocks, torch.Tensor) or not blocks.is_cuda:
            raise RuntimeError("blocks must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
        if blocks.dim() != 2 or blocks.shape[1] != 3 or blocks.dtype != torch.int32:
            raise ValueError("blocks must be (B,3) int32")
        self.voxel_size, self.trunc, self.origin = _grid(voxel_size, trunc, origin)
        if not (self.voxel_size > 0 and self.trunc > 0 and self.trunc + self.voxel_size <= 8 * self.voxel_size):
            raise ValueError("voxel_size and trunc must be > 0 with trunc + voxel_size <= 8 voxel_size")
        self.blocks = blocks.detach().contiguous()
        B = int(self.blocks.shape[0])
        self.tsdf = torch.ones((B, BLOCK_VOXELS), dtype=torch.float32, device=blocks.device)
        self.weight = torch.zeros((B, BLOCK_VOXELS), dtype=torch.float32, device=blocks.device)

    @property
    def nbytes(self) -> int:
        return int(self.blocks.shape[0]) * BLOCK_VOXELS * 8

    @torch.no_grad()
    def integrate(self, allmap: torch.Tensor, camera, world_T_model, min_opacity: float = 0.5, max_depth_dist: float = 0.1,
                  depth_ratio: float = 0.0) -> None:
        """Fuses one rendered keyframe: `allmap` the rasterizer forward's full (7,H,W) device tensor
        (`lean_allmap=False`), `camera` the `scene.Camera` it was rendered with, `world_T_model` 4x4 (or 3x4) on the host:
        the pose of the rendered model in the volume's frame.  One launch, nothing read back."""
        from .meshing import _host
        from .rasterizer import GaussianRasterizationSettings, get_camera
        if not isinstance(allmap, torch.Tensor) or not allmap.is_cuda:
            raise RuntimeError("integrate needs the allmap on a ROCm device; there is no CPU fallback")
        if allmap.dim() != 3 or allmap.shape[0] != 7:
            raise ValueError("allmap must be (7, H, W)")
        if allmap.device != self.blocks.device:
            raise ValueError("allmap and the volume must live on the same device")
        am = allmap.detach()
        if am.dtype != torch.float32 or not am.is_contiguous():
            am = am.float().contiguous()
        _, H, W = am.shape
        dev = am.device
        ce = get_camera(GaussianRasterizationSettings(H, W, 1.0, camera.world_view_transform, camera.projection_matrix), dev)
        cam = _abi.SlsCamera()
        C.memmove(C.byref(cam), C.byref(ce.cam), C.sizeof(cam))
        view = np.eye(4, dtype=np.float32)
        view[:3, :3] = np.asarray(ce.cam.Rvw, dtype=np.float32).reshape(3, 3)
        view[:3, 3] = np.asarray(ce.cam.tvw, dtype=np.float32)
        m = compose_volume_to_view(_host(world_T_model), view).reshape(3, 4)
        for i in range(3):
            for j in range(3):
                cam.Rvw[3 * i + j] = float(m[i, j])
            cam.tvw[i] = float(m[i, 3])
        with torch.cuda.device(dev):
            _abi.check(_abi.lib().sls_tsdf_integrate(C.byref(cam), int(self.blocks.shape[0]), self.blocks.data_ptr(),
                                                     self.tsdf.data_ptr(), self.weight.data_ptr(), am.data_ptr(), self.voxel_size,
                                                     self.trunc, self.origin.ctypes.data, float(min_opacity), float(max_depth_dist),
                                                     float(depth_ratio), _stream(dev)), "sls_tsdf_integrate")

    @torch.no_grad()
    def extract(self, min_weight: float = 1.0, weld: bool = False, details: bool = False):
        """The zero surface: `(vertices (3T,3) float32, faces (T,3) int32)`, a triangle soup in the fixed order ascending
        block, cube, tetrahedron, triangle, normals towards free space; only cubes all of whose eight corners have
        `weight >= min_weight`.  `weld=True` merges bit-equal vertices (`torch.unique`; the surface is watertight by
        construction, so shared vertices are bit-equal).  One host read (T).  `details=True` adds dict(counts: the
        triangles per block, a device tensor)."""
        return extract_surface(self.blocks, self.tsdf, self.weight, self.voxel_size, self.origin, min_weight, weld, details)


@torch.no_grad()
def extract_surface(blocks: torch.Tensor, values: torch.Tensor, weight: torch.Tensor, voxel_size: float, origin, min_weight: float = 1.0,
                    weld: bool = False, details: bool = False):
    """Marching tetrahedra over any `(B,512)` float32 value / weight arrays on the blocks (sls_tsdf_extract_count / _emit): what
    `TsdfVolume.extract` returns for its tsdf and `poisson.PoissonVolume.extract` for its chi.  `origin`: three float64 on
    the host."""
    lib = _abi.lib()
    dev = blocks.device
    B = int(blocks.shape[0])
    with torch.cuda.device(dev):
        st = _stream(dev)
        counts = torch.empty((max(B, 1),), dtype=torch.int32, device=dev)
        prefix = torch.empty((max(B, 1),), dtype=torch.int32, device=dev)
        status = torch.empty((4,), dtype=torch.int32, device=dev)
        _abi.check(lib.sls_tsdf_extract_count(B, blocks.data_ptr(), values.data_ptr(), weight.data_ptr(), float(min_weight),
                                              counts.data_ptr(), prefix.data_ptr(), status.data_ptr(), st), "sls_tsdf_extract_count")
        T = int(status.cpu().numpy().view(np.uint32)[0])            # the one host read
        tri = torch.empty((T, 3, 3), dtype=torch.float32, device=dev)
        _abi.check(lib.sls_tsdf_extract_emit(B, blocks.data_ptr(), values.data_ptr(), weight.data_ptr(), float(min_weight),
                                             float(voxel_size), origin.ctypes.data, prefix.data_ptr(), T, tri.data_ptr(), st),
                   "sls_tsdf_extract_emit")
    vertices = tri.view(-1, 3)
    faces = torch.arange(3 * T, dtype=torch.int32, device=dev).view(T, 3)
    if weld:
        vertices, faces = weld_soup(vertices)
    if details:
        return vertices, faces, {"counts": counts[:B]}
    return vertices, faces
