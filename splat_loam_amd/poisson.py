"""Screened Poisson surface reconstruction on the device, over the sparse block volume of `tsdf.py`: from an oriented cloud
to a closed triangle mesh.

The samples are splatted into a vector field and a density on the blocks (sls_poisson_splat), the least-squares system over
the edges of the band is solved by Jacobi-preconditioned conjugate gradients (sls_poisson_solve), the zero surface of the
solution leaves through the TSDF volume's marching tetrahedra (sls_tsdf_extract_count / _emit, unchanged) and is trimmed by
the smoothed sample density (sls_poisson_density).  include/sls_poisson_math.h states every rule and every order of
summation, DESIGN.md section 2 ("Poisson volume") the contract, tests/poisson_ref.py restates it in NumPy.

What it IS: a uniform-resolution band around the samples, trilinear splats, natural boundary conditions at the band's edge,
bit-reproducible.  What it is NOT: Kazhdan's adaptive octree, B-spline splats, a Dirichlet envelope; it is not compared
against Open3D's `create_from_point_cloud_poisson`, which is not a dependency, and no parity with it is claimed.

Device tensors only; there is no CPU path.  Host reads: `splat` none (one with `details=True`), `solve` one (the status
words), `density` none, `extract` one (the number of triangles).

`screening`, `tol`, `iterations`, `margin` and `density_sweeps` are JUDGEMENTS, not taken from any reference.  What was
observed: screening 4 closed the capped test sphere (0.1 m voxels) where screening 1 left stray components at the band's
edge; a margin of 3 voxels kept that sphere's and the test plane's surface inside the band; at tol = 1e-4 the solve takes
about a hundred passes on every case measured.  None of them was tuned beyond that; two sweeps give the density a reach of
three voxels, and a hole wider than that needs more (tests/test_poisson.py uses three for a 0.6 m hole at 0.1 m).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _abi, tsdf
from .tsdf import BLOCK_VOXELS, _device_points, _stream

FLAG_CONVERGED, FLAG_NOT_PD, FLAG_EMPTY = 1, 2, 4
STATUS_WORDS = 8                     # SLS_POISSON_STATUS_WORDS
MAX_ITERATIONS = 1000                # SLS_POISSON_MAX_ITERATIONS
DEFAULT_MARGIN_VOXELS = 3.0          # a judgement (see the module's docstring)


def _scratch(nbytes, dev):
    buf = torch.empty((int(nbytes) + 256,), dtype=torch.uint8, device=dev)
    return buf, (buf.data_ptr() + 255) & ~255


class PoissonVolume:
    """`blocks` (B,3) int32 device tensor in ascending key order (what `tsdf.allocate_blocks` returns), voxels of edge
    `voxel_size`, `origin` of block (0,0,0).  `.field` (B,512,4) float32: (Vx, Vy, Vz, W) per voxel, voxel l = x | y << 3 |
    z << 6 of block k at [k, l]; `.chi` (B,512) float32 after `solve`: negative inside."""

    def __init__(self, blocks: torch.Tensor, voxel_size: float, origin=(0.0, 0.0, 0.0)):
        if not isinstance(blocks, torch.Tensor) or not blocks.is_cuda:
            raise RuntimeError("blocks must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
        if blocks.dim() != 2 or blocks.shape[1] != 3 or blocks.dtype != torch.int32:
            raise ValueError("blocks must be (B,3) int32")
        self.voxel_size = float(voxel_size)
        self.origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
        if not (self.voxel_size > 0 and np.isfinite(self.voxel_size) and np.isfinite(self.origin).all()):
            raise ValueError("voxel_size must be a finite number > 0 and origin finite")
        self.blocks = blocks.detach().contiguous()
        B = int(self.blocks.shape[0])
        self.field = torch.zeros((B, BLOCK_VOXELS, 4), dtype=torch.float32, device=blocks.device)
        self.chi = None
        self.status = None

    @property
    def nbytes(self) -> int:
        return int(self.blocks.shape[0]) * BLOCK_VOXELS * 20

    @torch.no_grad()
    def splat(self, points: torch.Tensor, normals: torch.Tensor, details: bool = False):
        """Replaces `.field` by the splat of the (M,3) device points with their (M,3) normals.  Nothing is read back;
        `details=True` reads the status words and returns dict(n_nonfinite, n_out_of_range, n_dropped: points with at
        least one corner in no block)."""
        points, normals = _device_points(points, "points"), _device_points(normals, "normals")
        if points.shape != normals.shape or points.device != self.blocks.device:
            raise ValueError("points and normals must be (M,3) each, on the volume's device")
        lib = _abi.lib()
        dev = self.blocks.device
        M, B = int(points.shape[0]), int(self.blocks.shape[0])
        with torch.cuda.device(dev):
            status = torch.empty((4,), dtype=torch.int32, device=dev)
            nbytes = int(lib.sls_poisson_splat_scratch_bytes(M, B))
            buf, ptr = _scratch(nbytes, dev)
            if M == 0:
                self.field.zero_()
            _abi.check(lib.sls_poisson_splat(M, points.data_ptr(), normals.data_ptr(), B, self.blocks.data_ptr(), self.voxel_size,
                                             self.origin.ctypes.data, self.field.data_ptr(), status.data_ptr(), ptr, nbytes,
                                             _stream(dev)), "sls_poisson_splat")
            self.chi = None
            if details:
                w = status.cpu().numpy().view(np.uint32)
                return {"n_nonfinite": int(w[0]), "n_out_of_range": int(w[1]), "n_dropped": int(w[2])}
        return None

    @torch.no_grad()
    def solve(self, screening: float = 4.0, iterations: int = 300, tol: float = 1e-4):
        """Solves for `.chi` from `.field`: at most `iterations` passes of preconditioned conjugate gradients, ended when
        the residual's norm falls to `tol` times the right side's.  Returns dict(iterations, converged, residual: that
        ratio, iso, flags); ONE host read, after everything is enqueued.  The defaults are a judgement."""
        lib = _abi.lib()
        dev = self.blocks.device
        B = int(self.blocks.shape[0])
        with torch.cuda.device(dev):
            chi = torch.empty((B, BLOCK_VOXELS), dtype=torch.float32, device=dev)
            status = torch.empty((STATUS_WORDS,), dtype=torch.int64, device=dev)
            nbytes = int(lib.sls_poisson_solve_scratch_bytes(B))
            buf, ptr = _scratch(nbytes, dev)
            _abi.check(lib.sls_poisson_solve(B, self.blocks.data_ptr(), self.field.data_ptr(), float(screening), int(iterations),
                                             float(tol), chi.data_ptr(), status.data_ptr(), ptr, nbytes, _stream(dev)),
                       "sls_poisson_solve")
            self.status = status
            words = status.cpu().numpy().view(np.uint64)                # the one host read
        self.chi = chi
        rr, bb, iso = (float(v) for v in words[3:6].view(np.float64))
        flags = int(words[1])
        return {"iterations": int(words[0]), "converged": bool(flags & FLAG_CONVERGED), "residual": float(np.sqrt(rr / bb)) if bb > 0 else 0.0,
                "iso": iso, "flags": flags}

    @torch.no_grad()
    def density(self, sweeps: int = 2) -> torch.Tensor:
        """(B,512) float32: the splat weight W after `sweeps` averaging sweeps over the present neighbours.  Nothing read
        back.  The default is a judgement."""
        lib = _abi.lib()
        dev = self.blocks.device
        B = int(self.blocks.shape[0])
        with torch.cuda.device(dev):
            out = torch.empty((B, BLOCK_VOXELS), dtype=torch.float32, device=dev)
            nbytes = int(lib.sls_poisson_density_scratch_bytes(B))
            buf, ptr = _scratch(nbytes, dev)
            _abi.check(lib.sls_poisson_density(B, self.blocks.data_ptr(), self.field.data_ptr(), int(sweeps), out.data_ptr(), ptr,
                                               nbytes, _stream(dev)), "sls_poisson_density")
        return out

    @torch.no_grad()
    def extract(self, min_density=None, density_sweeps: int = 2, weld: bool = False, details: bool = False):
        """The zero surface of `.chi` through `tsdf.extract_surface`, the TSDF volume's extraction: `(vertices (3T,3), faces (T,3))`, a
        triangle soup in its fixed order, normals towards free space when the samples' normals point there.
        `min_density=t` keeps only the cubes all of whose corners have a smoothed density (`density(density_sweeps)`) of at
        least t: the surface the solution extrapolates beyond the samples' rim goes.  None: every cube of the band.  One
        host read (T).  `details=True` adds dict(counts, density)."""
        if self.chi is None:
            raise RuntimeError("extract needs a solution: call solve() first")
        if min_density is None:
            weight, threshold = torch.ones_like(self.chi), 1.0
        else:
            weight, threshold = self.density(density_sweeps), float(min_density)
        out = tsdf.extract_surface(self.blocks, self.chi, weight, self.voxel_size, self.origin, threshold, weld, details)
        if details:
            out[2]["density"] = None if min_density is None else weight
        return out


@torch.no_grad()
def reconstruct(points: torch.Tensor, normals: torch.Tensor, voxel_size: float, margin: float = None, *, screening: float = 4.0,
                iterations: int = 300, tol: float = 1e-4, min_density=None, density_sweeps: int = 2, origin=(0.0, 0.0, 0.0),
                weld: bool = False, details: bool = False):
    """An oriented cloud to a triangle soup: blocks allocated `margin` (default 3 voxels; a judgement; the allocator's limit
    is margin + voxel_size <= 8 voxel_size) around the points with `tsdf.allocate_blocks(points, voxel_size, trunc=margin)`,
    then `PoissonVolume.splat`, `.solve`, `.extract`.  Returns `(vertices, faces)`; `details=True` adds dict(blocks, solve:
    what `solve` returned, splat: the splat's counts, volume: the PoissonVolume).  Host reads: one for the blocks, one for
    the solve, one for the triangles (and one for the splat's counts with `details=True`)."""
    voxel_size = float(voxel_size)
    margin = DEFAULT_MARGIN_VOXELS * voxel_size if margin is None else float(margin)
    blocks = tsdf.allocate_blocks(points, voxel_size, margin, origin)
    vol = PoissonVolume(blocks, voxel_size, origin)
    splat = vol.splat(points, normals, details=details)
    solved = vol.solve(screening=screening, iterations=iterations, tol=tol)
    out = vol.extract(min_density=min_density, density_sweeps=density_sweeps, weld=weld, details=details)
    if details:
        det = out[2]
        det.update({"blocks": int(blocks.shape[0]), "solve": solved, "splat": splat, "volume": vol})
        return out[0], out[1], det
    return out
