"""Host side of the TSDF volume (sls_tsdf_blocks, sls_tsdf_integrate, sls_tsdf_extract_count / _emit,
splat_loam_amd/tsdf.py): the scratch size, every argument error (all checked before a launch: no device needed), the mesh
PLY writer against the reader, and the refusal of CPU tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from splat_loam_amd import _abi, meshing, ply_io, tsdf

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
ORIGIN = (C.c_double * 3)(0.0, 0.0, 0.0)
BAD_GRIDS = ((0.0, 0.4), (-0.1, 0.4), (float("nan"), 0.4), (float("inf"), 0.4), (0.1, 0.0), (0.1, -0.4), (0.1, float("nan")),
             (0.1, float("inf")), (0.1, 0.7001))             # the last: trunc + voxel_size > 8 voxel_size


def _camera(H=16, W=64):
    cam = _abi.SlsCamera()
    cam.H, cam.W, cam.wrap = H, W, 1
    cam.fx, cam.fy, cam.cx, cam.cy = -W / (2 * np.pi), -H / 1.0, W / 2, H / 2
    cam.near_cut = 0.2
    cam.Rvw[0] = cam.Rvw[4] = cam.Rvw[8] = 1.0
    return cam


def test_scratch_bytes():
    lib = _abi.lib()
    assert lib.sls_tsdf_blocks_scratch_bytes(0) == 0 and lib.sls_tsdf_blocks_scratch_bytes(-3) == 0
    assert lib.sls_tsdf_blocks_scratch_bytes((1 << 26) + 1) == 0
    last = 0
    for M in (1, 2, 255, 256, 257, 3000, 40_000, 1_000_000):
        n = lib.sls_tsdf_blocks_scratch_bytes(M)
        assert n % 256 == 0 and n >= last, M
        assert n >= lib.sls_sort_scratch_bytes(27 * M) + 24 * 27 * M        # the sorter over 27 keys per point + two key and two index arrays
        last = n


def test_blocks_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_tsdf_blocks_scratch_bytes(100)

    def call(M=100, p=FAKE, vs=0.1, tr=0.4, o=ORIGIN, cap=800, out=FAKE, status=FAKE, s=FAKE, n=need):
        return lib.sls_tsdf_blocks(M, p, vs, tr, o, cap, out, status, s, n, None)
    assert call(M=-1) == E_ARG and b"M negative" in lib.sls_last_error()
    assert call(M=(1 << 26) + 1) == E_ARG
    assert call(cap=-1) == E_ARG and b"capacity" in lib.sls_last_error()
    for vs, tr in BAD_GRIDS:
        assert call(vs=vs, tr=tr) == E_ARG and b"voxel_size" in lib.sls_last_error(), (vs, tr)
        assert call(M=0, vs=vs, tr=tr, status=None) == E_ARG                # a bad grid is an error for an empty cloud too
    assert call(o=None) == E_ARG and b"origin3" in lib.sls_last_error()
    assert call(o=(C.c_double * 3)(0.0, float("nan"), 0.0)) == E_ARG
    for kw in ({"p": None}, {"out": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(cap=0, out=None, n=need - 1) == E_SCRATCH                   # (no room asked for: a null output is legal)
    assert call(M=0, p=None, out=None, status=None, s=None, n=0) == 0       # an empty cloud: success, nothing touched
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_tsdf_blocks")


def test_integrate_argument_errors_need_no_device():
    lib = _abi.lib()
    cam = _camera()

    def call(c=cam, B=5, blocks=FAKE, t=FAKE, w=FAKE, am=FAKE, vs=0.1, tr=0.4, o=ORIGIN, mo=0.5, md=0.1, dr=0.0):
        return lib.sls_tsdf_integrate(C.byref(c) if c is not None else None, B, blocks, t, w, am, vs, tr, o, mo, md, dr, None)
    assert call(c=None) == E_ARG and b"null pointer" in lib.sls_last_error()
    assert call(B=-1) == E_ARG and b"B negative" in lib.sls_last_error()
    assert call(B=(1 << 19) + 1) == E_ARG
    for H, W in ((0, 64), (16, 0), (-1, 64), (1 << 16, 1 << 16)):
        assert call(c=_camera(H, W)) == E_ARG and b"image size" in lib.sls_last_error(), (H, W)
    for vs, tr in BAD_GRIDS:
        assert call(vs=vs, tr=tr) == E_ARG and b"voxel_size" in lib.sls_last_error(), (vs, tr)
    assert call(o=None) == E_ARG and b"origin3" in lib.sls_last_error()
    for kw in ({"mo": float("nan")}, {"md": float("nan")}, {"dr": float("nan")}):
        assert call(**kw) == E_ARG and b"NaN" in lib.sls_last_error(), kw
    for kw in ({"blocks": None}, {"t": None}, {"w": None}, {"am": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(B=0, blocks=None, t=None, w=None, am=None) == 0             # no block: success, nothing launched
    assert call(B=0, vs=-1.0) == E_ARG                                      # ... but a bad grid stays an error


def test_extract_argument_errors_need_no_device():
    lib = _abi.lib()

    def count(B=5, blocks=FAKE, t=FAKE, w=FAKE, mw=1.0, counts=FAKE, prefix=FAKE, status=FAKE):
        return lib.sls_tsdf_extract_count(B, blocks, t, w, mw, counts, prefix, status, None)
    assert count(B=-1) == E_ARG and b"B negative" in lib.sls_last_error()
    assert count(B=(1 << 19) + 1) == E_ARG
    assert count(mw=float("nan")) == E_ARG and b"min_weight" in lib.sls_last_error()
    for kw in ({"blocks": None}, {"t": None}, {"w": None}, {"counts": None}, {"prefix": None}, {"status": None}):
        assert count(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert count(B=0, status=None) == E_ARG                                 # the total has to go somewhere

    def emit(B=5, blocks=FAKE, t=FAKE, w=FAKE, mw=1.0, vs=0.1, o=ORIGIN, prefix=FAKE, T=10, out=FAKE):
        return lib.sls_tsdf_extract_emit(B, blocks, t, w, mw, vs, o, prefix, T, out, None)
    assert emit(B=-1) == E_ARG and b"B negative" in lib.sls_last_error()
    assert emit(mw=float("nan")) == E_ARG and b"min_weight" in lib.sls_last_error()
    for vs in (0.0, -0.1, float("nan"), float("inf")):
        assert emit(vs=vs) == E_ARG and b"voxel_size" in lib.sls_last_error(), vs
    assert emit(o=None) == E_ARG and b"origin3" in lib.sls_last_error()
    for kw in ({"blocks": None}, {"t": None}, {"w": None}, {"prefix": None}, {"out": None}):
        assert emit(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert emit(T=0, blocks=None, t=None, w=None, prefix=None, out=None) == 0         # no triangle: success, nothing launched
    assert emit(B=0, blocks=None, t=None, w=None, prefix=None, out=None) == 0


def test_save_mesh_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    v = rng.normal(0, 10, (50, 3)).astype(np.float32)
    v[0] = [-0.0, np.float32(1e-40), 3e38]                   # a negative zero, a denormal, a huge value: bits, not values
    f = rng.integers(0, 50, (120, 3)).astype(np.int32)
    ply_io.save_mesh(tmp_path / "sub" / "m.ply", v, f)
    v2, f2 = ply_io.load_mesh(tmp_path / "sub" / "m.ply")
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
    assert np.array_equal(ply_io.load_point_cloud(tmp_path / "sub" / "m.ply")[0].view(np.uint32), v.view(np.uint32))
    ply_io.save_mesh(tmp_path / "t.ply", torch.from_numpy(v), torch.from_numpy(f).long())         # tensors, int64 faces
    assert (tmp_path / "t.ply").read_bytes() == (tmp_path / "sub" / "m.ply").read_bytes()
    ply_io.save_mesh(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v3, f3 = ply_io.load_mesh(tmp_path / "e.ply")
    assert v3.shape == (0, 3) and f3.shape == (0, 3)
    with pytest.raises(ValueError, match="int32"):
        ply_io.save_mesh(tmp_path / "bad.ply", v, np.array([[0, 1, -1]]))


def test_tsdf_refuses_cpu_tensors_and_bad_grids():
    pts = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        tsdf.allocate_blocks(pts, 0.1, 0.4)
    with pytest.raises(RuntimeError, match="device tensor"):
        tsdf.allocate_blocks(pts.numpy(), 0.1, 0.4)
    with pytest.raises(RuntimeError, match="device tensor"):
        tsdf.TsdfVolume(torch.zeros((2, 3), dtype=torch.int32), 0.1, 0.4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        meshing.mesh_tsdf("nowhere", 0.1, device="cpu")


def test_compose_volume_to_view_inverts_compose_cam_to_world():
    rng = np.random.default_rng(8)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q * np.sign(np.linalg.det(q)), [30.0, -20.0, 2.0]
    q2, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    view = np.eye(4, dtype=np.float32)
    view[:3, :3], view[:3, 3] = q2 * np.sign(np.linalg.det(q2)), [1.0, 2.0, -0.5]
    fwd = np.vstack([meshing.compose_cam_to_world(T, view).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float64)
    back = np.vstack([tsdf.compose_volume_to_view(T, view).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float64)
    assert np.abs(back @ fwd - np.eye(4)).max() <= 1e-5
