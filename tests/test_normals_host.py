"""Host side of the PCA normal estimate (sls_cloud_normals, splat_loam_amd/evaluation.py: estimate_normals,
projector.py: DeviceProjector(normals="pca")): exports and constants, scratch sizes, every argument error (all checked before
a launch: no device needed), the refusal of CPU tensors, and options rejected before any work."""
import ctypes

import pytest
import torch

from splat_loam_amd import _abi, evaluation, projector

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
NN_MAX = 64


def header(name):
    return open(_abi.LIB_PATH.replace("splat_loam_amd/libsls_hip.so", "include/" + name)).read()


def test_exports_and_constants():
    lib = _abi.lib()
    for name in ("sls_cloud_normals_scratch_bytes", "sls_cloud_normals"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    assert f"#define SLS_NORMALS_NN_MAX {NN_MAX}" in header("sls_abi.h") and "#define SLS_NN_K_MAX 32" in header("sls_abi.h")
    assert f"#define SLS_NORMALS_NN_MAX {NN_MAX}" in header("sls_normals_math.h")
    assert evaluation.NORMALS_NN_MAX == NN_MAX and evaluation.NN_K_MAX == 32
    # lists beyond 32 are this call's alone: the k-nearest query and the filters still stop at 32
    assert lib.sls_nn_k_scratch_bytes(100, 100, 33) == 0 and lib.sls_outlier_scratch_bytes(100, 33) == 0
    assert lib.sls_nn_query_k(100, FAKE, 50, FAKE, 33, FAKE, FAKE, None, FAKE, 1 << 30, None) == E_ARG


def test_scratch_bytes():
    lib = _abi.lib()
    need = lib.sls_cloud_normals_scratch_bytes
    for M, k in ((0, 3), (-1, 3), (10, 0), (10, -2), (10, NN_MAX + 1), (10, 1000)):
        assert need(M, k) == 0, (M, k)
    sizes = (1, 2, 255, 256, 257, 6000, 200001, 2000000)
    up = lambda v: (v + 255) & ~255
    for k in (1, 4, 5, 20, 32, 33, 50, 64):
        for M in sizes:
            n = need(M, k)
            assert n % 256 == 0 and n >= lib.sls_nn_scratch_bytes(M, M) + 8 * M * k + 8 * M > 0
            assert n == up(lib.sls_nn_scratch_bytes(M, M)) + 2 * up(4 * M * k) + up(8 * M)   # the rows' places (sls_abi.h)
            assert n <= need(M + 1, k) and (k == NN_MAX or n <= need(M, k + 1))
            if k <= 32:
                assert n >= lib.sls_nn_k_scratch_bytes(M, M, k) + 8 * M * k
    for a, b in zip(sizes, sizes[1:]):
        assert need(a, 50) <= need(b, 50)
    assert need(2**31 - 1, 64) > 2**39                                                # 64-bit arithmetic throughout


def test_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_cloud_normals_scratch_bytes(100, 50)
    view = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    VIEW = ctypes.addressof(view)

    def call(M=100, x=FAKE, k=50, r=0.5, v=VIEW, on=FAKE, oc=FAKE, oe=FAKE, s=FAKE, n=need):
        return lib.sls_cloud_normals(M, x, k, r, v, on, oc, oe, s, n, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for k in (0, -1, NN_MAX + 1, 1000):
        assert call(k=k) == E_ARG and b"k outside" in lib.sls_last_error(), k
        assert call(k=k, M=0) == E_ARG                                      # ... even with no point
    for r in (0.0, -1.0, float("nan"), float("-inf")):
        assert call(r=r) == E_ARG and b"radius" in lib.sls_last_error(), r
        assert call(r=r, M=0) == E_ARG
    for kw in ({"x": None}, {"v": None}, {"on": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(oc=None, oe=None, n=need - 1) == E_SCRATCH                  # (null count and eigenvalues are legal)
    assert call(r=float("inf"), n=need - 1) == E_SCRATCH                    # (+inf is a legal radius: the k nearest)
    assert call(k=64, n=lib.sls_cloud_normals_scratch_bytes(100, 64) - 1) == E_SCRATCH and call(k=1, n=0) == E_SCRATCH
    assert call(M=0, x=None, v=None, on=None, oc=None, oe=None, s=None, n=0) == 0       # an empty cloud: success, nothing touched
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_cloud_normals")


def test_cpu_tensors_and_bad_arguments_are_refused():
    a = torch.zeros((10, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.estimate_normals(a)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.estimate_normals(a.numpy(), 0.5, 30)
    with pytest.raises(RuntimeError, match="GPU only"):
        projector.DeviceProjector(16, 128, device="cpu", normals="pca")
    proj = object.__new__(projector.DeviceProjector)                        # (a real one needs a device)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        proj.pca_normals_image(a, None, None)
    # the argument checks themselves (no tensor is touched): max_nn outside the range is refused before any work
    for k in (0, -1, 65, 2.5, True):
        with pytest.raises(ValueError, match=r"max_nn must be an integer in \[1, 64\]"):
            evaluation._check_normals_args(0.5, k, (0, 0, 0))
        with pytest.raises(ValueError, match="max_nn"):
            projector.DeviceProjector(16, 128, device="cpu", normals="pca", normal_max_nn=k)
    for r in (0.0, -2.0, float("nan"), 1e39):
        with pytest.raises(ValueError, match="radius"):
            evaluation._check_normals_args(r, 30, (0, 0, 0))
        with pytest.raises(ValueError, match="radius"):
            projector.DeviceProjector(16, 128, device="cpu", normals="pca", normal_radius=r)
    for v in ((0, 0), (0, 0, float("nan")), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="viewpoint"):
            evaluation._check_normals_args(0.5, 30, v)
    assert evaluation._check_normals_args(None, 50, (1, 2, 3)) == (float("inf"), 50, (1.0, 2.0, 3.0))
    assert evaluation._check_normals_args(0.5, 64.0, (0, 0, 0))[1] == 64
    with pytest.raises(ValueError, match="radial"):
        projector.DeviceProjector(16, 128, device="cpu", normals="open3d")
    with pytest.raises(RuntimeError, match="GPU only"):                     # the default is untouched: no normal option is read
        projector.DeviceProjector(16, 128, device="cpu", normal_max_nn=1000)
