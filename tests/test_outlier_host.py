"""Host side of the k-nearest-neighbour query and the outlier filters (sls_nn_query_k, sls_outlier_statistical,
sls_outlier_radius, splat_loam_amd/evaluation.py, meshing.py): scratch sizes, every argument error (all checked before a
launch: no device needed), the refusal of CPU tensors, and options rejected before any work."""
import numpy as np
import pytest
import torch

from splat_loam_amd import _abi, evaluation, meshing

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
K_MAX = 32


def test_exports_and_constants():
    lib = _abi.lib()
    for name in ("sls_nn_k_scratch_bytes", "sls_nn_query_k", "sls_outlier_scratch_bytes", "sls_outlier_statistical",
                 "sls_outlier_radius"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    header = open(_abi.LIB_PATH.replace("splat_loam_amd/libsls_hip.so", "include/sls_abi.h")).read()
    assert f"#define SLS_NN_K_MAX {K_MAX}" in header and "#define SLS_OUTLIER_STATUS_WORDS 8" in header
    assert evaluation.NN_K_MAX == K_MAX


def test_scratch_bytes():
    lib = _abi.lib()
    nnk, out = lib.sls_nn_k_scratch_bytes, lib.sls_outlier_scratch_bytes
    assert nnk(0, 10, 3) == 0 and nnk(-1, 10, 3) == 0 and nnk(10, -1, 3) == 0
    assert nnk(10, 10, 0) == 0 and nnk(10, 10, K_MAX + 1) == 0 and nnk(10, 10, -4) == 0
    assert out(0, 3) == 0 and out(-1, 3) == 0 and out(10, 0) == 0 and out(10, K_MAX + 1) == 0
    sizes = (1, 2, 255, 256, 257, 6000, 200001, 2000000)
    for k in (1, 4, 5, 20, 32):
        for Mt in sizes:
            for Mq in (0, 1, 257, 2000000):
                n = nnk(Mt, Mq, k)
                assert n % 256 == 0 and n >= lib.sls_nn_scratch_bytes(Mt, Mq) > 0
                assert n <= nnk(Mt + 1, Mq, k) and n <= nnk(Mt, Mq + 1, k) and (k == K_MAX or n <= nnk(Mt, Mq, k + 1))
            n = out(Mt, k)
            assert n % 256 == 0 and n >= nnk(Mt, Mt, k) + 8 * Mt             # the query's scratch + 8 bytes a point
            assert n <= out(Mt + 1, k) and (k == K_MAX or n <= out(Mt, k + 1))
    for a, b in zip(sizes, sizes[1:]):
        assert nnk(a, 100, 20) <= nnk(b, 100, 20) and nnk(100, a, 20) <= nnk(100, b, 20) and out(a, 20) <= out(b, 20)


def test_nn_query_k_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_nn_k_scratch_bytes(100, 50, 20)

    def call(Mt=100, t=FAKE, Mq=50, q=FAKE, k=20, d=FAKE, i=FAKE, m=FAKE, s=FAKE, n=need):
        return lib.sls_nn_query_k(Mt, t, Mq, q, k, d, i, m, s, n, None)
    assert call(Mt=0) == E_ARG and b"Mt < 1" in lib.sls_last_error()
    assert call(Mt=-5) == E_ARG and call(Mt=0, Mq=0) == E_ARG
    assert call(Mq=-1) == E_ARG and b"Mq" in lib.sls_last_error()
    for k in (0, -1, K_MAX + 1, 1000):
        assert call(k=k) == E_ARG and b"k outside" in lib.sls_last_error(), k
        assert call(k=k, Mq=0) == E_ARG                                     # ... even with no query
    assert call(Mq=0, t=None, q=None, d=None, i=None, m=None, s=None, n=0) == 0     # no query: success, nothing touched
    for kw in ({"t": None}, {"q": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(d=None, i=None, m=None, n=need - 1) == E_SCRATCH            # (null outputs are legal: the size check is reached)
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_nn_query_k")


@pytest.mark.parametrize("which", ["statistical", "radius"])
def test_outlier_argument_errors_need_no_device(which):
    lib = _abi.lib()
    stat = which == "statistical"
    need = lib.sls_outlier_scratch_bytes(100, 20)

    def call(M=100, x=FAKE, nrm=None, k=20 if stat else 19, p=2.0 if stat else 0.5, ox=FAKE, on=None, oi=FAKE, os_=FAKE, s=FAKE, n=need):
        fn = lib.sls_outlier_statistical if stat else lib.sls_outlier_radius
        return fn(M, x, nrm, k, p, ox, on, oi, os_, s, n, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    bad_k = (0, -1, K_MAX + 1) if stat else (-1, K_MAX, 100)
    for k in bad_k:
        assert call(k=k) == E_ARG and b"outside" in lib.sls_last_error(), k
        assert call(k=k, M=0) == E_ARG
    for p in (0.0, -1.0, float("nan"), float("inf")):
        assert call(p=p) == E_ARG and b"finite number > 0" in lib.sls_last_error(), p
    for kw in ({"x": None}, {"os_": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(on=FAKE) == E_ARG and b"out_normals without normals" in lib.sls_last_error()
    assert call(s=FAKE + 64) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nrm=FAKE, on=FAKE, ox=None, oi=None, n=need - 1) == E_SCRATCH   # (null outputs, normals: legal)
    assert call(M=0, x=None, ox=None, oi=None, os_=None, s=None, n=0) == 0      # an empty cloud: success, nothing touched
    if not stat:
        assert call(k=0, n=lib.sls_outlier_scratch_bytes(100, 1) - 1) == E_SCRATCH      # nb_points = 0 is legal


def test_cpu_tensors_and_bad_arguments_are_refused():
    a, b = torch.zeros((4, 3)), torch.ones((5, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.nearest_k(a, b, 3)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.remove_statistical_outlier(a)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.remove_radius_outlier(a, 3, 0.5)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.nearest_k(a.numpy(), b, 3)
    # the argument checks themselves (no tensor is touched)
    for k in (0, -1, 33, 2.5, True):
        with pytest.raises(ValueError, match=r"\[1, 32\]"):
            evaluation._check_k(k, "k")
        with pytest.raises(ValueError, match="nb_neighbors"):
            evaluation._check_stat_args(k, 2.0)
    assert evaluation._check_k(np.int64(20), "k") == 20 and evaluation._check_k(20.0, "k") == 20
    for r in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="std_ratio"):
            evaluation._check_stat_args(20, r)
    for nb in (-1, 32):
        with pytest.raises(ValueError, match=r"nb_points must be an integer in \[0, 31\]"):
            evaluation._check_k(nb, "nb_points", 0, 31)


def test_meshing_rejects_a_bad_outlier_option_before_any_work(tmp_path):
    """outlier_nb is checked first: before the results directory is read (this one does not exist) or a device is named."""
    missing = tmp_path / "no_such_results"
    for bad in (0, 33, -5, 2.5):
        with pytest.raises(ValueError, match="nb_neighbors"):
            meshing.sample_surface(missing, outlier_nb=bad)
        with pytest.raises(ValueError, match="nb_neighbors"):
            meshing.mesh_tsdf(missing, 0.1, outlier_nb=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="std_ratio"):
            meshing.sample_surface(missing, outlier_nb=20, outlier_std=bad)
        with pytest.raises(ValueError, match="std_ratio"):
            meshing.mesh_tsdf(missing, 0.1, outlier_nb=20, outlier_std=bad)
    assert meshing._check_outlier(None, "ignored") is None and meshing._check_outlier(20, 2) == (20, 2.0)
