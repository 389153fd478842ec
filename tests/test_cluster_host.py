"""Host side of the cloud clustering (sls_cloud_dbscan, sls_cloud_select, splat_loam_amd/evaluation.py, meshing.py): scratch
sizes, every argument error (all checked before a launch: no device needed), the refusal of CPU tensors, and options rejected
before any work."""
import numpy as np
import pytest
import torch

from splat_loam_amd import _abi, evaluation, meshing

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first


def test_exports_and_constants():
    lib = _abi.lib()
    for name in ("sls_cloud_dbscan_scratch_bytes", "sls_cloud_dbscan", "sls_cloud_select_scratch_bytes", "sls_cloud_select"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    root = _abi.LIB_PATH.replace("splat_loam_amd/libsls_hip.so", "include/")
    for header in ("sls_abi.h", "sls_cluster_math.h"):
        text = open(root + header).read()
        assert "#define SLS_CLUSTER_STATUS_WORDS 8" in text and "#define SLS_CLUSTER_SELECT_STATUS_WORDS 4" in text
    assert evaluation.CLUSTER_STATUS_WORDS == 8


def test_scratch_bytes():
    lib = _abi.lib()
    db, sel = lib.sls_cloud_dbscan_scratch_bytes, lib.sls_cloud_select_scratch_bytes
    assert db(0) == 0 and db(-1) == 0 and sel(0) == 0 and sel(-7) == 0
    sizes = (1, 2, 255, 256, 257, 1024, 1025, 6000, 200001, 2000000)
    for M in sizes:
        assert db(M) % 256 == 0 and db(M) >= lib.sls_knn_scratch_bytes(M) + 16 * M        # the index + four words a point
        assert sel(M) % 256 == 0 and sel(M) >= 256 + 4 * ((M + 1023) // 1024)
        assert db(M) <= db(M + 1) and sel(M) <= sel(M + 1)
    for a, b in zip(sizes, sizes[1:]):
        assert db(a) <= db(b) and sel(a) <= sel(b)


def test_dbscan_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_cloud_dbscan_scratch_bytes(100)

    def call(M=100, x=FAKE, eps=0.5, mp=10, lab=FAKE, cnt=FAKE, status=FAKE, s=FAKE, n=need):
        return lib.sls_cloud_dbscan(M, x, eps, mp, lab, cnt, status, s, n, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for eps in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(eps=eps) == E_ARG and b"eps is not a finite number > 0" in lib.sls_last_error(), eps
        assert call(eps=eps, M=0) == E_ARG                                   # ... even for an empty cloud
    assert call(eps=2.0e19) == E_ARG and b"eps * eps is not finite" in lib.sls_last_error()
    for mp in (0, -1, -(2 ** 31)):
        assert call(mp=mp) == E_ARG and b"min_points < 1" in lib.sls_last_error(), mp
    for kw in ({"x": None}, {"lab": None}, {"cnt": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(M=0, status=None) == E_ARG and b"null pointer" in lib.sls_last_error()
    for off in (1, 4, 64, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(mp=2 ** 31 - 1, n=need - 1) == E_SCRATCH                     # (min_points is not limited by a list length)
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_cloud_dbscan")


def test_select_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_cloud_select_scratch_bytes(100)

    def call(M=100, x=FAKE, nrm=None, lab=FAKE, cnt=FAKE, cs=FAKE, keep=1, floor=0, ox=FAKE, on=None, oi=FAKE, status=FAKE, s=FAKE,
             n=need):
        return lib.sls_cloud_select(M, x, nrm, lab, cnt, cs, keep, floor, ox, on, oi, status, s, n, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for kw in ({"x": None}, {"lab": None}, {"cnt": None}, {"cs": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(M=0, status=None) == E_ARG
    assert call(on=FAKE) == E_ARG and b"out_normals without normals" in lib.sls_last_error()
    assert call(s=FAKE + 128) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    for keep, floor in ((0, 0), (-5, -5), (2 ** 31 - 1, 2 ** 31 - 1)):          # any keep and floor are legal
        assert call(keep=keep, floor=floor, nrm=FAKE, on=FAKE, ox=None, oi=None, n=need - 1) == E_SCRATCH


def test_cpu_tensors_and_bad_arguments_are_refused():
    a = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.cluster_dbscan(a, 0.5)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.keep_clusters(a, 0.5)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.cluster_dbscan(a.numpy(), 0.5)
    # the argument checks themselves (no tensor is touched): the messages name the argument
    for eps in (0.0, -2.0, float("nan"), float("inf"), 2.0e19, 1e300):
        with pytest.raises(ValueError, match="eps"):
            evaluation._check_cluster_args(eps, 10)
    for mp in (0, -1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_points"):
            evaluation._check_cluster_args(0.5, mp)
    assert evaluation._check_cluster_args(0.1, np.int64(100)) == (float(np.float32(0.1)), 100)
    assert evaluation._check_cluster_args(np.float32(0.25), 1.0) == (0.25, 1)
    for bad in (1.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="keep must"):
            evaluation._check_select_args(bad, 0)
        with pytest.raises(ValueError, match="min_cluster_points"):
            evaluation._check_select_args(1, bad)
    assert evaluation._check_select_args(-3, np.int32(7)) == (-3, 7)


def test_meshing_rejects_a_bad_cluster_option_before_any_work(tmp_path):
    """cluster_eps and its companions are checked first: before the results directory is read (this one does not exist) or a
    device is named."""
    missing = tmp_path / "no_such_results"
    for fn, args in ((meshing.sample_surface, ()), (meshing.mesh_tsdf, (0.1,)), (meshing.mesh_poisson, (0.1,))):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="eps"):
                fn(missing, *args, cluster_eps=bad)
        with pytest.raises(ValueError, match="min_points"):
            fn(missing, *args, cluster_eps=0.2, cluster_min_points=0)
        with pytest.raises(ValueError, match="keep"):
            fn(missing, *args, cluster_eps=0.2, cluster_keep=1.5)
        with pytest.raises(ValueError, match="min_cluster_points"):
            fn(missing, *args, cluster_eps=0.2, cluster_min_size=2.5)
    assert meshing._check_cluster(None, "ignored", "ignored", "ignored") is None
    assert meshing._check_cluster(0.25, 10, 1, 0) == (0.25, 10, 1, 0)
