"""Host side of the cloud registration (sls_cloud_icp, splat_loam_amd/evaluation.py: register_icp, evaluate_recon(align=)):
exports and constants, scratch sizes, every argument error (all checked before a launch: no device needed), the refusals of
the Python layer, and evaluate_recon's default path, which builds no registration call."""
import ctypes
import math
import re

import pytest
import torch

import icp_ref as ref
from splat_loam_amd import _abi, evaluation

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first


def header(name):
    return open(_abi.LIB_PATH.replace("splat_loam_amd/libsls_hip.so", "include/" + name)).read()


def params(**kw):
    p = _abi.SlsIcpParams(method=0, iterations=30, min_inliers=6, max_distance=1.0, damping=1e-9, eps_rot=1e-7, eps_trans=1e-7)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_exports_and_constants():
    lib = _abi.lib()
    for name in ("sls_cloud_icp_scratch_bytes", "sls_cloud_icp"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    abi, math_h = header("sls_abi.h"), header("sls_icp_math.h")
    for text in (abi, math_h):
        for name, value in (("SLS_ICP_PLANE", ref.PLANE), ("SLS_ICP_POINT", ref.POINT), ("SLS_ICP_FLAG_CONVERGED", ref.FLAG_CONVERGED),
                            ("SLS_ICP_FLAG_FEW", ref.FLAG_FEW), ("SLS_ICP_FLAG_NOT_PD", ref.FLAG_NOT_PD)):
            assert re.search(rf"#define {name} {value}\b", text), name
    assert f"#define SLS_ICP_STATUS_WORDS {ref.STATUS_WORDS}" in abi and "#define SLS_ICP_MAX_ITERATIONS 1000" in abi
    assert f"#define SLS_ICP_TERMS {ref.TERMS}" in math_h and f"#define SLS_ICP_BLOCK {ref.BLOCK}" in math_h
    assert evaluation.ICP_STATUS_WORDS == ref.STATUS_WORDS and evaluation.ICP_MAX_ITERATIONS == 1000
    assert evaluation.ICP_METHODS == {"plane": ref.PLANE, "point": ref.POINT}
    assert (evaluation.ICP_FLAG_CONVERGED, evaluation.ICP_FLAG_FEW, evaluation.ICP_FLAG_NOT_PD) == (1, 2, 4)
    assert evaluation.ICP_DEFAULTS == ref.DEFAULTS
    assert ctypes.sizeof(_abi.SlsIcpParams) == 40
    assert [f for f, _ in _abi.SlsIcpParams._fields_] == ["method", "iterations", "min_inliers", "max_distance", "damping", "eps_rot",
                                                        "eps_trans"]


def test_scratch_bytes():
    lib = _abi.lib()
    need = lib.sls_cloud_icp_scratch_bytes
    for Ms, Mt in ((-1, 10), (10, 0), (10, -3), (0, 0)):
        assert need(Ms, Mt) == 0, (Ms, Mt)
    sizes = (0, 1, 2, 255, 256, 257, 6000, 65536, 65537, 200001, 2000000)
    for Ms in sizes:
        for Mt in sizes[1:]:
            n = need(Ms, Mt)
            assert n % 256 == 0 and n >= lib.sls_nn_scratch_bytes(Mt, Ms) > 0
            # the moved source, the association, the target's packed rows, a partial row per block of 256
            assert n >= lib.sls_nn_scratch_bytes(Mt, Ms) + 20 * Ms + 32 * Mt + 256 * ((Ms + 255) // 256)
            assert n <= need(Ms + 1, Mt) and n <= need(Ms, Mt + 1)
    for a, b in zip(sizes, sizes[1:]):
        assert need(a, 5000) <= need(b, 5000) and need(5000, max(a, 1)) <= need(5000, b)
    assert need(2**31 - 1, 2**31 - 1) > 2**37                                         # 64-bit arithmetic throughout


def test_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_cloud_icp_scratch_bytes(100, 200)
    pose = (ctypes.c_double * 12)(*ref.IDENTITY)
    POSE = ctypes.addressof(pose)

    def call(Ms=100, src=FAKE, Mt=200, tgt=FAKE, nrm=FAKE, prm=None, init=POSE, status=FAKE, system=FAKE, index=FAKE, dist2=FAKE,
             s=FAKE, n=need, **kw):
        prm = params(**kw) if prm is None else prm
        return lib.sls_cloud_icp(Ms, src, Mt, tgt, nrm, ctypes.byref(prm) if prm else None, init, status, system, index, dist2, s, n,
                                 None)
    assert call(Ms=-1) == E_ARG and b"negative Ms" in lib.sls_last_error()
    for Mt in (0, -1):
        assert call(Mt=Mt) == E_ARG and b"Mt < 1" in lib.sls_last_error()
    for kw in ({"src": None}, {"tgt": None}, {"init": None}, {"status": None}, {"s": None}, {"prm": False}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(nrm=None) == E_ARG and b"normals" in lib.sls_last_error()
    assert call(nrm=None, method=1, n=need - 1) == E_SCRATCH                # (point-to-point needs none)
    for m in (-1, 2, 100):
        assert call(method=m) == E_ARG and b"method" in lib.sls_last_error()
    for d in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(max_distance=d) == E_ARG and b"max_distance" in lib.sls_last_error(), d
        assert call(max_distance=d, Ms=0) == E_ARG                          # ... even with no point
    for name in ("damping", "eps_rot", "eps_trans"):
        for v in (-1e-30, float("nan"), float("inf")):
            assert call(**{name: v}) == E_ARG and name.encode() in lib.sls_last_error(), (name, v)
        assert call(**{name: 0.0}, n=need - 1) == E_SCRATCH                 # (zero is legal)
    for it in (-1, 1001, 2**31 - 1):
        assert call(iterations=it) == E_ARG and b"iterations" in lib.sls_last_error()
    assert call(iterations=0, n=need - 1) == E_SCRATCH and call(iterations=1000, n=need - 1) == E_SCRATCH
    assert call(min_inliers=-1) == E_ARG and b"min_inliers" in lib.sls_last_error()
    for k in (0, 5, 11):
        for v in (float("nan"), float("inf")):
            bad = (ctypes.c_double * 12)(*ref.IDENTITY)
            bad[k] = v
            assert call(init=ctypes.addressof(bad)) == E_ARG and b"init_pose12" in lib.sls_last_error()
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(system=None, index=None, dist2=None, n=need - 1) == E_SCRATCH          # (the optional outputs may be null)
    assert call(Ms=0, src=None, n=lib.sls_cloud_icp_scratch_bytes(0, 200) - 1) == E_SCRATCH    # (an empty source needs no pointer)
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_cloud_icp")


def test_cpu_tensors_and_bad_arguments_are_refused():
    a, b = torch.zeros((10, 3)), torch.zeros((20, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.register_icp(a, b)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.register_icp(a.numpy(), b.numpy(), max_distance=0.5, method="point")
    # the argument checks themselves (no tensor is touched)
    chk = evaluation._check_icp_args
    prm, pose = chk(0.5, 30, "plane", None, {})
    assert (prm.method, prm.iterations, prm.min_inliers, prm.max_distance) == (0, 30, 6, 0.5) and pose == list(ref.IDENTITY)
    assert (prm.damping, prm.eps_rot, prm.eps_trans) == (1e-9, 1e-7, 1e-7)
    prm, pose = chk(2, 0, "point", torch.arange(16.0).view(4, 4), dict(damping=0.0, min_inliers=0))
    assert prm.method == 1 and prm.iterations == 0 and prm.damping == 0.0 and prm.min_inliers == 0 and pose == [float(v) for v in range(12)]
    assert chk(1, 1, "plane", list(range(12)), {})[1] == chk(1, 1, "plane", torch.arange(12.0).view(3, 4), {})[1]
    assert chk(1, 1, "plane", [0.1] * 12, {})[1] == [0.1] * 12                 # (a list is taken as float64, not through float32)
    for m in ("planes", 0, None):
        with pytest.raises(ValueError, match="method"):
            chk(1.0, 30, m, None, {})
    for d in (0.0, -1.0, math.nan, math.inf, 1e39, "x"):
        with pytest.raises(ValueError, match="max_distance"):
            chk(d, 30, "plane", None, {})
    for it in (-1, 1001, 2.5, True):
        with pytest.raises(ValueError, match="iterations"):
            chk(1.0, it, "plane", None, {})
    for name in ("damping", "eps_rot", "eps_trans"):
        for v in (-1.0, math.nan, math.inf, "x"):
            with pytest.raises(ValueError, match=name):
                chk(1.0, 30, "plane", None, {name: v})
    with pytest.raises(ValueError, match="min_inliers"):
        chk(1.0, 30, "plane", None, {"min_inliers": -1})
    with pytest.raises(ValueError, match="unknown ICP parameter 'huber'"):
        chk(1.0, 30, "plane", None, {"huber": 1.0})
    for init in (torch.zeros(3, 3), [1.0] * 11, torch.full((3, 4), math.nan)):
        with pytest.raises(ValueError, match="init"):
            chk(1.0, 30, "plane", init, {})
    for align in ({}, {"iterations": 3}, 0.5, {"max_distance": 1.0, "return_details": True}, {"max_distance": 1.0, "max_points": 0}):
        with pytest.raises(ValueError, match="align|max_points"):
            evaluation._align_vertices(b, a, align)
    # _icp_result: the status words as the dict
    w = ref.status_words(dict(updates=3, inliers=50, flags=1, sum_r2=0.5, pose=ref.pose12(ref.rotation([0, 0, 1], 0.1), [1, 2, 3])), 100, 7)
    r = evaluation._icp_result(w.tolist())
    assert r["updates"] == 3 and r["fitness"] == 0.5 and r["inlier_rmse"] == 0.1 and r["converged"] and not r["too_few_inliers"]
    assert tuple(r["target_T_source"].shape) == (4, 4) and r["target_T_source"].dtype == torch.float64
    assert r["target_T_source"][3].tolist() == [0, 0, 0, 1] and r["target_T_source"][:3, 3].tolist() == [1, 2, 3]
    assert evaluation._icp_result(ref.status_words(dict(updates=0, inliers=0, flags=2, sum_r2=0.0, pose=ref.IDENTITY), 0, 7).tolist())["fitness"] == 0.0


def test_evaluate_recon_without_align_builds_no_registration_call(monkeypatch):
    """align=None reaches the library without having touched the registration; a dict goes through it first."""
    class Reached(Exception):
        pass
    calls = []

    def no_lib():
        raise Reached()
    monkeypatch.setattr(evaluation, "_cloud", lambda t, name: t)
    monkeypatch.setattr(evaluation, "_mesh", lambda v, f: (v, f))
    monkeypatch.setattr(evaluation._abi, "lib", no_lib)
    monkeypatch.setattr(evaluation, "_align_vertices", lambda r, v, a: calls.append(a) or {"target_T_source": torch.eye(4, dtype=torch.float64)})
    monkeypatch.setattr(evaluation, "register_icp", lambda *a, **k: calls.append("register_icp"))
    ref_pts, verts, faces = torch.zeros((5, 3)), torch.ones((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(Reached):
        evaluation.evaluate_recon(ref_pts, verts, faces)
    with pytest.raises(Reached):
        evaluation.evaluate_recon(ref_pts, verts, faces, align=None)
    assert calls == []
    with pytest.raises(Reached):
        evaluation.evaluate_recon(ref_pts, verts, faces, align=dict(max_distance=0.5))
    assert calls == [dict(max_distance=0.5)]
    import inspect
    assert inspect.signature(evaluation.evaluate_recon).parameters["align"].default is None
