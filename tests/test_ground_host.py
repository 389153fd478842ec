"""Host side of the ground segmentation (sls_ground_segment, splat_loam_amd/evaluation.py: segment_ground, ground_normals,
projector.py: DeviceProjector(ground=True)): exports and constants, scratch sizes, every argument error (all checked before a
launch: no device needed), the refusal of CPU tensors, and options rejected before any work."""
import ctypes

import pytest
import torch

from splat_loam_amd import _abi, evaluation, projector

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
BINS = 504


def header(name):
    return open(_abi.LIB_PATH.replace("splat_loam_amd/libsls_hip.so", "include/" + name)).read()


def test_exports_and_constants():
    lib = _abi.lib()
    for name in ("sls_ground_scratch_bytes", "sls_ground_segment"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    for h in ("sls_abi.h", "sls_ground_math.h"):
        assert f"#define SLS_GROUND_BINS {BINS}" in header(h) and "typedef struct SlsGroundParams" in header(h)
    assert evaluation.GROUND_BINS == BINS and len(evaluation.GROUND_STATES) == 6
    assert ctypes.sizeof(_abi.SlsGroundParams) == 72
    # the Python defaults are the header's
    prm = evaluation._check_ground_args(1.723, {})
    text = header("sls_ground_math.h")
    for field, lit in (("sensor_height", "1.723f"), ("min_range", "2.7f"), ("max_range", "80.0f"), ("th_seeds", "0.5f"),
                       ("th_dist", "0.125f"), ("uprightness_thr", "0.707f"), ("noise_margin", "1.1f")):
        assert f"p->{field} = {lit};" in text and getattr(prm, field) == ctypes.c_float(float(lit[:-1])).value
    assert [prm.num_lpr, prm.num_iter, prm.num_min_pts] == [20, 3, 10]
    assert "p->num_lpr = 20; p->num_iter = 3; p->num_min_pts = 10;" in text
    assert list(prm.elevation_thr) == [ctypes.c_float(v).value for v in (0.523, 0.746, 0.879, 1.125)]
    assert list(prm.flatness_thr) == [ctypes.c_float(v).value for v in (5e-4, 7.25e-4, 1e-3, 1e-3)]


def test_scratch_bytes():
    need = _abi.lib().sls_ground_scratch_bytes
    for M in (0, -1, -2**31):
        assert need(M) == 0, M
    sizes = (1, 2, 255, 256, 257, 6000, 131072, 200001, 2000000)
    for M in sizes:
        n = need(M)
        assert n % 256 == 0 and n >= 40 * M > 0            # two key arrays, two value arrays, the float4 rows
        assert n <= need(M + 1)
    for a, b in zip(sizes, sizes[1:]):
        assert need(a) <= need(b)
    assert need(2**31 - 1) > 40 * (2**31 - 1) > 2**36       # 64-bit arithmetic throughout


def test_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_ground_scratch_bytes(100)

    def call(M=100, x=FAKE, p=None, ol=FAKE, ob=FAKE, op=FAKE, oi=FAKE, os=FAKE, s=FAKE, n=need, null_prm=False, **fields):
        prm = evaluation._check_ground_args(1.723, {})
        for k, v in fields.items():
            if isinstance(v, tuple):
                v = (ctypes.c_float * 4)(*v)
            setattr(prm, k, v)
        return lib.sls_ground_segment(M, x, None if null_prm else ctypes.byref(prm), ol, ob, op, oi, os, s, n, None)

    def refused(text, **kw):
        assert call(**kw) == E_ARG and text in lib.sls_last_error(), (kw, lib.sls_last_error())
        if not set(kw) & {"M", "x", "ol", "s"}:                             # ... even with no point (where that is no legal call)
            assert call(**dict(kw, M=0)) == E_ARG and text in lib.sls_last_error(), kw
    refused(b"negative M", M=-1)
    refused(b"null pointer", null_prm=True)
    refused(b"null pointer", os=None)
    for kw in ({"x": None}, {"ol": None}, {"s": None}):
        refused(b"null pointer", **kw)
    for off in (1, 4, 16, 128, 255):
        refused(b"aligned", s=FAKE + off)
    bad = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))
    for v in bad:
        refused(b"min_range, max_range", min_range=v)
        refused(b"min_range, max_range", max_range=v)
        refused(b"sensor_height", sensor_height=v)
        for name in ("th_seeds", "th_dist", "uprightness_thr", "noise_margin"):
            refused(b"th_seeds, th_dist, uprightness_thr, noise_margin", **{name: v})
        for c in range(4):
            four = [0.5] * 4
            four[c] = v
            refused(b"elevation_thr, flatness_thr", elevation_thr=tuple(four))
            refused(b"elevation_thr, flatness_thr", flatness_thr=tuple(four))
    refused(b"min_range >= max_range", min_range=80.0)
    refused(b"min_range >= max_range", min_range=5.0, max_range=4.0)
    for v in (0, -1, 9, 1000):
        refused(b"num_iter outside [1, 8]", num_iter=v)
    for v in (0, -5):
        refused(b"num_lpr < 1", num_lpr=v)
    for v in (2, 0, -1):
        refused(b"num_min_pts < 3", num_min_pts=v)
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(ob=None, op=None, oi=None, n=need - 1) == E_SCRATCH         # (null bin, planes and info are legal)
    assert call(num_iter=1, n=need - 1) == E_SCRATCH and call(num_iter=8, num_lpr=1, num_min_pts=3, n=need - 1) == E_SCRATCH
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_ground_segment")
    # M == 0 needs neither points nor scratch, but its parameters and its status are still checked (that it succeeds and
    # writes the status alone is a launch: tests/test_ground.py)
    assert call(M=0, x=None, ol=None, s=None, n=0, os=None) == E_ARG and b"null pointer" in lib.sls_last_error()
    assert call(M=0, x=None, ol=None, s=None, n=0, num_iter=0) == E_ARG and b"num_iter" in lib.sls_last_error()


def test_cpu_tensors_and_bad_arguments_are_refused():
    a = torch.zeros((10, 3))
    for fn in (evaluation.segment_ground, evaluation.ground_normals):
        with pytest.raises(RuntimeError, match="device tensor"):
            fn(a)
        with pytest.raises(RuntimeError, match="device tensor"):
            fn(a.numpy(), 1.5)
    check = evaluation._check_ground_args
    for v in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="sensor_height"):
            check(v, {})
        for name in ("min_range", "max_range", "th_seeds", "th_dist", "uprightness_thr", "noise_margin"):
            with pytest.raises(ValueError, match=name):
                check(1.7, {name: v})
        with pytest.raises(ValueError, match="elevation_thr"):
            check(1.7, {"elevation_thr": (0.5, v, 0.5, 0.5)})
        with pytest.raises(ValueError, match="flatness_thr"):
            check(1.7, {"flatness_thr": (1e-3, 1e-3, 1e-3, v)})
    # the value is judged as the float32 the C struct holds: one that rounds to 0 or to infinity is refused here, not by
    # the native call later, and one below FLT_MAX is legal as it is there
    for v in (1e-50, -1e-50, 3.5e38, "x", None):
        with pytest.raises(ValueError, match="th_dist"):
            check(1.7, {"th_dist": v})
        with pytest.raises(ValueError, match="sensor_height"):
            check(v, {})
    assert check(1.7, {"max_range": 3.2e38, "th_dist": 1e-40}).max_range == ctypes.c_float(3.2e38).value
    with pytest.raises(ValueError, match="four"):
        check(1.7, {"elevation_thr": 0.5})
    with pytest.raises(ValueError, match="four"):
        check(1.7, {"elevation_thr": (0.5, 0.5, 0.5)})
    with pytest.raises(ValueError, match="min_range must be below max_range"):
        check(1.7, {"min_range": 90.0})
    for name, values in (("num_iter", (0, 9, -1)), ("num_lpr", (0, -3)), ("num_min_pts", (2, 0))):
        for v in values:
            with pytest.raises(ValueError, match=name):
                check(1.7, {name: v})
        for v in (2.5, True, float("inf"), float("nan"), 2**31, "3", None):
            with pytest.raises(ValueError, match=name):
                check(1.7, {name: v})
    with pytest.raises(ValueError, match="unknown ground parameter 'th_seed'"):
        check(1.7, {"th_seed": 0.5})
    with pytest.raises(ValueError, match="unknown ground parameter"):
        check(1.7, {"sensor_height": 2.0})                                  # (it has its own argument)
    prm = check(2.0, {"num_iter": 8, "max_range": 50, "flatness_thr": [1e-3] * 4})
    assert prm.sensor_height == 2.0 and prm.num_iter == 8 and prm.max_range == 50.0 and prm.num_lpr == 20


def test_device_projector_option_checks():
    P = projector.DeviceProjector
    # the existing order: the `normals` value first (its text names "radial"), then the pca options, then the ground
    # options — only when ground=True — and the device check after every option check
    with pytest.raises(ValueError, match="radial"):
        P(16, 128, device="cpu", normals="open3d", ground=True, sensor_height=-1.0)
    with pytest.raises(ValueError, match="max_nn"):
        P(16, 128, device="cpu", normals="pca", normal_max_nn=1000, ground=True, sensor_height=-1.0)
    with pytest.raises(ValueError, match="sensor_height"):
        P(16, 128, device="cpu", ground=True, sensor_height=-1.0)
    with pytest.raises(ValueError, match="sensor_height"):
        P(16, 128, device="cpu", normals="pca", ground=True, sensor_height=float("nan"))
    with pytest.raises(ValueError, match="num_iter"):
        P(16, 128, device="cpu", ground=True, ground_params={"num_iter": 9})
    with pytest.raises(ValueError, match="unknown ground parameter"):
        P(16, 128, device="cpu", ground=True, ground_params={"range": 9})
    with pytest.raises(RuntimeError, match="GPU only"):
        P(16, 128, device="cpu", ground=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        P(16, 128, device="cpu", ground=True, normals="pca", sensor_height=2.0, ground_params={"max_range": 50.0})
    # ground=False reads no ground option at all
    with pytest.raises(RuntimeError, match="GPU only"):
        P(16, 128, device="cpu", sensor_height=-1.0, ground_params={"num_iter": 100})
    with pytest.raises(RuntimeError, match="GPU only"):
        P(16, 128, device="cpu", normal_max_nn=1000)
    proj = object.__new__(P)                                                # (a real one needs a device)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        proj.ground_image(torch.zeros((10, 3)), None, None, None)
