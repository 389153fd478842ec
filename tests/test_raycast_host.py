"""Host side of the ray caster (sls_mesh_rayindex_bytes, sls_mesh_rayindex_build, sls_mesh_raycast,
splat_loam_amd/evaluation.py: cast_rays, mesh_ray_index, render_mesh, meshing.mesh_depth_check): the index size, every
argument error (all checked before a launch: no device needed), the refusal of malformed arguments and of CPU tensors."""
import inspect
import math

import numpy as np
import pytest
import torch

from splat_loam_amd import _abi, evaluation, meshing

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first


def test_index_bytes_properties():
    lib = _abi.lib()
    size = lib.sls_mesh_rayindex_bytes
    assert size(0, 10) == 0 and size(10, 0) == 0 and size(-1, -1) == 0
    for V, F in ((1, 1), (3, 1), (100, 31), (200, 256), (300, 257), (9000, 16928), (600000, 1130000)):
        n = size(V, F)
        nboxes = (F + 255) // 256
        assert n % 256 == 0
        assert n >= 48 * F + 32 * nboxes * 9 + 16 * F           # three float4 per face, the boxes and sub-boxes, codes and indices
        assert n == size(V + 7, F)                              # (the vertices are read in place)
        assert n <= size(V, F + 1)
        # what one cast keeps (items, boxes) is what sls_mesh_distance keeps of its index: no second copy of the mesh
        assert n < lib.sls_mesh_distance_scratch_bytes(V, F, 0) + 48 * F + 65536


def test_rayindex_build_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_rayindex_bytes(100, 50)

    def call(V=100, v=FAKE, F=50, f=FAKE, index=FAKE, n=need, status=FAKE):
        return lib.sls_mesh_rayindex_build(V, v, F, f, index, n, status, None)
    assert call(F=0) == E_ARG and b"F < 1" in lib.sls_last_error()
    assert call(F=-3) == E_ARG
    assert call(V=0) == E_ARG and b"V < 1" in lib.sls_last_error()
    for kw in ({"v": None}, {"f": None}, {"index": None}, {"status": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(index=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"index too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    with pytest.raises(RuntimeError, match="index too small"):
        _abi.check(call(n=need - 1), "sls_mesh_rayindex_build")


def test_raycast_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_rayindex_bytes(100, 50)

    def call(V=100, v=FAKE, F=50, f=FAKE, index=FAKE, n=need, Mr=20, o=FAKE, d=FAKE, t_min=0.0, t_max=math.inf, t=FAKE, face=FAKE,
             uv=FAKE, status=FAKE):
        return lib.sls_mesh_raycast(V, v, F, f, index, n, Mr, o, d, t_min, t_max, t, face, uv, status, None)
    assert call(F=0) == E_ARG and b"F < 1" in lib.sls_last_error()
    assert call(V=0) == E_ARG and b"V < 1" in lib.sls_last_error()
    assert call(Mr=-1) == E_ARG and b"Mr" in lib.sls_last_error()
    assert call(F=0, Mr=0) == E_ARG                                     # an empty mesh is an error even with no ray
    for kw in ({"v": None}, {"f": None}, {"index": None}, {"o": None}, {"d": None}, {"t": None}, {"status": None},
               {"Mr": 0, "status": None}, {"Mr": 0, "index": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(index=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    for t_min in (-1.0, -1e-30, float("nan"), -math.inf):
        assert call(t_min=t_min) == E_ARG and b"t_min" in lib.sls_last_error(), t_min
    for t_min, t_max in ((1.0, 0.5), (0.0, float("nan")), (0.0, -1.0), (math.inf, 1.0)):
        assert call(t_min=t_min, t_max=t_max) == E_ARG and b"t_max" in lib.sls_last_error(), (t_min, t_max)
    assert call(n=need - 1) == E_SCRATCH and b"index too small" in lib.sls_last_error()
    assert call(face=None, uv=None, n=need - 1) == E_SCRATCH            # (the two optional outputs: the size check is reached)
    assert call(Mr=0, o=None, d=None, t=None, n=need - 1) == E_SCRATCH  # Mr == 0 writes the status
    assert call(t_min=2.0, t_max=2.0, n=need - 1) == E_SCRATCH          # an empty range is not: t_min == t_max is allowed


def test_python_refuses_cpu_tensors_and_bad_arguments():
    o, d = torch.zeros((4, 3)), torch.ones((4, 3))
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.cast_rays(o, d, v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.mesh_ray_index(v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.render_mesh(v, f, camera=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshing.mesh_depth_check("nowhere", v, f, device="cpu")
    with pytest.raises(TypeError, match="unexpected keyword argument 'kf_samples'"):
        meshing.mesh_depth_check("nowhere", v, f, kf_samples=5)
    for lo, hi in ((-1.0, 1.0), (float("nan"), 1.0), (2.0, 1.0), (0.0, float("nan")), ("a", 1.0)):
        with pytest.raises(ValueError):
            evaluation._check_t_range(lo, hi)
    assert evaluation._check_t_range(0, math.inf) == (0.0, math.inf) and evaluation._check_t_range(1.5, 1.5) == (1.5, 1.5)


def test_signatures_and_the_options_stated_once():
    sig = inspect.signature(evaluation.cast_rays)
    assert list(sig.parameters) == ["origins", "directions", "vertices", "faces", "t_min", "t_max", "return_face", "return_uv", "index"]
    assert (sig.parameters["t_min"].default, sig.parameters["t_max"].default) == (0.0, math.inf)
    assert sig.parameters["return_face"].default is True and sig.parameters["return_uv"].default is False
    assert list(inspect.signature(evaluation.render_mesh).parameters) == ["vertices", "faces", "camera", "t_max", "index"]
    # mesh_depth_check states no default of the sampler's options: they are sample_surface's
    params = inspect.signature(meshing.mesh_depth_check).parameters
    assert params["truncation"].default == 0.5 and "options" in params
    assert not set(meshing._DEPTH_CHECK_OPTIONS) & set(params)
    assert set(meshing._DEPTH_CHECK_OPTIONS) <= set(meshing._SAMPLE_OPTIONS)
