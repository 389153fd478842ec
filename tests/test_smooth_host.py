"""Host side of the smoothing stage (sls_mesh_adjacency, sls_mesh_smooth, mesh_ops.vertex_adjacency, mesh_ops.smooth): the
scratch sizes, every argument error (all checked before a launch: no device needed), the refusal of CPU tensors and bad
arguments, and the bindings of the new symbols."""
import math

import pytest
import torch

from splat_loam_amd import _abi, mesh_ops

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
OTHER = 0x20000
MAX_T = 1 << 29         # SLS_MESH_MAX_TRIANGLES
MAX_V = 3 * MAX_T       # SLS_MESH_MAX_VERTICES
SIZES = (1, 2, 255, 2047, 2048, 2049, 3000, 40_000, 1_000_000)


@pytest.mark.parametrize("name", ("sls_mesh_adjacency_scratch_bytes", "sls_mesh_smooth_scratch_bytes"))
def test_scratch_bytes(name):
    fn = getattr(_abi.lib(), name)
    assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(-1, 5) == 0 and fn(5, -1) == 0
    assert fn(5, MAX_T + 1) == 0 and fn(MAX_V + 1, 5) == 0 and fn(MAX_V, MAX_T) > 0
    for a in SIZES:
        assert fn(a, 100) % 256 == 0 and fn(100, a) % 256 == 0 and fn(a, a) > 0
    for lo, hi in zip(SIZES, SIZES[1:]):                            # monotone in each argument
        assert fn(lo, 100) <= fn(hi, 100) and fn(100, lo) <= fn(100, hi) and fn(lo, lo) <= fn(hi, hi)
    for n in SIZES:                                                 # two copies of the 6 T pairs of u32 and the sorter's own scratch
        assert fn(n, n) >= _abi.lib().sls_sort_scratch_bytes(6 * n) + 2 * 8 * 6 * n


def test_smooth_scratch_holds_the_adjacency_and_the_two_buffers():
    lib = _abi.lib()
    for n in SIZES:                                                 # offsets, neighbours, boundary flags, two float4 buffers
        assert lib.sls_mesh_smooth_scratch_bytes(n, n) >= lib.sls_mesh_adjacency_scratch_bytes(n, n) + 4 * (n + 1) + 24 * n + n + 32 * n


def test_adjacency_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_adjacency_scratch_bytes(60, 100)

    def call(V=60, T=100, f=FAKE, off=FAKE, nbr=FAKE, bnd=FAKE, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_adjacency(V, T, f, off, nbr, bnd, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG and b"SLS_MESH_MAX_VERTICES" in lib.sls_last_error()
    for kw in ({"f": None}, {"off": None}, {"nbr": None}, {"bnd": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(V=0, f=None, off=None, nbr=None, bnd=None, status=None, s=None, nb=0) == 0      # no vertex: nothing to write
    assert call(T=0, off=None, status=None) == E_ARG and b"null pointer" in lib.sls_last_error()  # V > 0: the offsets are written


def test_smooth_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_smooth_scratch_bytes(60, 100)

    def call(V=60, v=FAKE, T=100, f=FAKE, method=2, weights=1, n=3, lam=0.5, mu=-0.53, fix=0, out=OTHER, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_smooth(V, v, T, f, method, weights, n, lam, mu, fix, out, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG and b"SLS_MESH_MAX_VERTICES" in lib.sls_last_error()
    for method in (-1, 3, 9):
        assert call(method=method) == E_ARG and b"method" in lib.sls_last_error(), method
    for weights in (-1, 2, 5):
        assert call(weights=weights) == E_ARG and b"weights" in lib.sls_last_error(), weights
    for n in (-1, -100):
        assert call(n=n) == E_ARG and b"iterations" in lib.sls_last_error(), n
    for bad in (math.inf, -math.inf, math.nan):
        assert call(lam=bad) == E_ARG and b"finite" in lib.sls_last_error(), bad
        assert call(mu=bad) == E_ARG and b"finite" in lib.sls_last_error(), bad
    assert call(out=FAKE) == E_ARG and b"must not be vertices" in lib.sls_last_error()           # no aliasing
    for kw in ({"v": None}, {"f": None}, {"out": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(n=0, lam=0.0, mu=0.0, nb=need - 1) == E_SCRATCH    # (no iteration and zero factors are legal)
    assert call(V=0, v=None, f=None, out=None, status=None, s=None, nb=0) == 0                  # no vertex: success, nothing touched
    assert call(T=0, n=-1, status=None) == E_ARG                    # ... but a bad argument stays an error
    assert call(V=0, out=FAKE, status=None) == E_ARG                # ... aliasing too
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(nb=need - 1), "sls_mesh_smooth")


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for call in (lambda: mesh_ops.smooth(v, f, 1), lambda: mesh_ops.smooth(v.numpy(), f, 1), lambda: mesh_ops.vertex_adjacency(f, 6),
                 lambda: mesh_ops.vertex_adjacency(f.numpy(), 6), lambda: mesh_ops.clean_mesh(v, f, smooth=1)):
        with pytest.raises(RuntimeError, match="device tensor"):
            call()
    with pytest.raises(ValueError, match="method"):
        mesh_ops._smooth_args(1, "cotangent", "uniform", 0.5, -0.53)
    with pytest.raises(ValueError, match="weights"):
        mesh_ops._smooth_args(1, "taubin", "cotangent", 0.5, -0.53)
    for n in (-1, 1.5, True):
        with pytest.raises(ValueError, match="iterations"):
            mesh_ops._smooth_args(n, "taubin", "uniform", 0.5, -0.53)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            mesh_ops._smooth_args(1, "taubin", "uniform", bad, -0.53)
        with pytest.raises(ValueError, match="finite"):
            mesh_ops._smooth_args(1, "taubin", "uniform", 0.5, bad)
    assert mesh_ops._smooth_args(3, "taubin", "inverse_distance", 0.5, -0.53) == (3, 2, 1, 0.5, -0.53)
    assert mesh_ops._smooth_args(0, "simple", "uniform", 1, 0) == (0, 0, 0, 1.0, 0.0)
    assert mesh_ops._smooth_args(2.0, "laplacian", "uniform", 0.25, 0)[:3] == (2, 1, 0)


def test_the_table_binds_the_new_symbols():
    lib = _abi.lib()
    for name in ("sls_mesh_adjacency_scratch_bytes", "sls_mesh_adjacency", "sls_mesh_smooth_scratch_bytes", "sls_mesh_smooth"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.sls_mesh_smooth.argtypes) == 15 and len(lib.sls_mesh_adjacency.argtypes) == 10
    names = [lib.sls_timing_name(s).decode() for s in range(lib.sls_timing_slots())]
    assert names[-2:] == ["smooth_adjacency", "smooth_step"]         # appended: the slots in front keep their numbers
