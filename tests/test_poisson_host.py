"""Host side of the Poisson volume (sls_poisson_splat, sls_poisson_solve, sls_poisson_density, splat_loam_amd/poisson.py):
the scratch sizes, every argument error (all checked before a launch: no device needed) and the refusal of CPU tensors."""
import ctypes as C

import pytest
import torch

from splat_loam_amd import _abi, meshing, poisson

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
ORIGIN = (C.c_double * 3)(0.0, 0.0, 0.0)
NAN, INF = float("nan"), float("inf")


def test_scratch_bytes():
    lib = _abi.lib()
    assert lib.sls_poisson_splat_scratch_bytes(0, 5) == 0 and lib.sls_poisson_splat_scratch_bytes(-3, 5) == 0
    assert lib.sls_poisson_splat_scratch_bytes((1 << 26) + 1, 5) == 0 and lib.sls_poisson_splat_scratch_bytes(10, (1 << 19) + 1) == 0
    assert lib.sls_poisson_splat_scratch_bytes(10, -1) == 0
    for fn in (lib.sls_poisson_solve_scratch_bytes, lib.sls_poisson_density_scratch_bytes):
        assert fn(0) == 0 and fn(-1) == 0 and fn((1 << 19) + 1) == 0
    last = 0
    for M in (1, 2, 255, 256, 257, 3000, 40_000, 1_000_000):
        n = lib.sls_poisson_splat_scratch_bytes(M, 100)
        assert n % 256 == 0 and n >= last, M
        assert n >= lib.sls_sort_scratch_bytes(M) + 16 * M + 24 * M + 2 * 4 * 512 * 100    # sorter, two key and index arrays, fractions, cells
        last = n
    last = [0, 0, 0]
    for B in (1, 2, 3, 64, 1089, 1 << 19):
        got = [lib.sls_poisson_splat_scratch_bytes(1000, B), lib.sls_poisson_solve_scratch_bytes(B), lib.sls_poisson_density_scratch_bytes(B)]
        assert all(g % 256 == 0 and g >= l for g, l in zip(got, last)), B
        assert got[1] >= 6 * 2048 * B + 24 * B + 16 * B and got[2] >= 2048 * B + 24 * B
        last = got


def test_splat_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_poisson_splat_scratch_bytes(100, 5)

    def call(M=100, p=FAKE, nrm=FAKE, B=5, blocks=FAKE, vs=0.1, o=ORIGIN, out=FAKE, status=FAKE, s=FAKE, n=need):
        return lib.sls_poisson_splat(M, p, nrm, B, blocks, vs, o, out, status, s, n, None)
    assert call(M=-1) == E_ARG and b"M negative" in lib.sls_last_error()
    assert call(M=(1 << 26) + 1) == E_ARG
    assert call(B=-1) == E_ARG and b"B negative" in lib.sls_last_error()
    assert call(B=(1 << 19) + 1) == E_ARG
    for vs in (0.0, -0.1, NAN, INF):
        assert call(vs=vs) == E_ARG and b"voxel_size" in lib.sls_last_error(), vs
        assert call(M=0, vs=vs, status=None) == E_ARG                       # a bad grid is an error for an empty cloud too
    assert call(o=None) == E_ARG and b"origin3" in lib.sls_last_error()
    assert call(o=(C.c_double * 3)(0.0, NAN, 0.0)) == E_ARG
    for kw in ({"p": None}, {"nrm": None}, {"blocks": None}, {"out": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(M=0, p=None, nrm=None, blocks=None, out=None, status=None, s=None, n=0) == 0    # an empty cloud: nothing touched
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_poisson_splat")


def test_solve_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_poisson_solve_scratch_bytes(5)

    def call(B=5, blocks=FAKE, field=FAKE, alpha=4.0, it=300, tol=1e-4, chi=FAKE, status=FAKE, s=FAKE, n=need):
        return lib.sls_poisson_solve(B, blocks, field, alpha, it, tol, chi, status, s, n, None)
    assert call(B=-1) == E_ARG and b"B negative" in lib.sls_last_error()
    assert call(B=(1 << 19) + 1) == E_ARG
    for alpha in (0.0, -1.0, NAN, INF):
        assert call(alpha=alpha) == E_ARG and b"alpha" in lib.sls_last_error(), alpha
    for tol in (NAN, -1e-4, INF):
        assert call(tol=tol) == E_ARG and b"tol" in lib.sls_last_error(), tol
    for it in (-1, 1001):
        assert call(it=it) == E_ARG and b"iterations" in lib.sls_last_error(), it
    for kw in ({"blocks": None}, {"field": None}, {"chi": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(B=0, status=None) == E_ARG                                   # the status has to go somewhere
    assert call(B=0, alpha=0.0) == E_ARG                                     # a bad screening stays an error without blocks
    for off in (1, 16, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()


def test_density_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_poisson_density_scratch_bytes(5)

    def call(B=5, blocks=FAKE, field=FAKE, sweeps=2, out=FAKE, s=FAKE, n=need):
        return lib.sls_poisson_density(B, blocks, field, sweeps, out, s, n, None)
    assert call(B=-1) == E_ARG and call(B=(1 << 19) + 1) == E_ARG
    for sweeps in (-1, 65):
        assert call(sweeps=sweeps) == E_ARG and b"sweeps" in lib.sls_last_error()
    for kw in ({"blocks": None}, {"field": None}, {"out": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(s=FAKE + 8) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH
    assert call(B=0, blocks=None, field=None, out=None, s=None, n=0) == 0    # no block: success, nothing launched
    assert call(B=0, sweeps=-1) == E_ARG


def test_poisson_refuses_cpu_tensors():
    pts = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        poisson.PoissonVolume(torch.zeros((2, 3), dtype=torch.int32), 0.1)
    with pytest.raises(RuntimeError, match="device tensor"):
        poisson.reconstruct(pts, pts, 0.1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        meshing.mesh_poisson("nowhere", 0.1, device="cpu")
    with pytest.raises(ValueError, match="not both"):
        meshing.mesh_poisson("nowhere", 0.1, min_density=1.0, min_density_quantile=0.1)
