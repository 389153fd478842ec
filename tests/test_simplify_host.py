"""Host side of the simplification stage (sls_mesh_simplify, mesh_ops.simplify_vertex_clustering): the scratch sizes, every
argument error (all checked before a launch: no device needed), and the refusal of CPU tensors and bad arguments."""
import math

import pytest
import torch

from splat_loam_amd import _abi, mesh_ops

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
MAX_T = 1 << 29         # SLS_MESH_MAX_TRIANGLES
MAX_V = 3 * MAX_T       # SLS_MESH_MAX_VERTICES
SIZES = (1, 2, 255, 2047, 2048, 2049, 3000, 40_000, 1_000_000)


def test_scratch_bytes():
    fn = _abi.lib().sls_mesh_simplify_scratch_bytes
    assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(-1, 5) == 0 and fn(5, -1) == 0
    assert fn(5, MAX_T + 1) == 0 and fn(MAX_V + 1, 5) == 0 and fn(MAX_V, MAX_T) > 0
    for a in SIZES:
        assert fn(a, 100) % 256 == 0 and fn(100, a) % 256 == 0 and fn(a, a) > 0
    for lo, hi in zip(SIZES, SIZES[1:]):                            # monotone in each argument
        assert fn(lo, 100) <= fn(hi, 100) and fn(100, lo) <= fn(100, hi) and fn(lo, lo) <= fn(hi, hi)
    for n in SIZES:                                                 # the three sorts' pairs and the sorter's own scratch
        assert fn(n, n) >= _abi.lib().sls_sort_scratch_bytes(3 * n) + 24 * n + 24 * n + 48 * n


def test_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_simplify_scratch_bytes(60, 100)

    def call(V=60, v=FAKE, T=100, f=FAKE, h=0.5, how=1, lam=1e-3, ov=FAKE, of=FAKE, vmap=FAKE, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_simplify(V, v, T, f, h, how, lam, ov, of, vmap, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG and b"SLS_MESH_MAX_VERTICES" in lib.sls_last_error()
    for h in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert call(h=h) == E_ARG and b"voxel_size" in lib.sls_last_error(), h
    for how in (-1, 2, 7):
        assert call(how=how) == E_ARG and b"contraction" in lib.sls_last_error(), how
    for lam in (-1e-9, math.inf, math.nan):
        assert call(lam=lam) == E_ARG and b"regularisation" in lib.sls_last_error(), lam
    assert call(lam=0.0, nb=need - 1) == E_SCRATCH                  # (0 is a legal regularisation)
    for kw in ({"v": None}, {"f": None}, {"ov": None}, {"of": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(vmap=None, nb=need - 1) == E_SCRATCH                # (the vertex map is optional)
    for kw in ({"T": 0}, {"V": 0}):                                 # an empty mesh: success, nothing touched without a status or a map
        assert call(v=None, f=None, ov=None, of=None, vmap=None, status=None, s=None, nb=0, **kw) == 0
    assert call(T=0, h=0.0, status=None, vmap=None) == E_ARG        # ... but a bad argument stays an error
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(nb=need - 1), "sls_mesh_simplify")


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for call in (lambda: mesh_ops.simplify_vertex_clustering(v, f, 0.5), lambda: mesh_ops.simplify_vertex_clustering(v.numpy(), f, 0.5),
                 lambda: mesh_ops.clean_mesh(v, f, simplify=0.5)):
        with pytest.raises(RuntimeError, match="device tensor"):
            call()
    with pytest.raises(ValueError, match="contraction"):
        mesh_ops._simplify_args(0.5, "median", 1e-3)
    for h in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            mesh_ops._simplify_args(h, "average", 1e-3)
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="regularisation"):
            mesh_ops._simplify_args(0.5, "quadric", lam)
    assert mesh_ops._simplify_args(0.5, "quadric", 0) == (0.5, 1, 0.0) and mesh_ops._simplify_args(2, "average", 1e-3) == (2.0, 0, 1e-3)
