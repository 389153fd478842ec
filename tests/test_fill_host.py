"""Host side of the hole-filling stage (sls_mesh_boundary_loops, sls_mesh_fill_holes, mesh_ops.boundary_loops,
mesh_ops.fill_holes): the scratch sizes, every argument error (all checked before a launch: no device needed), the refusal of
CPU tensors and bad arguments, and the bindings of the new symbols."""
import math

import pytest
import torch

from splat_loam_amd import _abi, mesh_ops

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
OTHER = 0x20000
THIRD = 0x30000
MAX_T = 1 << 29         # SLS_MESH_MAX_TRIANGLES
MAX_V = 3 * MAX_T       # SLS_MESH_MAX_VERTICES
SIZES = (1, 2, 255, 2047, 2048, 2049, 3000, 40_000, 1_000_000)


@pytest.mark.parametrize("name", ("sls_mesh_boundary_loops_scratch_bytes", "sls_mesh_fill_holes_scratch_bytes"))
def test_scratch_bytes(name):
    fn = getattr(_abi.lib(), name)
    assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(-1, 5) == 0 and fn(5, -1) == 0
    assert fn(5, MAX_T + 1) == 0 and fn(MAX_V + 1, 5) == 0 and fn(MAX_V, MAX_T) > 0
    for a in SIZES:
        assert fn(a, 100) % 256 == 0 and fn(100, a) % 256 == 0 and fn(a, a) > 0
    for lo, hi in zip(SIZES, SIZES[1:]):                            # monotone in each argument
        assert fn(lo, 100) <= fn(hi, 100) and fn(100, lo) <= fn(100, hi) and fn(lo, lo) <= fn(hi, hi)
    for n in SIZES:                                                 # two copies of the 3 T pairs of u32, the half-edges, and the sorter's own scratch
        assert fn(n, n) >= _abi.lib().sls_sort_scratch_bytes(3 * n) + 2 * 8 * 3 * n + 8 * 3 * n + 3 * 4 * n


def test_boundary_loops_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_boundary_loops_scratch_bytes(60, 100)

    def call(V=60, T=100, f=FAKE, counts=None, he=FAKE, loop=FAKE, edges=FAKE, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_boundary_loops(V, T, f, counts, he, loop, edges, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG and b"SLS_MESH_MAX_VERTICES" in lib.sls_last_error()
    for kw in ({"f": None}, {"he": None}, {"loop": None}, {"edges": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(V=0, f=None, he=None, loop=None, edges=None, status=None, s=None, nb=0) == 0        # no vertex, no status: nothing to write
    assert call(T=0, f=None, he=None, loop=None, edges=None, status=None, s=None, nb=0) == 0


def test_fill_holes_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_fill_holes_scratch_bytes(60, 100)

    def call(V=60, v=FAKE, T=100, f=OTHER, counts=None, edges=64, size=0.0, cap_v=80, out_v=THIRD, cap_t=150, out_f=THIRD + 0x10000,
             status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_fill_holes(V, v, T, f, counts, edges, size, cap_v, out_v, cap_t, out_f, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1, cap_t=MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1, cap_v=MAX_V + 1) == E_ARG and b"SLS_MESH_MAX_VERTICES" in lib.sls_last_error()
    for edges in (2, 0, -1):
        assert call(edges=edges) == E_ARG and b"max_edges" in lib.sls_last_error(), edges
    for bad in (math.inf, -math.inf, math.nan, -1.0, -1e-300):
        assert call(size=bad) == E_ARG and b"max_size" in lib.sls_last_error(), bad
    assert call(cap_v=59) == E_ARG and b"cap_vertices" in lib.sls_last_error()
    assert call(cap_t=99) == E_ARG and b"cap_triangles" in lib.sls_last_error()
    assert call(cap_v=MAX_V + 1) == E_ARG and b"cap_vertices" in lib.sls_last_error()
    assert call(cap_t=MAX_T + 1) == E_ARG and b"cap_triangles" in lib.sls_last_error()
    assert call(out_v=FAKE) == E_ARG and b"must not be vertices" in lib.sls_last_error()          # no aliasing
    assert call(out_f=OTHER) == E_ARG and b"must not be faces" in lib.sls_last_error()
    for kw in ({"v": None}, {"f": None}, {"out_v": None}, {"out_f": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(edges=3, size=1e-300, cap_v=60, cap_t=100, nb=need - 1) == E_SCRATCH      # (the smallest legal values are legal)
    assert call(V=0, v=None, T=0, f=None, cap_v=0, out_v=None, cap_t=0, out_f=None, status=None, s=None, nb=0) == 0    # nothing: success, nothing touched
    assert call(T=0, edges=2, status=None) == E_ARG                 # ... but a bad argument stays an error
    assert call(V=0, cap_v=0, v=None, out_v=None, out_f=None) == E_ARG and b"null pointer" in lib.sls_last_error()     # T > 0: the faces are copied
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(nb=need - 1), "sls_mesh_fill_holes")


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for call in (lambda: mesh_ops.fill_holes(v, f), lambda: mesh_ops.fill_holes(v.numpy(), f), lambda: mesh_ops.boundary_loops(f, 6),
                 lambda: mesh_ops.boundary_loops(f.numpy(), 6), lambda: mesh_ops.clean_mesh(v, f, fill_holes=64)):
        with pytest.raises(RuntimeError, match="device tensor"):
            call()
    for n in (2, -1, 3.5, True):
        with pytest.raises(ValueError, match="max_edges"):
            mesh_ops._fill_args(n, None, 0.25)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="max_size"):
            mesh_ops._fill_args(64, bad, 0.25)
        with pytest.raises(ValueError, match="capacity"):
            mesh_ops._fill_args(64, None, bad)
    assert mesh_ops._fill_args(64, None, 0.25) == (64, 0.0, 0.25) and mesh_ops._fill_args(3.0, 2, 0) == (3, 2.0, 0.0)
    # the room: max(ceil(capacity T), 64) new triangles, and a vertex for every four of them, plus one
    assert mesh_ops._fill_room(100, 1000, 0.25) == (100 + 250 // 4 + 1, 1250) and mesh_ops._fill_room(10, 20, 0.25) == (10 + 16 + 1, 84)
    assert mesh_ops._fill_room(0, 0, 0.25) == (17, 64) and mesh_ops._fill_room(7, 1001, 0.1) == (7 + 101 // 4 + 1, 1001 + 101)
    with pytest.raises(ValueError, match="123 triangles and 45 vertices"):
        mesh_ops._fill_errors([0] * 12 + [45, 123, 1, 1])
    mesh_ops._fill_errors([0] * 12 + [45, 123, 0, 1])


def test_the_table_binds_the_new_symbols():
    lib = _abi.lib()
    for name in ("sls_mesh_boundary_loops_scratch_bytes", "sls_mesh_boundary_loops", "sls_mesh_fill_holes_scratch_bytes", "sls_mesh_fill_holes"):
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.sls_mesh_boundary_loops.argtypes) == 11 and len(lib.sls_mesh_fill_holes.argtypes) == 15
    assert len(mesh_ops.FILL_STATUS) == 15
