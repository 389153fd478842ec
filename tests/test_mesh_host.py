"""Host side of the mesh cleaning stage (sls_mesh_weld, sls_mesh_clusters, sls_mesh_filter, sls_mesh_vertex_normals,
splat_loam_amd/mesh_ops.py): the scratch sizes, every argument error (all checked before a launch: no device needed), the
PLY writer with normals against the readers, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from splat_loam_amd import _abi, mesh_ops, ply_io

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
MAX_T = 1 << 29         # SLS_MESH_MAX_TRIANGLES
MAX_V = 3 * MAX_T       # SLS_MESH_MAX_VERTICES
SIZES = (1, 2, 255, 2047, 2048, 2049, 3000, 40_000, 1_000_000)


def test_scratch_bytes():
    lib = _abi.lib()
    for fn in (lib.sls_mesh_weld_scratch_bytes, lib.sls_mesh_clusters_scratch_bytes):
        assert fn(0) == 0 and fn(-3) == 0
        last = 0
        for n in SIZES:
            assert fn(n) % 256 == 0 and fn(n) >= last, n
            last = fn(n)
    assert lib.sls_mesh_weld_scratch_bytes(3 * MAX_T) > 0 and lib.sls_mesh_clusters_scratch_bytes(MAX_T + 1) == 0
    for n in SIZES:
        assert lib.sls_mesh_weld_scratch_bytes(n) >= lib.sls_sort_scratch_bytes(n) + 16 * n          # two key and two row arrays
        assert lib.sls_mesh_clusters_scratch_bytes(n) >= lib.sls_sort_scratch_bytes(3 * n) + 24 * 3 * n + 12 * n
    for fn in (lib.sls_mesh_filter_scratch_bytes, lib.sls_mesh_vertex_normals_scratch_bytes):
        assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(-1, 5) == 0 and fn(5, -1) == 0
        assert fn(5, MAX_T + 1) == 0 and fn(MAX_V + 1, 5) == 0
        for a in SIZES:                             # monotone in each argument
            assert fn(a, 100) % 256 == 0 and fn(100, a) % 256 == 0
        for lo, hi in zip(SIZES, SIZES[1:]):
            assert fn(lo, 100) <= fn(hi, 100) and fn(100, lo) <= fn(100, hi) and fn(lo, lo) <= fn(hi, hi)


def test_weld_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_weld_scratch_bytes(300)

    def call(n=300, soup=FAKE, out=FAKE, index=FAKE, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_weld(n, soup, out, index, status, s, nb, None)
    assert call(n=-1) == E_ARG and b"n_rows negative" in lib.sls_last_error()
    assert call(n=3 * MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    for kw in ({"soup": None}, {"out": None}, {"index": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(n=0, soup=None, out=None, index=None, status=None, s=None, nb=0) == 0       # no rows: success, nothing touched
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(nb=need - 1), "sls_mesh_weld")


def test_clusters_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_clusters_scratch_bytes(100)

    def call(T=100, faces=FAKE, V=60, labels=FAKE, counts=FAKE, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_clusters(T, faces, V, labels, counts, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG and b"SLS_MESH_MAX_TRIANGLES" in lib.sls_last_error()
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG
    for kw in ({"faces": None}, {"labels": None}, {"counts": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(s=FAKE + 64) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(V=0, nb=need - 1) == E_SCRATCH                  # (V = 0 is legal: every triangle is out of range)
    assert call(T=0, faces=None, labels=None, counts=None, status=None, s=None, nb=0) == 0
    assert call(T=0, V=-1, status=None) == E_ARG                # ... but a bad size stays an error


def test_filter_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_filter_scratch_bytes(60, 100)

    def call(V=60, v=FAKE, T=100, f=FAKE, labels=FAKE, counts=FAKE, cs=FAKE, keep=1, floor=50, ov=FAKE, of=FAKE, vmap=FAKE,
             status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_filter(V, v, T, f, labels, counts, cs, keep, floor, ov, of, vmap, status, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG
    for kw in ({"v": None}, {"f": None}, {"labels": None}, {"counts": None}, {"cs": None}, {"ov": None}, {"of": None}, {"status": None},
               {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(s=FAKE + 1) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(vmap=None, nb=need - 1) == E_SCRATCH            # (the vertex map is optional)
    for kw in ({"T": 0}, {"V": 0}):                             # an empty mesh: success, nothing touched without a status
        assert call(v=None, f=None, labels=None, counts=None, cs=None, ov=None, of=None, vmap=None, status=None, s=None, nb=0, **kw) == 0


def test_vertex_normals_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_vertex_normals_scratch_bytes(60, 100)

    def call(V=60, v=FAKE, T=100, f=FAKE, out=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_vertex_normals(V, v, T, f, out, s, nb, None)
    assert call(T=-1) == E_ARG and b"T negative" in lib.sls_last_error()
    assert call(T=MAX_T + 1) == E_ARG
    assert call(V=-1) == E_ARG and b"V negative" in lib.sls_last_error()
    assert call(V=MAX_V + 1) == E_ARG
    for kw in ({"v": None}, {"f": None}, {"out": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(T=0, f=None, s=None, out=None) == E_ARG         # the zeros have to go somewhere
    assert call(s=FAKE + 128) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(V=0, v=None, f=None, out=None, s=None, nb=0) == 0               # no vertex: success, nothing launched


def test_save_mesh_with_normals_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    v = rng.normal(0, 10, (50, 3)).astype(np.float32)
    n = rng.normal(0, 1, (50, 3)).astype(np.float32)
    n[0] = [-0.0, np.float32(1e-40), 0.0]                       # bits, not values
    f = rng.integers(0, 50, (120, 3)).astype(np.int32)
    ply_io.save_mesh(tmp_path / "n.ply", v, f, normals=n)
    v2, f2 = ply_io.load_mesh(tmp_path / "n.ply")
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
    p3, n3 = ply_io.load_point_cloud(tmp_path / "n.ply")
    assert np.array_equal(p3.view(np.uint32), v.view(np.uint32)) and np.array_equal(n3.view(np.uint32), n.view(np.uint32))
    ply_io.save_mesh(tmp_path / "t.ply", torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n))
    assert (tmp_path / "t.ply").read_bytes() == (tmp_path / "n.ply").read_bytes()
    ply_io.save_mesh(tmp_path / "plain.ply", v, f)              # without normals: the bytes of the three-property layout
    ply_io.save_mesh(tmp_path / "none.ply", v, f, normals=None)
    blob = (tmp_path / "plain.ply").read_bytes()
    assert blob == (tmp_path / "none.ply").read_bytes() and b"nx" not in blob[:blob.index(b"end_header")]
    assert len(blob) == blob.index(b"end_header\n") + 11 + 50 * 12 + 120 * 13
    with pytest.raises(ValueError, match="same number of rows"):
        ply_io.save_mesh(tmp_path / "bad.ply", v, f, normals=n[:10])


def test_mesh_ops_refuse_cpu_tensors_and_bad_shapes():
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for call in (lambda: mesh_ops.weld(v), lambda: mesh_ops.weld(v.numpy()), lambda: mesh_ops.cluster_triangles(f, 6),
                 lambda: mesh_ops.keep_clusters(v, f), lambda: mesh_ops.vertex_normals(v, f), lambda: mesh_ops.clean_mesh(v, f)):
        with pytest.raises(RuntimeError, match="device tensor"):
            call()
