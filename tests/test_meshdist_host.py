"""Host side of the point-to-mesh distance (sls_mesh_distance, sls_error_colors, splat_loam_amd/evaluation.py:
point_to_mesh, error_colors, evaluate_recon(completeness=, error_map=)): scratch sizes, every argument error (all checked
before a launch: no device needed), vertex colours in the PLY writers and readers, the refusal of malformed arguments and
of CPU tensors."""
import inspect

import numpy as np
import pytest
import torch

from splat_loam_amd import _abi, evaluation, ply_io

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
STATS_BYTES = 32768     # SLS_NN_STATS_SCRATCH_BYTES


def test_scratch_bytes_properties():
    lib = _abi.lib()
    size = lib.sls_mesh_distance_scratch_bytes
    assert size(0, 10, 10) == 0 and size(10, 0, 10) == 0 and size(10, 10, -1) == 0 and size(-1, -1, -1) == 0
    for V, F, Mq in ((1, 1, 0), (3, 1, 1), (100, 31, 64), (200, 256, 65), (300, 257, 256), (9000, 16928, 4000),
                     (600000, 1130000, 2000000), (10, 1000, 2000000)):
        n = size(V, F, Mq)
        assert n % 256 == 0 and n >= STATS_BYTES                        # sls_nn_stats can follow on the same scratch
        assert n >= lib.sls_nn_scratch_bytes(F, Mq) + 48 * F            # the search's buffers + three float4 per face
        assert n == size(V + 7, F, Mq)                                  # (the vertices are read in place)
    for V, F, Mq in ((100, 1000, 500), (100, 255, 63), (100, 256, 64)):  # monotone
        assert size(V, F, Mq) <= size(V, F, Mq + 1) and size(V, F, Mq) <= size(V, F + 1, Mq) and size(V, F, Mq) <= size(V + 1, F, Mq)


def test_mesh_distance_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_distance_scratch_bytes(100, 50, 20)

    def call(V=100, v=FAKE, F=50, f=FAKE, Mq=20, q=FAKE, d=FAKE, face=FAKE, closest=FAKE, status=FAKE, s=FAKE, n=need):
        return lib.sls_mesh_distance(V, v, F, f, Mq, q, d, face, closest, status, s, n, None)
    assert call(F=0) == E_ARG and b"F < 1" in lib.sls_last_error()
    assert call(F=-3) == E_ARG
    assert call(V=0) == E_ARG and b"V < 1" in lib.sls_last_error()
    assert call(Mq=-1) == E_ARG and b"Mq" in lib.sls_last_error()
    assert call(F=0, Mq=0) == E_ARG                                     # an empty mesh is an error even with no query
    for kw in ({"v": None}, {"f": None}, {"q": None}, {"d": None}, {"status": None}, {"s": None}, {"Mq": 0, "status": None},
               {"Mq": 0, "s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(face=None, closest=None, n=need - 1) == E_SCRATCH       # (the two optional outputs: the size check is reached)
    assert call(Mq=0, q=None, d=None, n=lib.sls_mesh_distance_scratch_bytes(100, 50, 0) - 1) == E_SCRATCH   # Mq == 0 writes the status
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_mesh_distance")


def test_error_colors_argument_errors_need_no_device():
    lib = _abi.lib()

    def call(M=10, d=FAKE, trunc=0.5, out=FAKE):
        return lib.sls_error_colors(M, d, trunc, out, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for kw in ({"d": None}, {"out": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for trunc in (0.0, -0.5, float("nan"), float("inf"), -float("inf"), 1e-60):      # (1e-60 is 0 as a float32)
        assert call(trunc=trunc) == E_ARG and b"truncation" in lib.sls_last_error(), trunc
    assert call(M=0, d=None, out=None) == 0                             # nothing to colour: success, nothing touched
    assert call(M=0, d=None, out=None, trunc=0.0) == E_ARG              # ... but the truncation is checked first


def _mesh_bytes(vertices, faces, props="xyz"):
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(vertices)
    header += "".join(f"property float {p}\n" for p in props)
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces)
    rec = np.empty(len(faces), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, faces
    return header.encode("ascii") + np.asarray(vertices, "<f4").tobytes() + rec.tobytes()


def test_ply_vertex_colours(tmp_path):
    rng = np.random.default_rng(12)
    v = rng.normal(0, 20, (211, 3)).astype(np.float32)
    n = rng.normal(0, 1, (211, 3)).astype(np.float32)
    f = rng.integers(0, 211, (97, 3)).astype(np.int32)
    rgb = rng.integers(0, 256, (211, 3)).astype(np.uint8)
    # a mesh: colours round-trip, with and without normals, from NumPy and from tensors
    ply_io.save_mesh(tmp_path / "c.ply", v, f, colors=rgb)
    v2, f2, c2 = ply_io.load_mesh(tmp_path / "c.ply", return_colors=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and c2.dtype == np.uint8 and np.array_equal(c2, rgb)
    assert len(ply_io.load_mesh(tmp_path / "c.ply")) == 2               # (the default: as ever)
    ply_io.save_mesh(tmp_path / "nc.ply", torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(rgb))
    v2, f2, c2 = ply_io.load_mesh(tmp_path / "nc.ply", return_colors=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(c2, rgb)
    p2, n2, c2 = ply_io.load_point_cloud(tmp_path / "nc.ply", return_colors=True)    # a coloured mesh is a coloured cloud too
    assert np.array_equal(p2, v) and np.array_equal(n2, n) and np.array_equal(c2, rgb)
    head = (tmp_path / "nc.ply").read_bytes().split(b"end_header\n")[0].decode()
    assert "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 97" in head
    # a cloud
    ply_io.save_point_cloud(tmp_path / "p.ply", v, n, rgb)
    p2, n2, c2 = ply_io.load_point_cloud(tmp_path / "p.ply", return_colors=True)
    assert np.array_equal(p2, v) and np.array_equal(n2, n) and np.array_equal(c2, rgb)
    assert len(ply_io.load_point_cloud(tmp_path / "p.ply")) == 2
    assert (tmp_path / "p.ply").stat().st_size == len((tmp_path / "p.ply").read_bytes().split(b"end_header\n")[0]) + 11 + 211 * 27
    # without colours: None from the readers, and the writers' bytes are what they have always been
    ply_io.save_mesh(tmp_path / "m.ply", v, f)
    assert (tmp_path / "m.ply").read_bytes() == _mesh_bytes(v, f)
    ply_io.save_mesh(tmp_path / "mn.ply", v, f, n, None)
    assert (tmp_path / "mn.ply").read_bytes() == _mesh_bytes(np.concatenate([v, n], 1), f, ("x", "y", "z", "nx", "ny", "nz"))
    ply_io.save_point_cloud(tmp_path / "q.ply", v, n)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 211\n" + "".join(f"property float {p}\n" for p in ply_io.CLOUD_PROPS)
    assert (tmp_path / "q.ply").read_bytes() == (header + "end_header\n").encode("ascii") + np.concatenate([v, n], 1).astype("<f4").tobytes()
    assert ply_io.load_mesh(tmp_path / "m.ply", return_colors=True)[2] is None
    assert ply_io.load_point_cloud(tmp_path / "q.ply", return_colors=True)[2] is None
    # float colours in the file are not uchar colours; malformed colours are refused by the writers
    rec = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "<f4"), ("green", "<f4"), ("blue", "<f4")]))
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 3\n" + "".join(f"property float {p}\n" for p in rec.dtype.names)
    (tmp_path / "fc.ply").write_bytes((header + "end_header\n").encode("ascii") + rec.tobytes())
    assert ply_io.load_point_cloud(tmp_path / "fc.ply", return_colors=True)[2] is None
    for bad in (rgb[:-1], rgb.astype(np.float32), rgb[:, :2]):
        with pytest.raises(ValueError, match="colors"):
            ply_io.save_mesh(tmp_path / "bad.ply", v, f, colors=bad)
        with pytest.raises(ValueError, match="colors"):
            ply_io.save_point_cloud(tmp_path / "bad.ply", v, n, bad)


def test_new_arguments_are_refused_where_malformed():
    pts, faces = torch.zeros((4, 3)), torch.zeros((1, 3), dtype=torch.int32)
    sig = inspect.signature(evaluation.evaluate_recon).parameters
    assert sig["completeness"].default == "sampled" and sig["error_map"].default is False
    for bad in ("Exact", "mesh", "", None, True, 1):
        with pytest.raises(ValueError, match="completeness"):
            evaluation.evaluate_recon(pts, pts, faces, completeness=bad)
    for bad in ("yes", 1, None, 0.5):
        with pytest.raises(ValueError, match="error_map"):
            evaluation.evaluate_recon(pts, pts, faces, error_map=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, "wide", None):
        with pytest.raises(ValueError, match="truncation"):
            evaluation._check_truncation(bad)
    assert evaluation._check_truncation(0.5) == 0.5 and evaluation._check_truncation(np.float32(0.1)) == float(np.float32(0.1))
    sig = inspect.signature(evaluation.point_to_mesh).parameters
    assert sig["return_face"].default is True and sig["return_closest"].default is False


def test_cpu_tensors_are_refused():
    pts, faces = torch.zeros((4, 3)), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.point_to_mesh(pts, pts, faces)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.point_to_mesh(pts.numpy(), pts, faces)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.error_colors(torch.zeros((4,)), 0.5)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.error_colors([0.0, 1.0], 0.5)
    for kw in ({"completeness": "exact"}, {"error_map": True}, {"completeness": "exact", "error_map": True}):
        with pytest.raises(RuntimeError, match="device tensor"):
            evaluation.evaluate_recon(pts, pts, faces, **kw)
