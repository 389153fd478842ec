"""Host side of the signed distance (sls_mesh_pseudonormals, sls_mesh_signed_distance, sls_signed_stats,
sls_signed_error_colors; splat_loam_amd/evaluation.py: mesh_pseudonormals, signed_distance, signed_error_colors,
evaluate_recon(signed=)): the scratch sizes, every argument error (all checked before a launch: no device needed), the
refusal of malformed arguments and of CPU tensors."""
import inspect
import math

import pytest
import torch

from splat_loam_amd import _abi, evaluation

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
STATS_BYTES = 32768     # SLS_NN_STATS_SCRATCH_BYTES


def test_scratch_size_properties():
    lib = _abi.lib()
    size = lib.sls_mesh_pseudonormals_scratch_bytes
    assert size(0, 10) == 0 and size(10, 0) == 0 and size(-1, -1) == 0 and size(10, 2**29 + 1) == 0
    for V, F in ((1, 1), (3, 1), (100, 31), (200, 256), (300, 257), (9000, 16928), (103041, 204800), (600000, 1130000)):
        n = size(V, F)
        assert n % 256 == 0
        # per corner: the float64 normal and angle, the u64 edge key and its copy, the corner id and its copy; then the
        # corner-by-vertex sort of the vertex normals
        assert n >= 3 * F * (8 + 8 + 8 + 8 + 4 + 4) + lib.sls_mesh_vertex_normals_scratch_bytes(V, F)
        assert n <= size(V, F + 1)
    size = lib.sls_mesh_signed_distance_scratch_bytes
    assert size(0, 10, 5) == 0 and size(10, 0, 5) == 0 and size(10, 10, -1) == 0
    for V, F, M in ((1, 1, 0), (3, 1, 1), (100, 31, 65), (9000, 16928, 20000), (600000, 1130000, 2000000)):
        n = size(V, F, M)
        assert n % 256 == 0 and n >= lib.sls_mesh_distance_scratch_bytes(V, F, M) + 8 * M
        assert n >= STATS_BYTES                                         # sls_signed_stats can follow on the same scratch
        assert n <= size(V, F, M + 1) and n <= size(V, F + 1, M)


def test_pseudonormals_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_pseudonormals_scratch_bytes(100, 50)

    def call(V=100, v=FAKE, F=50, f=FAKE, fn=FAKE, en=FAKE, vn=FAKE, status=FAKE, scratch=FAKE, n=need):
        return lib.sls_mesh_pseudonormals(V, v, F, f, fn, en, vn, status, scratch, n, None)
    assert call(F=0) == E_ARG and b"F < 1" in lib.sls_last_error()
    assert call(F=-3) == E_ARG and call(F=2**29 + 1) == E_ARG
    assert call(V=0) == E_ARG and b"V < 1" in lib.sls_last_error()
    for kw in ({"v": None}, {"f": None}, {"fn": None}, {"en": None}, {"vn": None}, {"status": None}, {"scratch": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(scratch=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_mesh_pseudonormals")


def test_signed_distance_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_signed_distance_scratch_bytes(100, 50, 20)

    def call(V=100, v=FAKE, F=50, f=FAKE, fn=FAKE, en=FAKE, vn=FAKE, M=20, q=FAKE, sd=FAKE, face=FAKE, closest=FAKE, feature=FAKE,
             status=FAKE, scratch=FAKE, n=need):
        return lib.sls_mesh_signed_distance(V, v, F, f, fn, en, vn, M, q, sd, face, closest, feature, status, scratch, n, None)
    assert call(F=0) == E_ARG and b"F < 1" in lib.sls_last_error()
    assert call(V=0) == E_ARG and b"V < 1" in lib.sls_last_error()
    assert call(M=-1) == E_ARG and b"Mq" in lib.sls_last_error()
    assert call(F=0, M=0) == E_ARG                                      # an empty mesh is an error even with no query
    for kw in ({"v": None}, {"f": None}, {"fn": None}, {"en": None}, {"vn": None}, {"q": None}, {"sd": None}, {"status": None},
               {"scratch": None}, {"M": 0, "status": None}, {"M": 0, "vn": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(scratch=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(face=None, closest=None, feature=None, n=need - 1) == E_SCRATCH     # the optional outputs: the size check is reached
    assert call(M=0, q=None, sd=None, n=lib.sls_mesh_signed_distance_scratch_bytes(100, 50, 0) - 1) == E_SCRATCH


def test_signed_stats_and_colours_argument_errors_need_no_device():
    lib = _abi.lib()

    def stats(M=10, sd=FAKE, trunc=0.5, out=FAKE, scratch=FAKE, n=STATS_BYTES):
        return lib.sls_signed_stats(M, sd, trunc, out, scratch, n, None)
    assert stats(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for kw in ({"sd": None}, {"out": None}, {"scratch": None}, {"M": 0, "out": None}):
        assert stats(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert stats(trunc=float("nan")) == E_ARG and b"NaN" in lib.sls_last_error()
    assert stats(scratch=FAKE + 64) == E_ARG and b"aligned" in lib.sls_last_error()
    assert stats(n=STATS_BYTES - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert stats(M=0, sd=None, n=STATS_BYTES - 1) == E_SCRATCH          # M == 0 still writes its four words

    def colors(M=10, sd=FAKE, trunc=0.5, rgb=FAKE):
        return lib.sls_signed_error_colors(M, sd, trunc, rgb, None)
    assert colors(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for kw in ({"sd": None}, {"rgb": None}):
        assert colors(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for trunc in (0.0, -1.0, float("nan"), math.inf):
        assert colors(trunc=trunc) == E_ARG and b"truncation" in lib.sls_last_error(), trunc
    assert colors(M=0, sd=None, rgb=None) == 0                          # nothing to do, nothing launched


def test_python_refuses_cpu_tensors_and_bad_arguments():
    p = torch.zeros((4, 3))
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.signed_distance(p, v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.mesh_pseudonormals(v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.signed_error_colors(torch.zeros(4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.evaluate_recon(p, v, f, signed=True)
    for bad in (1, 0, "yes", None):                                     # refused before anything touches a tensor
        with pytest.raises(ValueError, match="signed must be True or False"):
            evaluation.evaluate_recon(p, v, f, signed=bad)
    with pytest.raises(TypeError, match="mesh_pseudonormals"):
        evaluation._use_pseudonormals(object(), v, f)
    pn = evaluation.MeshPseudoNormals(v, f, None, None, None, None)
    assert evaluation._use_pseudonormals(pn, v, f) is pn
    with pytest.raises(ValueError, match="another mesh"):
        evaluation._use_pseudonormals(pn, torch.zeros((4, 3)), f)
    with pytest.raises(ValueError, match="another mesh"):
        evaluation._use_pseudonormals(pn, v, torch.zeros((2, 3), dtype=torch.int32))
    # the status words: counts are details, the two kinds of bad face are errors with point_to_mesh's messages
    assert evaluation._pseudonormals_status([1, 0, 0, 2, 3, 4, 5, 1], "x") == {
        "degenerate_faces": 1, "zero_area_faces": 2, "boundary_edges": 3, "nonmanifold_edges": 4, "inconsistent_edges": 5}
    with pytest.raises(ValueError, match="x: 2 faces have a vertex index outside the vertices"):
        evaluation._pseudonormals_status([3, 2, 0, 0, 0, 0, 0, 1], "x")
    with pytest.raises(ValueError, match="x: 1 faces have a vertex with a non-finite coordinate"):
        evaluation._pseudonormals_status([0, 0, 1, 0, 0, 0, 0, 1], "x")


def test_signatures():
    sig = inspect.signature(evaluation.signed_distance)
    assert list(sig.parameters) == ["points", "vertices", "faces", "return_face", "return_closest", "return_feature", "pseudonormals"]
    assert all(sig.parameters[k].default is False for k in ("return_face", "return_closest", "return_feature"))
    assert sig.parameters["pseudonormals"].default is None
    assert list(inspect.signature(evaluation.mesh_pseudonormals).parameters) == ["vertices", "faces", "return_details"]
    assert inspect.signature(evaluation.evaluate_recon).parameters["signed"].default is False
    assert "not a signed distance" not in evaluation.point_to_mesh.__doc__.lower()
    assert "signed distance" not in evaluation.cast_rays.__doc__.lower()
