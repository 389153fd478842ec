"""Host side of the voxel down-sampling and of the mesh sampling (sls_voxel_downsample, sls_mesh_sample,
splat_loam_amd/evaluation.py): scratch sizes, every argument error (all checked before a launch: no device needed), the
mesh PLY reader, the refusal of CPU tensors, the NumPy restatements (cloud_ref.py) against independent implementations,
and include/sls_cloud_math.h compiled as plain C against the restatement, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cloud_ref
from splat_loam_amd import _abi, evaluation, ply_io

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_bytes():
    lib = _abi.lib()
    assert lib.sls_voxel_scratch_bytes(0) == 0 and lib.sls_voxel_scratch_bytes(-3) == 0
    last = 0
    for M in (1, 2, 63, 64, 65, 1023, 1024, 1025, 6000, 13340, 2_000_000, 10_000_000):
        n = lib.sls_voxel_scratch_bytes(M)
        assert n % 256 == 0 and n >= last, M                              # monotonic
        assert n >= lib.sls_sort_scratch_bytes(M)                         # the sorter runs over the whole cloud
        assert n >= lib.sls_sort_scratch_bytes(M) + 28 * M                # ... + two key and two index arrays, the segment starts
        last = n
    for bad in ((-1, 5, 5), (5, -1, 5), (5, 5, -1)):
        assert lib.sls_mesh_sample_scratch_bytes(*bad) == 0
    assert lib.sls_mesh_sample_scratch_bytes(0, 0, 0) % 256 == 0
    last = 0
    for F in (0, 1, 2, 128, 1023, 1024, 1025, 1_000_000):
        n = lib.sls_mesh_sample_scratch_bytes(3 * F, F, 1000)
        assert n % 256 == 0 and n >= last and n >= 16 * F                 # a float64 area and a 64-bit prefix per face
        assert lib.sls_mesh_sample_scratch_bytes(3 * F + 7, F, 1000) >= n   # monotonic in V and in n_samples too
        assert lib.sls_mesh_sample_scratch_bytes(3 * F, F, 10_000_000) >= n
        last = n


def test_voxel_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_voxel_scratch_bytes(100)

    def call(M=100, p=FAKE, vs=0.02, out=FAKE, cnt=FAKE, status=FAKE, s=FAKE, n=need):
        return lib.sls_voxel_downsample(M, p, vs, out, cnt, status, s, n, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for vs in (0.0, -0.02, float("nan"), float("inf"), -float("inf")):
        assert call(vs=vs) == E_ARG and b"voxel_size" in lib.sls_last_error(), vs
        assert call(M=0, vs=vs, status=None) == E_ARG                      # a bad voxel size is an error for an empty cloud too
    for kw in ({"p": None}, {"out": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(cnt=None, n=need - 1) == E_SCRATCH                        # (null counts are legal: the size check is reached)
    assert call(M=0, p=None, out=None, cnt=None, status=None, s=None, n=0) == 0     # an empty cloud: success, nothing touched
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_voxel_downsample")


def test_mesh_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_mesh_sample_scratch_bytes(30, 10, 50)

    def call(V=30, v=FAKE, F=10, f=FAKE, box=FAKE, n=50, seed=1, out=FAKE, face=FAKE, status=FAKE, s=FAKE, nb=need):
        return lib.sls_mesh_sample(V, v, F, f, box, n, seed, out, face, status, s, nb, None)
    assert call(V=-1) == E_ARG and b"negative V or F" in lib.sls_last_error()
    assert call(F=-1) == E_ARG and b"negative V or F" in lib.sls_last_error()
    assert call(n=-1) == E_ARG and b"n_samples" in lib.sls_last_error()
    for kw in ({"v": None}, {"f": None}, {"out": None}, {"status": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 8, 64, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(nb=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(nb=0) == E_SCRATCH
    assert call(box=None, face=None, nb=need - 1) == E_SCRATCH            # (both optional: the size check is reached)
    assert call(n=0, v=None, f=None, box=None, out=None, face=None, status=None, s=None, nb=0) == 0    # no sample: success
    assert call(n=0, V=-1) == E_ARG                                       # ... but a bad size stays an error


def test_voxel_restatement_against_a_dictionary_of_lists():
    rng = np.random.default_rng(11)
    for vs, pts in ((0.3, rng.normal(0, 2, (3000, 3))), (0.125, rng.integers(-64, 65, (2000, 3)) / 16.0),
                    (1.0, -np.abs(rng.normal(0, 5, (500, 3))) - 3.0), (200.0, rng.uniform(-45, 45, (300, 3)))):      # (extent < size / 2: one voxel)
        pts = pts.astype(np.float32)
        rows, counts = cloud_ref.voxel_down_sample(pts, vs)
        mn = [min(float(p[a]) for p in pts) for a in range(3)]
        cells = {}
        for p in pts:
            idx = tuple(int(np.floor((float(p[a]) - (mn[a] - 0.5 * vs)) / vs)) for a in range(3))
            cells.setdefault(idx, []).append(p)
        order = sorted(cells, key=lambda i: i[0] | (i[1] << 21) | (i[2] << 42))
        assert len(order) == len(rows) and counts.sum() == len(pts)
        for row, count, idx in zip(rows, counts, order):
            mean = [np.float32(sum(float(p[a]) for p in cells[idx]) / len(cells[idx])) for a in range(3)]
            assert count == len(cells[idx]) and row.tolist() == mean
    assert len(cloud_ref.voxel_down_sample(pts, 200.0)[0]) == 1
    assert cloud_ref.voxel_down_sample(np.zeros((0, 3)), 1.0)[0].shape == (0, 3)
    with pytest.raises(ValueError, match="non-finite"):
        cloud_ref.voxel_down_sample(np.array([[0, 0, 0], [1, np.nan, 0]], np.float32), 1.0)
    with pytest.raises(ValueError, match="2\\^21"):
        cloud_ref.voxel_down_sample(np.array([[0, 0, 0], [64, 0, 0]], np.float32), 2.0 ** -16)
    assert len(cloud_ref.voxel_down_sample(np.array([[0, 0, 0], [31.9, 0, 0]], np.float32), 2.0 ** -16)[0]) == 2


def test_mesh_weights_against_a_direct_area():
    vertices, faces, zero = cloud_ref.grid_mesh()
    assert len(faces) == 128
    w, n_bad = cloud_ref.mesh_weights(vertices, faces)
    v = vertices.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1)
    assert n_bad == 0 and np.all(w[zero] == 0) and np.all(np.delete(w, zero) > 0) and w.max() == 1 << 32
    assert np.abs(w.astype(np.float64) / 2.0 ** 32 - area / area.max()).max() <= 2.0 ** -31
    assert np.array_equal(w[[9, 10]], w[[60, 60]])
    # a crop box: a vertex exactly on the box face is inside; a face with one vertex outside is dropped
    box = np.array([-4, -4, -1, 0, 4, 1], np.float32)
    wc, _ = cloud_ref.mesh_weights(vertices, faces, box)
    inside = (vertices[faces][:, :, 0] <= 0).all(1)
    assert np.array_equal(wc > 0, inside & (w > 0)) and 0 < (wc > 0).sum() < (w > 0).sum()
    assert (vertices[faces[wc > 0]][:, :, 0] == 0).any()                       # faces that touch the box face were kept
    # bad indices and NaN vertices
    bad = faces.copy()
    bad[3, 0], bad[17, 2] = -1, len(vertices)
    assert cloud_ref.mesh_weights(vertices, bad)[1] == 2 and cloud_ref.mesh_weights(vertices, bad)[0][[3, 17]].tolist() == [0, 0]
    nanv = vertices.copy()
    nanv[0] = np.nan
    wn, _ = cloud_ref.mesh_weights(nanv, faces)
    assert np.all(wn[(faces == 0).any(1)] == 0) and wn.max() == 1 << 32
    with pytest.raises(ValueError, match="no area"):
        cloud_ref.sample_mesh(vertices, faces[zero], 10)
    with pytest.raises(ValueError, match="index"):
        cloud_ref.sample_mesh(vertices, bad, 10)


def test_restatement_draws_in_proportion_to_area():
    """Two triangles of areas 1 : 3: the share of the small one within five sigma of 0.25 (sigma = sqrt(.25 .75 / n) =
    0.00097 at n = 200 000) for the seed the device test uses, and for a few others; every point lies in its face."""
    vertices, faces = cloud_ref.ONE_TO_THREE
    w, _ = cloud_ref.mesh_weights(vertices, faces)
    assert w.tolist() == [(1 << 32) // 3, 1 << 32]
    sigma = np.sqrt(0.25 * 0.75 / cloud_ref.PROPORTION_N)
    for seed in (cloud_ref.PROPORTION_SEED, 0, 1, 2 ** 40 + 3):
        pts, face = cloud_ref.sample_mesh(vertices, faces, cloud_ref.PROPORTION_N, seed)
        share = float((face == 0).mean())
        print(f"seed {seed}: share of the small face {share:.5f} ({(share - 0.25) / sigma:+.2f} sigma)")
        assert abs(share - 0.25) <= 5 * sigma
        assert np.all(pts[face == 0][:, 1] >= 0) and np.all(pts[face == 1][:, 1] <= 0) and np.all(pts[:, 2] == 0)
        assert np.all(pts[:, 0] >= 0) and np.all(pts[:, 0] / 2 + np.where(face == 0, pts[:, 1], -pts[:, 1] / 3) <= 1 + 1e-12)
    # uniform inside a face: the mean of the points of a triangle is its centroid
    c0 = vertices[faces[0]].mean(0)
    assert np.abs(pts[face == 0].mean(0) - c0).max() < 0.01
    # a pure function of i: the first rows of a longer draw
    assert np.array_equal(cloud_ref.sample_mesh(vertices, faces, 100, 5)[0], cloud_ref.sample_mesh(vertices, faces, 1000, 5)[0][:100])


def _mesh_ply(path, vertex_props, vrec, index_type, faces, fmt="binary_little_endian", list_name="vertex_indices", extra=b""):
    header = f"ply\nformat {fmt} 1.0\ncomment a mesh export\nelement vertex {len(vrec)}\n"
    header += "".join(f"property {k} {n}\n" for k, n in vertex_props)
    header += f"element face {len(faces)}\nproperty list uchar {index_type} {list_name}\nend_header\n"
    body = b""
    for f in faces:
        body += bytes([len(f)]) + np.asarray(f, "<u4" if index_type == "uint" else "<i4").tobytes()
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(body + extra)


def test_load_mesh(tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.normal(0, 10, (7, 3))
    faces = [[0, 1, 2], [2, 3, 4], [6, 5, 4], [0, 6, 3]]
    f32 = np.empty(7, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    f32["x"], f32["y"], f32["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    _mesh_ply(tmp_path / "f.ply", [("float", n) for n in "xyz"], f32, "int", faces)
    v, f = ply_io.load_mesh(tmp_path / "f.ply")
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.flags.c_contiguous and f.flags.c_contiguous
    assert np.array_equal(v, pts.astype(np.float32)) and f.tolist() == faces
    # double vertices with a property in between, unsigned indices, the other list name, bytes behind the faces
    f64 = np.empty(7, np.dtype([("x", "<f8"), ("quality", "u1"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4")]))
    f64["x"], f64["y"], f64["z"], f64["quality"], f64["nx"] = pts[:, 0], pts[:, 1], pts[:, 2], 9, 1.0
    _mesh_ply(tmp_path / "d.ply", [("double", "x"), ("uchar", "quality"), ("double", "y"), ("double", "z"), ("float", "nx")], f64,
              "uint", faces, list_name="vertex_index", extra=b"trailing")
    v, f = ply_io.load_mesh(tmp_path / "d.ply")
    assert v.dtype == np.float32 and np.array_equal(v, pts.astype(np.float32)) and f.dtype == np.int32 and f.tolist() == faces
    assert np.array_equal(ply_io.load_point_cloud(tmp_path / "d.ply")[0], v)          # the cloud reader sees the same vertices
    # no face at all; an index that does not fit int32
    _mesh_ply(tmp_path / "e.ply", [("float", n) for n in "xyz"], f32, "int", [])
    assert ply_io.load_mesh(tmp_path / "e.ply")[1].shape == (0, 3)
    _mesh_ply(tmp_path / "u.ply", [("float", n) for n in "xyz"], f32, "uint", [[0, 1, 0x80000000]])
    with pytest.raises(ValueError, match="int32"):
        ply_io.load_mesh(tmp_path / "u.ply")
    # a quad anywhere among the faces, ASCII, big-endian, a face element with a second property, no faces, short data
    for k, quads in enumerate(([[0, 1, 2], [2, 3, 4, 5], [6, 5, 4]], [[0, 1, 2], [2, 3, 4, 5]], [[0, 1, 2, 3]])):
        _mesh_ply(tmp_path / f"q{k}.ply", [("float", n) for n in "xyz"], f32, "int", quads)
        with pytest.raises(ValueError, match="triangle"):
            ply_io.load_mesh(tmp_path / f"q{k}.ply")
    (tmp_path / "a.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                                     b"element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    with pytest.raises(ValueError, match="little-endian"):
        ply_io.load_mesh(tmp_path / "a.ply")
    _mesh_ply(tmp_path / "b.ply", [("float", n) for n in "xyz"], f32, "int", faces, fmt="binary_big_endian")
    with pytest.raises(ValueError, match="little-endian"):
        ply_io.load_mesh(tmp_path / "b.ply")
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
    (tmp_path / "p.ply").write_bytes(head + b"element face 0\nproperty list uchar int vertex_indices\nproperty uchar flags\nend_header\n")
    with pytest.raises(ValueError, match="exactly one list property"):
        ply_io.load_mesh(tmp_path / "p.ply")
    (tmp_path / "l.ply").write_bytes(head + b"element face 0\nproperty list uint int vertex_indices\nend_header\n")
    with pytest.raises(ValueError, match="unsupported face property"):
        ply_io.load_mesh(tmp_path / "l.ply")
    (tmp_path / "n.ply").write_bytes(head + b"end_header\n")
    with pytest.raises(ValueError, match="no face element"):
        ply_io.load_mesh(tmp_path / "n.ply")
    (tmp_path / "s.ply").write_bytes(head + b"element face 2\nproperty list uchar int vertex_indices\nend_header\n" + b"\x03" + bytes(12))
    with pytest.raises(ValueError, match="shorter"):
        ply_io.load_mesh(tmp_path / "s.ply")


def test_evaluation_refuses_cpu_tensors_and_bad_shapes():
    pts, faces = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.voxel_down_sample(pts, 0.02)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.voxel_down_sample(pts.numpy(), 0.02)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.sample_mesh(pts, faces, 10)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.evaluate_recon(pts, pts, faces)


def test_cloud_math_header_on_the_host(tmp_path):
    """include/sls_cloud_math.h as plain C99 against cloud_ref.py, bit for bit: voxel keys (the double division, points
    on voxel faces, indices beyond 2^21), face areas and weights, mulhi64, the random words and the sampled point."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "cloud_math.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "sls_cloud_math.h"
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    double vs; unsigned n, i;
    fread(&vs, 8, 1, in); fread(&n, 4, 1, in);
    float mn[3]; fread(mn, 4, 3, in);
    for (i = 0; i < n; ++i) {
        float p[3]; uint64_t key; int ok;
        fread(p, 4, 3, in);
        ok = sls_voxel_key(p[0], p[1], p[2], sls_voxel_origin(mn[0], vs), sls_voxel_origin(mn[1], vs), sls_voxel_origin(mn[2], vs), vs, &key);
        fwrite(&key, 8, 1, out); fwrite(&ok, 4, 1, out);
    }
    double amax; fread(&amax, 8, 1, in); fread(&n, 4, 1, in);
    for (i = 0; i < n; ++i) {
        float v[9]; double a; uint64_t w;
        fread(v, 4, 9, in);
        a = sls_mesh_face_area(v, v + 3, v + 6);
        w = sls_mesh_weight(a, amax);
        fwrite(&a, 8, 1, out); fwrite(&w, 8, 1, out);
    }
    uint64_t seed, W; fread(&seed, 8, 1, in); fread(&W, 8, 1, in); fread(&n, 4, 1, in);
    float tri[9]; fread(tri, 4, 9, in);
    for (i = 0; i < n; ++i) {
        uint32_t r[4]; uint64_t t; float p[3];
        sls_mesh_words(i, seed, r);
        t = sls_mesh_target(r, W);
        sls_mesh_point(r, tri, tri + 3, tri + 6, p);
        fwrite(r, 4, 4, out); fwrite(&t, 8, 1, out); fwrite(p, 4, 3, out);
    }
    fclose(out);
    return 0;
}
''')
    exe = tmp_path / "cloud_math"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-lm"])
    rng = np.random.default_rng(6)
    vs = 0.3
    pts = np.concatenate([rng.normal(0, 3, (4000, 3)), rng.integers(-64, 65, (2000, 3)) * 0.3, [[700000.0, 0, 0], [0, 0, 3e38]]]).astype(np.float32)
    mn = pts.min(0)
    vertices, faces, _ = cloud_ref.grid_mesh()
    tris = vertices[faces].reshape(-1, 9)
    area, _ = cloud_ref.face_areas(vertices, faces)
    seed, W = (0xDEADBEEF << 32) | 12345, (1 << 40) * 117 + 99
    tri = np.array([[1.25, -3, 0.5], [40, 2.0625, -7], [-12.5, 9, 33]], np.float32)
    n3 = 5000
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.float64(vs).tobytes() + np.uint32(len(pts)).tobytes() + mn.tobytes() + pts.tobytes())
        f.write(np.float64(area.max()).tobytes() + np.uint32(len(tris)).tobytes() + tris.tobytes())
        f.write(np.uint64(seed).tobytes() + np.uint64(W).tobytes() + np.uint32(n3).tobytes() + tri.tobytes())
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    blob = (tmp_path / "out.bin").read_bytes()
    a = np.frombuffer(blob, np.dtype([("key", "<u8"), ("ok", "<i4")]), len(pts))
    off = a.nbytes
    b = np.frombuffer(blob, np.dtype([("area", "<f8"), ("w", "<u8")]), len(tris), off)
    off += b.nbytes
    c = np.frombuffer(blob, np.dtype([("r", "<u4", 4), ("t", "<u8"), ("p", "<f4", 3)]), n3, off)
    assert off + c.nbytes == len(blob)
    assert a["ok"][:-2].all() and not a["ok"][-2:].any() and np.all(a["key"][-2:] == 0)      # 700000 / 0.3 > 2^21; 3e38 / 0.3 = inf
    assert np.array_equal(a["key"][:-2], cloud_ref.voxel_keys(np.concatenate([pts[:-2], mn[None]]), vs)[:-1])
    assert np.array_equal(b["area"], area) and np.array_equal(b["w"], cloud_ref.mesh_weights(vertices, faces)[0])
    i = np.arange(n3, dtype=np.uint64)
    z = np.zeros(n3, np.uint64)
    r = np.stack(cloud_ref.philox4x32_10(i, z + np.uint64(2), z, z, seed & 0xFFFFFFFF, seed >> 32), 1)
    assert np.array_equal(c["r"].astype(np.uint64), r)
    assert np.array_equal(c["t"], cloud_ref.mulhi64(r[:, 0] | (r[:, 1] << np.uint64(32)), np.uint64(W)))
    assert [int(t) for t in c["t"][:50]] == [((int(x[0]) | (int(x[1]) << 32)) * W) >> 64 for x in r[:50]]     # against Python's integers
    # the same stream as the other users of Philox in this project, one counter word apart
    import densify_draw_ref
    key = (seed & 0xFFFFFFFF, seed >> 32)
    assert int(r[5, 0]) != int(densify_draw_ref.philox4x32_10((5, 0, 0, 0), key)[0][0])
    assert [int(x[0]) for x in densify_draw_ref.philox4x32_10((5, 2, 0, 0), key)] == [int(x) for x in r[5]]
    # the point: one triangle, so face 0 everywhere; the float32 mode is the header's bits, the float64 mode close to it
    p32, face = cloud_ref.sample_mesh(tri, np.array([[0, 1, 2]]), n3, seed, float32=True)
    p64, _ = cloud_ref.sample_mesh(tri, np.array([[0, 1, 2]]), n3, seed)
    assert np.all(face == 0) and np.array_equal(c["p"].view(np.uint32), p32.view(np.uint32))
    assert np.abs(c["p"] - p64).max() <= 1e-5 * 40
