"""The mesh cleaning stage on the device (sls_mesh_weld, sls_mesh_clusters, sls_mesh_filter, sls_mesh_vertex_normals,
splat_loam_amd/mesh_ops.py, meshing.mesh_tsdf's clean stage) against the restatement of tests/mesh_ref.py and
include/sls_mesh_math.h run on the host: weld equal to tsdf.weld_soup and np.unique, labels / counts / status words equal
to the breadth-first walk, the selection equal to the rule, normals equal to the header bit for bit."""
import numpy as np
import pytest
import torch

import mesh_ref as ref
from mesh_ref import bits
from splat_loam_amd import _abi, evaluation, mesh_ops, meshing, ply_io, tsdf
from test_mesh_math import SELECTIONS
from test_tsdf import K2, SEED, VS2, _write_room

pytestmark = pytest.mark.gpu

WELD_CASES = ref.weld_cases()
CLUSTER_CASES = ref.cluster_cases()
# One workgroup's share of every chunked pass the weld runs: the sorter's histogram / scatter take 1024 items per wave and,
# at the 11-bit digits of a 32-bit key, 4 waves = 4096 items per workgroup; the head scan takes 2048 positions.
CHUNKS = {"sort_wave": 1024, "head_scan": 2048, "sort_workgroup": 4096}
SIZED = sorted({n + d for n in CHUNKS.values() for d in (-1, 0, 1)})


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _check_weld(device, rows):
    d = _dev(rows, device)
    v, index = mesh_ops.weld_rows(d)
    want_v, want_i = ref.weld(rows)
    assert v.dtype == torch.float32 and index.dtype == torch.int32 and index.shape == (len(rows),)
    assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(index.cpu().numpy(), want_i)
    if len(rows):                                                   # torch.unique on the int32 view: the same order
        uniq, inverse = torch.unique(d.view(torch.int32), dim=0, return_inverse=True)
        assert torch.equal(v.view(torch.int32), uniq) and torch.equal(index.long(), inverse)
    v2, index2 = mesh_ops.weld_rows(d)                              # the same bytes on every run
    assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(index2, index)
    return v, index


@pytest.mark.parametrize("case", sorted(WELD_CASES))
def test_weld(device, case):
    rows = WELD_CASES[case]
    v, index = _check_weld(device, rows)
    if len(rows) % 3 == 0:                                          # as a soup: tsdf.weld_soup is the yardstick
        d = _dev(rows, device)
        got_v, got_f = mesh_ops.weld(d)
        want_v, want_f = tsdf.weld_soup(d)
        assert got_f.dtype == torch.int32 and got_f.shape == want_f.shape
        assert torch.equal(got_v.view(torch.int32), want_v.view(torch.int32)) and torch.equal(got_f, want_f)
    if case == "sphere":
        assert v.shape == (3578, 3)


@pytest.mark.parametrize("n", SIZED)
def test_weld_chunk_boundaries(device, n):
    _check_weld(device, ref.sized_rows(n))


def test_weld_capacity_tail_untouched(device):
    rows = _dev(WELD_CASES["lattice"], device)
    lib, N = _abi.lib(), int(rows.shape[0])
    out = torch.full((N, 3), 7.0, dtype=torch.float32, device=device)
    index = torch.empty((N,), dtype=torch.int32, device=device)
    status = torch.zeros((4,), dtype=torch.int32, device=device)
    nbytes = lib.sls_mesh_weld_scratch_bytes(N)
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    _abi.check(lib.sls_mesh_weld(N, rows.data_ptr(), out.data_ptr(), index.data_ptr(), status.data_ptr(), (scratch.data_ptr() + 255) & ~255,
                                 nbytes, torch.cuda.current_stream(device).cuda_stream), "sls_mesh_weld")
    assert status.tolist() == [40, 0, 0, 1] and bool((out[40:] == 7.0).all())
    status.fill_(9)                                                 # zero rows: the status words alone
    _abi.check(lib.sls_mesh_weld(0, None, None, None, status.data_ptr(), None, 0, torch.cuda.current_stream(device).cuda_stream), "sls_mesh_weld")
    assert status.tolist() == [0, 0, 0, 1]


def _clusters(device, faces, V):
    status = torch.full((8,), 9, dtype=torch.int32, device=device)
    f = _dev(faces, device).contiguous()
    if len(faces) == 0:
        lib = _abi.lib()
        _abi.check(lib.sls_mesh_clusters(0, None, V, None, None, status.data_ptr(), None, 0, torch.cuda.current_stream(device).cuda_stream),
                   "sls_mesh_clusters")
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64), status.cpu().numpy()
    labels, counts = mesh_ops._clusters_launch(f, V, status)
    w = status.cpu().numpy()
    return labels.cpu().numpy().astype(np.int64), counts[:int(w[0])].cpu().numpy().astype(np.int64), w


@pytest.mark.parametrize("case", sorted(CLUSTER_CASES))
def test_clusters(device, case):
    faces, V = CLUSTER_CASES[case]
    want_l, want_c, s = ref.clusters(faces, V)
    for run in range(2):                                            # the same labels whatever the order of execution
        labels, counts, w = _clusters(device, faces, V)
        assert list(w[:6]) == [s["clusters"], s["degenerate"], s["out_of_range"], s["boundary_edges"], s["nonmanifold_edges"], 1], case
        assert list(w[6:]) == [9, 9]
        assert np.array_equal(labels, want_l) and np.array_equal(counts, want_c)
    expected = {"two_tets": 2, "strip": 1, "fan": 1, "degenerate": 2, "isolated": 1, "scene": 7, "empty": 0}
    assert s["clusters"] == expected[case]


def test_cluster_triangles_details_and_range_error(device):
    faces, V = ref.FAN
    labels, counts, det = mesh_ops.cluster_triangles(_dev(faces, device), V, details=True)
    assert labels.tolist() == [0, 0, 0] and counts.tolist() == [3]
    assert det == {"clusters": 1, "degenerate": 0, "out_of_range": 0, "boundary_edges": 6, "nonmanifold_edges": 1}
    labels, counts = mesh_ops.cluster_triangles(_dev(faces, device).long(), V)          # int64 faces are converted
    assert labels.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="outside the vertices"):
        mesh_ops.cluster_triangles(_dev(ref.DEGENERATE[0], device), ref.DEGENERATE[1])
    with pytest.raises(ValueError, match="outside the vertices"):
        mesh_ops.keep_clusters(torch.zeros((6, 3), device=device), _dev(ref.DEGENERATE[0], device))
    sv, sf = ref.floater_scene()                                    # a large T with the capacity tail of counts untouched
    status = torch.zeros((8,), dtype=torch.int32, device=device)
    lib, T = _abi.lib(), len(sf)
    f = _dev(sf, device)
    labels = torch.empty((T,), dtype=torch.int32, device=device)
    counts = torch.full((T,), -5, dtype=torch.int32, device=device)
    nbytes = lib.sls_mesh_clusters_scratch_bytes(T)
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    _abi.check(lib.sls_mesh_clusters(T, f.data_ptr(), len(sv), labels.data_ptr(), counts.data_ptr(), status.data_ptr(),
                                     (scratch.data_ptr() + 255) & ~255, nbytes, torch.cuda.current_stream(device).cuda_stream), "sls_mesh_clusters")
    assert bool((counts[7:] == -5).all()) and int(counts[:7].sum()) == T


@pytest.mark.parametrize("keep,floor", SELECTIONS)
def test_selection(device, keep, floor):
    v, f = ref.floater_scene()
    want_v, want_f, want_n = ref.select(v, f, keep, floor)
    got_v, got_f, det = mesh_ops.keep_clusters(_dev(v, device), _dev(f, device), keep_clusters=keep, min_triangles=floor, details=True)
    assert det["n_min"] == want_n and det["clusters"] == 7 and det["cluster_count"].tolist() == list(ref.clusters(f, len(v))[1])
    assert got_f.dtype == torch.int32
    assert np.array_equal(bits(got_v.cpu().numpy()), bits(want_v)) and np.array_equal(got_f.cpu().numpy(), want_f)
    if (keep, floor) == (1, 50):                                    # the big sphere alone, closed
        _, counts, closed = mesh_ops.cluster_triangles(got_f, int(got_v.shape[0]), details=True)
        assert counts.tolist() == [7152] and closed["boundary_edges"] == 0 and closed["nonmanifold_edges"] == 0
        assert got_v.shape == (3578, 3) and ref.euler(got_f.cpu().numpy()) == 2
    if (keep, floor) == (2, 50):                                    # both spheres
        assert mesh_ops.cluster_triangles(got_f, int(got_v.shape[0]), details=True)[2]["clusters"] == 2
    if (keep, floor) == (100, 2):                                   # k > C: only the floaters go
        assert int(got_f.shape[0]) == len(f) - 5 and int(got_v.shape[0]) == len(v) - 15


def test_selection_ties_empty_and_vertex_map(device):
    faces, V = ref.TWO_TETS                                         # two equal-sized clusters at the threshold: both stay
    verts = torch.arange(3 * V, dtype=torch.float32, device=device).view(V, 3)
    got_v, got_f, det = mesh_ops.keep_clusters(verts, _dev(faces, device), keep_clusters=1, min_triangles=0, details=True)
    assert det["n_min"] == 4 and torch.equal(got_v, verts) and np.array_equal(got_f.cpu().numpy(), faces)
    # one tetrahedron and an unreferenced vertex in front of it: the vertex map through the C entry
    f = _dev(faces[:4] + 1, device).contiguous()
    v = torch.arange(3 * (V + 1), dtype=torch.float32, device=device).view(V + 1, 3)
    status = torch.zeros((16,), dtype=torch.int32, device=device)
    labels, counts = mesh_ops._clusters_launch(f, V + 1, status[0:8])
    lib = _abi.lib()
    out_v = torch.full((V + 1, 3), -1.0, device=device)
    out_f = torch.full((4, 3), -7, dtype=torch.int32, device=device)
    vmap = torch.full((V + 1,), 99, dtype=torch.int32, device=device)
    nbytes = lib.sls_mesh_filter_scratch_bytes(V + 1, 4)
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    _abi.check(lib.sls_mesh_filter(V + 1, v.data_ptr(), 4, f.data_ptr(), labels.data_ptr(), counts.data_ptr(), status.data_ptr(), 1, 50,
                                   out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), status[8:].data_ptr(), (scratch.data_ptr() + 255) & ~255,
                                   nbytes, torch.cuda.current_stream(device).cuda_stream), "sls_mesh_filter")
    assert status[8:12].tolist() == [0, 0, 50, 1]                   # 4 triangles < the floor of 50: nothing stays
    assert vmap.tolist() == [-1] * (V + 1) and bool((out_v == -1.0).all()) and bool((out_f == -7).all())
    _abi.check(lib.sls_mesh_filter(V + 1, v.data_ptr(), 4, f.data_ptr(), labels.data_ptr(), counts.data_ptr(), status.data_ptr(), 1, 0,
                                   out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), status[8:].data_ptr(), (scratch.data_ptr() + 255) & ~255,
                                   nbytes, torch.cuda.current_stream(device).cuda_stream), "sls_mesh_filter")
    assert status[8:12].tolist() == [4, 4, 4, 1] and vmap.tolist() == [-1, 0, 1, 2, 3, -1, -1, -1]
    assert torch.equal(out_v[:4], v[1:5]) and bool((out_v[4:] == -1.0).all()) and np.array_equal(out_f.cpu().numpy(), faces[:4])
    e_v, e_f = mesh_ops.keep_clusters(v, torch.zeros((0, 3), dtype=torch.int32, device=device))      # T = 0
    assert e_v.shape == (0, 3) and e_f.shape == (0, 3)


def test_vertex_normals(device):
    h = ref.host()
    rng = np.random.default_rng(2)
    cancel_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [5, 5, 5], [0, 0, 0]], np.float32)
    cancel_f = np.array([[0, 1, 2], [0, 2, 1], [6, 1, 2]], np.int32)
    for v, f in (ref.floater_scene(), (rng.normal(0, 1, (7, 3)).astype(np.float32), ref.DEGENERATE[0]), (cancel_v, cancel_f),
                 (cancel_v, np.zeros((0, 3), np.int32))):
        got = mesh_ops.vertex_normals(_dev(v, device), _dev(f, device)).cpu().numpy()
        assert np.array_equal(bits(got), bits(h.normals(v, f)))                        # the header on the host, bit for bit
        assert np.abs(got.astype(np.float64) - ref.normals64(v, f)[0]).max() <= 1e-5
    got = mesh_ops.vertex_normals(_dev(cancel_v, device), _dev(cancel_f, device)).cpu().numpy()
    assert np.array_equal(bits(got[[0, 3, 4, 5]]), bits(np.zeros((4, 3))))              # cancelled exactly; unreferenced
    assert np.array_equal(got[6], [0, 0, 1])
    assert mesh_ops.vertex_normals(torch.zeros((0, 3), device=device), torch.zeros((0, 3), dtype=torch.int32, device=device)).shape == (0, 3)


def test_clean_mesh_scene(device):
    """The soup of both spheres and the floaters through the whole chain, one host read: equal to the restatement."""
    soup = np.concatenate([ref.sphere_soup(), ref.sphere_soup(0.5, ref.FAR), ref.floater_scene()[0][-15:]])
    faces = np.arange(len(soup), dtype=np.int32).reshape(-1, 3)
    want_v, want_f, want_n = ref.clean(soup, faces, 1, 50)
    v, f, n, det = mesh_ops.clean_mesh(_dev(soup, device), _dev(faces, device), details=True)
    assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
    assert np.array_equal(bits(n.cpu().numpy()), bits(ref.host().normals(want_v, want_f)))
    assert np.abs(n.cpu().numpy().astype(np.float64) - want_n).max() <= 1e-5
    assert det["clusters"] == 7 and det["n_min"] == 7152 and det["boundary_edges"] == 15 and det["welded_vertices"] == len(ref.weld(soup)[0])
    v2, f2 = mesh_ops.clean_mesh(_dev(soup, device), _dev(faces, device), keep_clusters=None, normals=False)    # weld alone
    wv, wf = tsdf.weld_soup(_dev(soup, device))
    assert torch.equal(v2.view(torch.int32), wv.view(torch.int32)) and torch.equal(f2, wf)
    sv, sf = ref.floater_scene()                                    # an indexed mesh, no weld
    v3, f3, n3 = mesh_ops.clean_mesh(_dev(sv, device), _dev(sf, device), weld=False, keep_clusters=2)
    want3_v, want3_f, _ = ref.select(sv, sf, 2, 50)
    assert np.array_equal(bits(v3.cpu().numpy()), bits(want3_v)) and np.array_equal(f3.cpu().numpy(), want3_f)
    assert np.array_equal(bits(n3.cpu().numpy()), bits(ref.host().normals(want3_v, want3_f)))


def test_clean_mesh_end_to_end(device, tmp_path):
    _write_room(tmp_path, True)
    soup, soup_faces, det0 = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True)
    v0, f0 = det0["volume"].extract()                               # the defaults: the soup as TsdfVolume.extract gives it
    assert torch.equal(soup.view(torch.int32), v0.view(torch.int32)) and torch.equal(soup_faces, f0) and "clean" not in det0
    assert "clean" not in det0["stage_ms"]
    plain = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device)
    assert len(plain) == 2 and torch.equal(plain[0].view(torch.int32), v0.view(torch.int32)) and torch.equal(plain[1], f0)
    v, f, n, det = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, keep_clusters=1, normals=True)
    want_v, want_f, want_n = ref.clean(soup.cpu().numpy(), soup_faces.cpu().numpy(), 1, 50)
    print(f"room: {int(soup_faces.shape[0])} triangles -> {int(f.shape[0])} kept; {det['clean']['clusters']} clusters, n_min "
          f"{det['clean']['n_min']}, clean {det['stage_ms']['clean']:.2f} ms")
    assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
    assert np.array_equal(bits(n.cpu().numpy()), bits(ref.host().normals(want_v, want_f)))
    assert np.abs(n.cpu().numpy().astype(np.float64) - want_n).max() <= 1e-5
    assert "clean" in det["stage_ms"] and det["clean"]["clusters"] >= 1 and len(want_f) > 1000
    v1, f1 = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, keep_clusters=1)
    assert torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(f1, f)
    ply_io.save_mesh(tmp_path / "clean.ply", v, f, normals=n)
    lv, lf = ply_io.load_mesh(tmp_path / "clean.ply")
    assert np.array_equal(bits(lv), bits(v.cpu().numpy())) and np.array_equal(lf, f.cpu().numpy())
    assert np.array_equal(bits(ply_io.load_point_cloud(tmp_path / "clean.ply")[1]), bits(n.cpu().numpy()))
    pts, _ = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    metrics = evaluation.evaluate_recon(pts, v, f, down_sample_res=0.02, mesh_sample_point=20000, seed=1)
    assert all(np.isfinite(float(x)) for x in metrics.values() if isinstance(x, (int, float)))
