"""Mesh simplification on the device (sls_mesh_simplify, mesh_ops.simplify_vertex_clustering, the stage inside
mesh_ops.clean_mesh and meshing.mesh_tsdf) against include/sls_simplify_math.h run on the host (tests/simplify_ref.py): every
case of the table bit for bit, both contractions; the capacity tails untouched; the same bits on every run; the stage inside
clean_mesh equal to the composition of the public calls with one host read."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref
import simplify_ref as ref
import tsdf_ref
from mesh_ref import bits
from splat_loam_amd import _abi, evaluation, mesh_ops, meshing, ply_io
from test_simplify_math import SPHERE
from test_tsdf import K2, SEED, VS2, _write_room

pytestmark = pytest.mark.gpu

CASES = ref.cases()
SENTINEL_V, SENTINEL_F = 7.0, -7


@functools.lru_cache(maxsize=None)
def _host(case, contraction):
    v, f, h = CASES[case]
    return ref.host().simplify(v, f, h, contraction)


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _call(device, v, f, h, contraction, regularisation=1e-3):
    """the C entry with pre-filled outputs: (vertices (V,3), faces (T,3), vmap (V,), status (10,)) at capacity, as NumPy"""
    lib, V, T = _abi.lib(), len(v), len(f)
    dv, df = _dev(v, device).contiguous(), _dev(f, device).contiguous()
    out_v = torch.full((max(V, 1), 3), SENTINEL_V, dtype=torch.float32, device=device)
    out_f = torch.full((max(T, 1), 3), SENTINEL_F, dtype=torch.int32, device=device)
    vmap = torch.full((max(V, 1),), 99, dtype=torch.int32, device=device)
    status = torch.full((10,), 9, dtype=torch.int32, device=device)
    nbytes = int(lib.sls_mesh_simplify_scratch_bytes(V, T))
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    _abi.check(lib.sls_mesh_simplify(V, dv.data_ptr(), T, df.data_ptr() if T else None, float(h), int(contraction), float(regularisation),
                                     out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), status.data_ptr(),
                                     ((scratch.data_ptr() + 255) & ~255) if nbytes else None, nbytes,
                                     torch.cuda.current_stream(device).cuda_stream), "sls_mesh_simplify")
    return out_v.cpu().numpy()[:V], out_f.cpu().numpy()[:T], vmap.cpu().numpy()[:V], status.cpu().numpy().tolist()


@pytest.mark.parametrize("contraction", (ref.AVERAGE, ref.QUADRIC))
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_equals_header(device, case, contraction):
    v, f, h = CASES[case]
    want_v, want_f, want_m, want_s = _host(case, contraction)
    got_v, got_f, got_m, status = _call(device, v, f, h, contraction)
    assert status == want_s + [9, 9], case
    nv, nt = status[0], status[1]
    assert np.array_equal(got_f[:nt], want_f) and np.array_equal(got_m, want_m)
    assert np.array_equal(bits(got_v[:nv]), bits(want_v))
    assert (got_v[nv:] == SENTINEL_V).all() and (got_f[nt:] == SENTINEL_F).all()     # rows beyond V' / T' are untouched
    again = _call(device, v, f, h, contraction)                     # the same bits on every run
    assert np.array_equal(bits(again[0]), bits(got_v)) and np.array_equal(again[1], got_f) and np.array_equal(again[2], got_m)
    assert again[3] == status
    if case == "sphere":
        assert [nv, nt, status[5], status[6]] == [SPHERE["vertices"], SPHERE["triangles"], SPHERE["duplicates"], SPHERE["fallbacks"]]
        edges = mesh_ops.cluster_triangles(_dev(got_f[:nt], device), nv, details=True)[2]
        assert (edges["boundary_edges"] == 0 and edges["nonmanifold_edges"] == 0) == SPHERE["closed"] and edges["clusters"] == 1


def test_out_of_grid_is_counted_and_stays_in_bounds(device):
    v, f, h = ref.big_case()
    for contraction in (ref.AVERAGE, ref.QUADRIC):
        got_v, got_f, got_m, status = _call(device, v, f, h, contraction)
        assert status[2:4] == [0, 2] and status[7:] == [1, 9, 9]
        nv, nt = status[0], status[1]
        assert 0 <= nv <= len(v) and 0 <= nt <= len(f) and (nt == 0 or (got_f[:nt].min() >= 0 and got_f[:nt].max() < nv))
        assert got_m.min() >= -1 and got_m.max() < max(nv, 1)
    with pytest.raises(ValueError, match="voxel_size 1.0 is too small"):
        mesh_ops.simplify_vertex_clustering(_dev(v, device), _dev(f, device), h)


def test_public_call(device):
    v, f, h = CASES["cube_0.210"]
    dv, df = _dev(v, device), _dev(f, device)
    for name, code in mesh_ops.CONTRACTIONS.items():
        want_v, want_f, want_m, want_s = _host("cube_0.210", code)
        out_v, out_f, det = mesh_ops.simplify_vertex_clustering(dv, df.long(), h, contraction=name, details=True)     # int64 faces are converted
        assert out_v.dtype == torch.float32 and out_f.dtype == torch.int32 and det["vmap"].dtype == torch.int32
        assert np.array_equal(bits(out_v.cpu().numpy()), bits(want_v)) and np.array_equal(out_f.cpu().numpy(), want_f)
        assert np.array_equal(det["vmap"].cpu().numpy(), want_m)
        assert [det[k] for k in ref.STATUS] == want_s[:7]
        plain = mesh_ops.simplify_vertex_clustering(dv, df, h, contraction=name)
        assert len(plain) == 2 and torch.equal(plain[0].view(torch.int32), out_v.view(torch.int32)) and torch.equal(plain[1], out_f)
    sharp = mesh_ops.simplify_vertex_clustering(dv, df, h, contraction="quadric", regularisation=1e-6)[0]
    assert ref.cube_distance(sharp.cpu().numpy()).max() <= 1e-5 * h
    nv, nf, _ = CASES["nonfinite"]
    with pytest.raises(ValueError, match="non-finite"):
        mesh_ops.simplify_vertex_clustering(_dev(nv, device), _dev(nf, device), 1.0)
    with pytest.raises(ValueError, match="contraction"):
        mesh_ops.simplify_vertex_clustering(dv, df, h, contraction="median")
    e_v, e_f, det = mesh_ops.simplify_vertex_clustering(dv, torch.zeros((0, 3), dtype=torch.int32, device=device), h, details=True)       # T = 0
    assert e_v.shape == (0, 3) and e_f.shape == (0, 3) and det["vmap"].tolist() == [-1] * len(v)


def _scene():
    soup = np.concatenate([mesh_ref.sphere_soup(), mesh_ref.sphere_soup(0.5, mesh_ref.FAR), mesh_ref.floater_scene()[0][-15:]])
    return soup, np.arange(len(soup), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("contraction", ("average", "quadric"))
def test_clean_mesh_with_simplify_is_the_composition(device, contraction, monkeypatch):
    """clean_mesh(simplify=h) = clean_mesh() -> simplify_vertex_clustering(h) -> vertex_normals, with ONE host read (counted
    the way test_cloud_ops counts them: every Tensor.cpu() call)"""
    soup, faces = _scene()
    h = 2 * tsdf_ref.VS
    ds, df = _dev(soup, device), _dev(faces, device)
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    v, f, n, det = mesh_ops.clean_mesh(ds, df, simplify=h, contraction=contraction, details=True)
    monkeypatch.undo()
    print(f"host reads: {reads}")
    assert len(reads) == 1
    v0, f0, det0 = mesh_ops.clean_mesh(ds, df, normals=False, details=True)
    v1, f1, det1 = mesh_ops.simplify_vertex_clustering(v0, f0, h, contraction=contraction, details=True)
    n1 = mesh_ops.vertex_normals(v1, f1)
    assert 0 < f1.shape[0] < f0.shape[0] and 0 < v1.shape[0] < v0.shape[0]
    assert torch.equal(v.view(torch.int32), v1.view(torch.int32)) and torch.equal(f, f1) and torch.equal(n.view(torch.int32), n1.view(torch.int32))
    assert {k: det["simplify"][k] for k in ref.STATUS} == {k: det1[k] for k in ref.STATUS}
    assert torch.equal(det["simplify"]["vmap"][:v0.shape[0]], det1["vmap"]) and bool((det["simplify"]["vmap"][v0.shape[0]:] == -1).all())
    assert {k: det[k] for k in det0 if k not in ("cluster_count", "labels")} == {k: det0[k] for k in det0 if k not in ("cluster_count", "labels")}
    want_v, want_f, _, want_s = ref.host().simplify(v0.cpu().numpy(), f0.cpu().numpy(), h, mesh_ops.CONTRACTIONS[contraction])
    assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
    v2, f2 = mesh_ops.clean_mesh(ds, df, simplify=h, contraction=contraction, normals=False, keep_clusters=None)       # without a selection
    w0, g0 = mesh_ops.clean_mesh(ds, df, normals=False, keep_clusters=None)
    w1, g1 = mesh_ops.simplify_vertex_clustering(w0, g0, h, contraction=contraction)
    assert torch.equal(v2.view(torch.int32), w1.view(torch.int32)) and torch.equal(f2, g1)


def test_clean_mesh_without_simplify_is_unchanged(device):
    """simplify=None on the scene of test_mesh_ops.test_clean_mesh_scene: the restatement of mesh_ref, the same details"""
    soup, faces = _scene()
    want_v, want_f, want_n = mesh_ref.clean(soup, faces, 1, 50)
    for kw in ({}, {"simplify": None, "contraction": "quadric", "regularisation": 0.5}):
        v, f, n, det = mesh_ops.clean_mesh(_dev(soup, device), _dev(faces, device), details=True, **kw)
        assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
        assert np.array_equal(bits(n.cpu().numpy()), bits(mesh_ref.host().normals(want_v, want_f)))
        assert sorted(det) == sorted(["clusters", "degenerate", "out_of_range", "boundary_edges", "nonmanifold_edges", "cluster_count", "labels",
                                      "n_min", "welded_vertices"])
        assert det["clusters"] == 7 and det["n_min"] == 7152 and det["boundary_edges"] == 15 and det["welded_vertices"] == len(mesh_ref.weld(soup)[0])


def test_mesh_tsdf_simplify_end_to_end(device, tmp_path):
    _write_room(tmp_path, True)
    v0, f0 = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, keep_clusters=1)
    v, f, n, det = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, keep_clusters=1, normals=True,
                                     simplify=2 * VS2, contraction="quadric")
    s = det["clean"]["simplify"]
    print(f"room: {int(f0.shape[0])} triangles -> {int(f.shape[0])} at twice the voxel; {s['collapsed']} collapsed, {s['duplicates']} duplicates, "
          f"{s['fallbacks']} fallbacks, clean {det['stage_ms']['clean']:.2f} ms")
    assert 0 < f.shape[0] < f0.shape[0] and 0 < v.shape[0] < v0.shape[0] and n.shape == v.shape
    assert s["triangles"] == f.shape[0] and s["vertices"] == v.shape[0] and f0.shape[0] == s["triangles"] + s["collapsed"] + s["duplicates"]
    want_v, want_f = mesh_ops.simplify_vertex_clustering(v0, f0, 2 * VS2, contraction="quadric")
    assert torch.equal(v.view(torch.int32), want_v.view(torch.int32)) and torch.equal(f, want_f)
    ply_io.save_mesh(tmp_path / "small.ply", v, f, normals=n)
    lv, lf = ply_io.load_mesh(tmp_path / "small.ply")
    assert np.array_equal(bits(lv), bits(v.cpu().numpy())) and np.array_equal(lf, f.cpu().numpy())
    pts, _ = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    metrics = evaluation.evaluate_recon(pts, v, f, down_sample_res=0.02, mesh_sample_point=20000, seed=1)
    assert isinstance(metrics, dict) and "Chamfer_L1 (cm)" in metrics
    assert all(np.isfinite(float(x)) for x in metrics.values() if isinstance(x, (int, float)))
