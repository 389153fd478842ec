"""Mesh smoothing on the device (sls_mesh_adjacency, sls_mesh_smooth, mesh_ops.vertex_adjacency, mesh_ops.smooth, the stage
inside mesh_ops.clean_mesh and meshing.mesh_tsdf) against include/sls_smooth_math.h run on the host (tests/smooth_ref.py):
every case of the table and every setting bit for bit; the capacity tail untouched; the same bits on every run; the stage
inside clean_mesh equal to the composition of the public calls with one host read."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref
import smooth_ref as ref
from mesh_ref import bits
from splat_loam_amd import _abi, evaluation, mesh_ops, meshing, ply_io
from test_tsdf import K2, SEED, VS2, _write_room

pytestmark = pytest.mark.gpu

CASES = ref.cases()
SETTINGS = ref.settings()
SENTINEL_V, SENTINEL_N = 7.0, -7


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _aligned(nbytes, device):
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    return scratch, (((scratch.data_ptr() + 255) & ~255) if nbytes else None)


def _adjacency(device, f, V):
    """the C entry with pre-filled outputs: (offsets (V+1,), neighbours (6T,) at capacity, boundary (V,), status (10,)), as NumPy"""
    lib, T = _abi.lib(), len(f)
    df = _dev(f, device).contiguous()
    offsets = torch.full((V + 1,), 99, dtype=torch.int32, device=device)
    nbr = torch.full((max(6 * T, 1),), SENTINEL_N, dtype=torch.int32, device=device)
    boundary = torch.full((max(V, 1),), 9, dtype=torch.uint8, device=device)
    status = torch.full((10,), 9, dtype=torch.int32, device=device)
    nbytes = int(lib.sls_mesh_adjacency_scratch_bytes(V, T))
    hold, ptr = _aligned(nbytes, device)
    _abi.check(lib.sls_mesh_adjacency(V, T, df.data_ptr() if T else None, offsets.data_ptr(), nbr.data_ptr(), boundary.data_ptr(),
                                      status.data_ptr(), ptr, nbytes, torch.cuda.current_stream(device).cuda_stream), "sls_mesh_adjacency")
    return offsets.cpu().numpy(), nbr.cpu().numpy()[:6 * T], boundary.cpu().numpy()[:V], status.cpu().numpy().tolist()


def _smooth(device, dv, df, V, T, method, weights, fix, n):
    """the C entry with a pre-filled output: (vertices (V,3), status (10,)), as NumPy"""
    lib = _abi.lib()
    out = torch.full((max(V, 1), 3), SENTINEL_V, dtype=torch.float32, device=device)
    status = torch.full((10,), 9, dtype=torch.int32, device=device)
    nbytes = int(lib.sls_mesh_smooth_scratch_bytes(V, T))
    hold, ptr = _aligned(nbytes, device)
    _abi.check(lib.sls_mesh_smooth(V, dv.data_ptr() if V else None, T, df.data_ptr() if T else None, method, weights, n, ref.LAMBDA, ref.MU,
                                   int(fix), out.data_ptr(), status.data_ptr(), ptr, nbytes, torch.cuda.current_stream(device).cuda_stream),
               "sls_mesh_smooth")
    return out.cpu().numpy()[:V], status.cpu().numpy().tolist()


@functools.lru_cache(maxsize=None)
def _host(case, setting):
    v, f = CASES[case]
    method, weights, fix, n = setting
    return ref.host().smooth(v, f, n, method, weights, fix_boundary=fix)


@pytest.mark.parametrize("case", sorted(CASES))
def test_adjacency_equals_header(device, case):
    v, f = CASES[case]
    want_o, want_n, want_b, want_s = ref.host().adjacency(f, len(v))
    got_o, got_n, got_b, status = _adjacency(device, f, len(v))
    assert status == want_s + [9, 9], case
    n2 = 2 * status[1]
    assert np.array_equal(got_o, want_o) and np.array_equal(got_n[:n2], want_n) and np.array_equal(got_b, want_b)
    assert (got_n[n2:] == SENTINEL_N).all()                         # entries beyond 2 E are untouched
    again = _adjacency(device, f, len(v))                           # the same on every run
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], (got_o, got_n, got_b))) and again[3] == status


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_equals_header(device, case):
    v, f = CASES[case]
    V, T = len(v), len(f)
    dv, df = _dev(v, device).contiguous(), _dev(f, device).contiguous()
    for setting in SETTINGS:
        want_v, want_s = _host(case, setting)
        got_v, status = _smooth(device, dv, df, V, T, *setting)
        assert status == want_s + [9, 9], (case, setting)
        if case not in ref.UNSPECIFIED:
            assert np.array_equal(bits(got_v), bits(want_v)), (case, setting)       # all V rows, the copied ones included
        again_v, again_s = _smooth(device, dv, df, V, T, *setting)                 # the same bits on every run
        assert np.array_equal(bits(again_v), bits(got_v)) and again_s == status, (case, setting)


def test_public_calls(device):
    v, f = CASES["sheet_noisy"]
    dv, df = _dev(v, device), _dev(f, device)
    offsets, nbr, boundary, det = mesh_ops.vertex_adjacency(df.long(), len(v), details=True)        # int64 faces are converted
    want_o, want_n, want_b, want_s = ref.host().adjacency(f, len(v))
    assert offsets.dtype == torch.int32 and nbr.dtype == torch.int32 and boundary.dtype == torch.uint8 and nbr.shape == (2 * want_s[1],)
    assert np.array_equal(offsets.cpu().numpy(), want_o) and np.array_equal(nbr.cpu().numpy(), want_n)
    assert np.array_equal(boundary.cpu().numpy(), want_b)
    assert det == {k: x for k, x in zip(ref.STATUS, want_s) if k != "nonfinite"}
    assert len(mesh_ops.vertex_adjacency(df, len(v))) == 3
    for method, m in ref.METHODS.items():
        for weights, w in ref.WEIGHTS.items():
            for fix in (False, True):
                want_v, want_s = _host("sheet_noisy", (m, w, fix, 2))
                out, det = mesh_ops.smooth(dv, df.long(), 2, method=method, weights=weights, fix_boundary=fix, details=True)
                assert out.dtype == torch.float32 and out.shape == dv.shape
                assert np.array_equal(bits(out.cpu().numpy()), bits(want_v)) and [det[k] for k in ref.STATUS] == want_s[:7]
    plain = mesh_ops.smooth(dv, df, 2)                              # the defaults: Taubin, inverse distance, 0.5 / -0.53
    assert torch.is_tensor(plain) and np.array_equal(bits(plain.cpu().numpy()), bits(_host("sheet_noisy", (ref.TAUBIN, ref.INVERSE_DISTANCE, False, 2))[0]))
    other = mesh_ops.smooth(dv, df, 2, method="laplacian", lambda_=0.25)
    assert np.array_equal(bits(other.cpu().numpy()), bits(ref.host().smooth(v, f, 2, ref.LAPLACIAN, lam=0.25)[0]))
    nv, nf = CASES["nan_live"]
    with pytest.raises(ValueError, match="non-finite"):
        mesh_ops.smooth(_dev(nv, device), _dev(nf, device), 1)
    bv, bf = CASES["bad_indices"]
    with pytest.raises(ValueError, match="outside the vertices"):
        mesh_ops.smooth(_dev(bv, device), _dev(bf, device), 1)
    with pytest.raises(ValueError, match="outside the vertices"):
        mesh_ops.vertex_adjacency(_dev(bf, device), len(bv))
    with pytest.raises(ValueError, match="method"):
        mesh_ops.smooth(dv, df, 1, method="cotangent")
    empty = mesh_ops.smooth(dv, torch.zeros((0, 3), dtype=torch.int32, device=device), 3, details=True)                     # T = 0
    assert torch.equal(empty[0].view(torch.int32), dv.view(torch.int32)) and empty[1]["live"] == 0


def _scene():
    soup = np.concatenate([mesh_ref.sphere_soup(), mesh_ref.sphere_soup(0.5, mesh_ref.FAR), mesh_ref.floater_scene()[0][-15:]])
    return soup, np.arange(len(soup), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("kw", ({}, {"smooth_method": "laplacian", "smooth_weights": "uniform", "fix_boundary": True, "smooth_lambda": 0.25},
                                {"simplify": 0.25}))
def test_clean_mesh_with_smooth_is_the_composition(device, kw, monkeypatch):
    """clean_mesh(smooth=n) = clean_mesh() -> smooth(n) -> vertex_normals, with ONE host read (counted the way
    test_simplify counts them: every Tensor.cpu() call)"""
    soup, faces = _scene()
    ds, df = _dev(soup, device), _dev(faces, device)
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    v, f, n, det = mesh_ops.clean_mesh(ds, df, smooth=3, details=True, **kw)
    monkeypatch.undo()
    print(f"host reads: {reads}")
    assert len(reads) == 1
    first = {k: x for k, x in kw.items() if k == "simplify"}
    v0, f0, det0 = mesh_ops.clean_mesh(ds, df, normals=False, details=True, **first)
    v1, det1 = mesh_ops.smooth(v0, f0, 3, method=kw.get("smooth_method", "taubin"), weights=kw.get("smooth_weights", "inverse_distance"),
                               lambda_=kw.get("smooth_lambda", 0.5), fix_boundary=kw.get("fix_boundary", False), details=True)
    n1 = mesh_ops.vertex_normals(v1, f0)
    assert torch.equal(f, f0) and v.shape == v0.shape and not torch.equal(v, v0)        # the faces are unchanged by the stage
    assert torch.equal(v.view(torch.int32), v1.view(torch.int32)) and torch.equal(n.view(torch.int32), n1.view(torch.int32))
    # the stage ran at capacity: rows of -1 and unreferenced vertices took no part, and count as such
    same = ("live", "edges", "boundary", "nonfinite", "max_row")
    assert {k: det["smooth"][k] for k in same} == {k: det1[k] for k in same} and det["smooth"]["live"] == v0.shape[0]
    assert {k: det[k] for k in det0 if k not in ("cluster_count", "labels", "simplify")} == \
        {k: det0[k] for k in det0 if k not in ("cluster_count", "labels", "simplify")}
    want = ref.host().smooth(v0.cpu().numpy(), f0.cpu().numpy(), 3, ref.METHODS[kw.get("smooth_method", "taubin")],
                             ref.WEIGHTS[kw.get("smooth_weights", "inverse_distance")], lam=kw.get("smooth_lambda", 0.5),
                             fix_boundary=kw.get("fix_boundary", False))[0]
    assert np.array_equal(bits(v.cpu().numpy()), bits(want))


def test_clean_mesh_without_smooth_is_unchanged(device):
    """smooth=None on the scene of test_mesh_ops.test_clean_mesh_scene: the restatement of mesh_ref, the same details"""
    soup, faces = _scene()
    want_v, want_f, want_n = mesh_ref.clean(soup, faces, 1, 50)
    for kw in ({}, {"smooth": None, "smooth_method": "simple", "fix_boundary": True}):
        v, f, n, det = mesh_ops.clean_mesh(_dev(soup, device), _dev(faces, device), details=True, **kw)
        assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
        assert np.array_equal(bits(n.cpu().numpy()), bits(mesh_ref.host().normals(want_v, want_f)))
        assert "smooth" not in det and "simplify" not in det


def test_mesh_tsdf_smooth_end_to_end(device, tmp_path):
    _write_room(tmp_path, True)
    v0, f0 = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, keep_clusters=1)
    v, f, n, det = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, keep_clusters=1, normals=True,
                                     smooth=2)
    s = det["clean"]["smooth"]
    moved = (v - v0).norm(dim=1)
    print(f"room: {int(f.shape[0])} triangles, {s['live']} live vertices, {s['edges']} edges, {s['boundary']} boundary vertices, largest row "
          f"{s['max_row']}; moved {float(moved.mean()):.4f} m on average, {float(moved.max()):.4f} m at most; clean {det['stage_ms']['clean']:.2f} ms")
    assert torch.equal(f, f0) and v.shape == v0.shape and n.shape == v.shape        # faces are unchanged by the stage
    assert s["live"] == v.shape[0] and s["nonfinite"] == 0 and float(moved.max()) > 0 and bool(torch.isfinite(v).all())
    want = mesh_ops.smooth(v0, f0, 2)
    assert torch.equal(v.view(torch.int32), want.view(torch.int32))
    ply_io.save_mesh(tmp_path / "smooth.ply", v, f, normals=n)
    lv, lf = ply_io.load_mesh(tmp_path / "smooth.ply")
    assert np.array_equal(bits(lv), bits(v.cpu().numpy())) and np.array_equal(lf, f.cpu().numpy())
    pts, _ = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    metrics = evaluation.evaluate_recon(pts, v, f, down_sample_res=0.02, mesh_sample_point=20000, seed=1)
    assert isinstance(metrics, dict) and "Chamfer_L1 (cm)" in metrics
    assert all(np.isfinite(float(x)) for x in metrics.values() if isinstance(x, (int, float)))
