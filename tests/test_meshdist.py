"""sls_mesh_distance / sls_error_colors / splat_loam_amd.evaluation (point_to_mesh, error_colors, evaluate_recon's exact
completeness and error map) on the device, against the float64 brute force and the header compiled for the host
(tests/meshdist_ref.py).

What is asserted of the search is what it promises: the float64 distance to the RETURNED face is within 1e-5 of the scale
of the float64 minimum over all faces — not that the face is the brute force's argmin, since outside a convex mesh a large
share of the queries are nearest to a shared edge or vertex and two or more faces tie in truth — and that dist2 and the
closest point are the header's bits for (query, returned face)."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import mesh_ref
import meshdist_ref as R
from splat_loam_amd import _abi, evaluation, ply_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tt(a, device):
    return torch.tensor(np.ascontiguousarray(a), device=device)


def run(device, q, v, f):
    d2, face, closest = evaluation.point_to_mesh(tt(q, device), tt(v, device), tt(f, device), return_face=True, return_closest=True)
    assert d2.dtype == torch.float32 and face.dtype == torch.int32 and closest.dtype == torch.float32
    assert d2.shape == face.shape == (len(q),) and closest.shape == (len(q), 3)
    return d2.cpu().numpy(), face.cpu().numpy(), closest.cpu().numpy()


@functools.lru_cache(maxsize=None)
def brute(name, F, Mq):
    """(q, v, f, float64 minimum over all faces): computed once per case"""
    v, f = mesh(name, F)
    q = R.queries_for(v, f, Mq, seed=1000 * F + Mq)
    return q, v, f, R.mesh64(q, v, f)[0]


def check(device, name, F, Mq):
    q, v, f, d2_min = brute(name, F, Mq)
    d2, face, closest = run(device, q, v, f)
    assert ((face >= 0) & (face < len(f))).all()
    a, b, c = (v[f[face, k]] for k in range(3))
    # 1. the returned face is a nearest one, within the bar; no query is excluded
    d_face = np.sqrt(R.triangle64(q, a, b, c)[0])
    excess = (d_face - np.sqrt(d2_min)) / R.scale_of(q, a, b, c)
    print(f"{name} F={F} Mq={Mq}: returned face beyond the float64 minimum by {excess.max():.3e} of the scale at most")
    assert (excess <= R.BAR).all()
    # 2. dist2 and the closest point are the header's bits for (query, returned face)
    h2, hclosest = R.host().triangles(q, a, b, c)
    assert np.array_equal(d2.view(np.uint32), h2.view(np.uint32))
    assert np.array_equal(closest.view(np.uint32), hclosest.view(np.uint32))
    # 3. two runs give identical bytes
    again = run(device, q, v, f)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((d2, face, closest), again))
    return d2, face


@functools.lru_cache(maxsize=None)
def mesh(name, F):
    if name == "grid":                      # the first F faces of the 92 x 92 grid, in its seeded random face order
        v, f = R.grid_mesh()
        return v, f[:F]
    if name == "sphere":                    # the marching-tetrahedra sphere, welded: slivers included
        v, index = mesh_ref.weld(mesh_ref.sphere_soup())
        return v, index.reshape(-1, 3).astype(np.int32)
    if name == "loose":                     # the grid plus ONE triangle spanning its whole bounding box: loose boxes
        v, f = R.grid_mesh()
        lo, hi = v.min(0), v.max(0)
        big = np.array([lo, [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]]], np.float32)
        return np.concatenate([v, big]), np.concatenate([f[:F - 1], [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    raise KeyError(name)


# the seams of the sweep: a single face; the run of 32; the box of 256; 16 928 faces = 67 boxes, a second chunk of 64 boxes
# — against the wave's seams on the query side
@pytest.mark.parametrize("Mq", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("F", [1, 31, 32, 33, 255, 256, 257])
def test_grid_at_the_seams(device, F, Mq):
    check(device, "grid", F, Mq)


@pytest.mark.parametrize("Mq", [1, 65, 256])
def test_grid_second_chunk_of_boxes(device, Mq):
    assert len(R.grid_mesh()[1]) == 16928 > 64 * 256
    check(device, "grid", 16928, Mq)


@pytest.mark.parametrize("Mq", [64, 257])
def test_sphere(device, Mq):
    v, f = mesh("sphere", 0)
    check(device, "sphere", 0, Mq)
    # outside a convex mesh the nearest feature is often shared: the reason the argmin is not asserted
    assert len(f) == 7152


@pytest.mark.parametrize("F,Mq", [(300, 65), (16928, 256)])
def test_one_huge_triangle_among_small_ones(device, F, Mq):
    d2, face = check(device, "loose", F, Mq)
    print(f"queries nearest to the huge triangle: {(face == F - 1).sum()} of {Mq}")
    assert 0 < (face == F - 1).sum() < Mq


def test_duplicate_faces_lowest_index(device):
    """Every face twice, the copies in another order behind the originals: equal d2 BITS, so the lower index of the pair
    must be named whichever run or box each copy falls into (the radix sort is stable: copies are neighbours on the
    curve, and about one pair in 32 straddles a run, one in 256 a box)."""
    v, f0 = R.grid_mesh()
    f0 = f0[:1500]
    perm = np.random.default_rng(3).permutation(len(f0))
    f = np.concatenate([f0, f0[perm]])
    first = np.concatenate([np.arange(len(f0)), perm])                   # the lowest index holding the same face
    q = R.queries_for(v, f0, 512, seed=77)
    d2, face, closest = run(device, q, v, f)
    assert np.array_equal(face, first[face])
    # ... and it names the same faces, with the same bits, as the mesh without the copies
    d2_single, face_single, closest_single = run(device, q, v, f0)
    assert np.array_equal(face, face_single) and d2.tobytes() == d2_single.tobytes() and closest.tobytes() == closest_single.tobytes()


def test_outputs_are_optional_and_no_query_is_fine(device):
    q, v, f, _ = brute("grid", 257, 65)
    d2, face, closest = run(device, q, v, f)
    tq, tv, tf = tt(q, device), tt(v, device), tt(f, device)
    only = evaluation.point_to_mesh(tq, tv, tf, return_face=False)
    assert isinstance(only, torch.Tensor) and only.cpu().numpy().tobytes() == d2.tobytes()
    d2b, closest_b = evaluation.point_to_mesh(tq, tv, tf.long(), return_face=False, return_closest=True)      # int64 faces too
    assert d2b.cpu().numpy().tobytes() == d2.tobytes() and closest_b.cpu().numpy().tobytes() == closest.tobytes()
    d2c, face_c = evaluation.point_to_mesh(tq, tv, tf)
    assert face_c.cpu().numpy().tobytes() == face.tobytes()
    empty, eface = evaluation.point_to_mesh(tq[:0], tv, tf)
    assert empty.shape == (0,) and eface.shape == (0,)


def test_bad_faces_are_counted_not_dereferenced(device):
    v, f = (np.array(x) for x in mesh("grid", 600))
    q = tt(R.queries_for(v, f, 100, seed=5), device)
    lib = _abi.lib()

    def status(vertices, faces, points=q):
        st = torch.cuda.current_stream(device).cuda_stream
        out = evaluation._mesh_distance_enqueue(lib, points, tt(vertices, device), tt(faces, device), True, True, st)
        return out[3].cpu().tolist()
    assert status(v, f) == [600, 0, 0, 1]
    bad = f.copy()
    bad[3, 1], bad[77, 0], bad[599, 2], bad[300] = -1, len(v), 2**31 - 1, (-5, len(v) + 9, 0)
    assert status(v, bad) == [600, 4, 0, 1]
    nonfinite = v.copy()
    nonfinite[f[10, 0], 2], nonfinite[f[400, 1], 0] = np.nan, np.inf
    n_hit = int(np.isin(f, [f[10, 0], f[400, 1]]).any(1).sum())
    assert n_hit >= 2 and status(nonfinite, f) == [600, 0, n_hit, 1]
    n_both = int((np.isin(bad, [f[10, 0], f[400, 1]]).any(1) & ((bad >= 0) & (bad < len(v))).all(1)).sum())
    assert status(nonfinite, bad) == [600, 4, n_both, 1]                # (an index out of range is counted as that alone)
    assert status(v, bad, q[:0]) == [600, 4, 0, 1]                      # no query: the status all the same
    for vertices, faces in ((v, bad), (nonfinite, f)):
        with pytest.raises(ValueError, match="faces have a vertex"):
            evaluation.point_to_mesh(q, tt(vertices, device), tt(faces, device))
    with pytest.raises(ValueError, match="at least one vertex and one face"):
        evaluation.point_to_mesh(q, tt(v, device), tt(f[:0], device))
    d2, face = evaluation.point_to_mesh(q, tt(v, device), tt(f, device))  # the device is fine
    assert bool(torch.isfinite(d2).all())


def test_error_colors_are_the_headers(device):
    rng = np.random.default_rng(4)
    d2 = np.concatenate([rng.uniform(0, 0.7, 5000) ** 2, [0.0, np.nan, np.inf, 0.0625, 0.25], (np.arange(300) / 512.0) ** 2]).astype(np.float32)
    for trunc in (0.5, 0.40625, 2.0):
        got = evaluation.error_colors(tt(d2, device), trunc)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.host().colors(d2, trunc))
    assert evaluation.error_colors(tt(d2[:0], device), 0.5).shape == (0, 3)
    with pytest.raises(ValueError, match="truncation"):
        evaluation.error_colors(tt(d2, device), 0.0)


# ---- evaluate_recon on the sphere ------------------------------------------------------------------------------------
SETTINGS = dict(down_sample_res=0.0, threshold=0.03, truncation_acc=0.05, truncation_com=0.06, mesh_sample_point=20000)
KEYS = ["MAE_accuracy (cm)", "MAE_completeness (cm)", "Chamfer_L1 (cm)", "Precision [Accuracy] (%)", "Recall [Completeness] (%)",
        "F-score (%)", "Inlier_threshold (m)", "Outlier_truncation_acc (m)", "Outlier_truncation_com (m)"]


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """The welded sphere and a reference cloud over its upper part with 1 cm of noise: the reference's bounding box cuts the
    mesh, so crop_to_reference drops faces."""
    import tsdf_ref
    v, f = mesh("sphere", 0)
    rng = np.random.default_rng(17)
    d = rng.normal(0, 1, (6000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[d[:, 2] > 0.2]
    reference = (tsdf_ref.CENTRE + d * (1.0 + rng.normal(0, 0.01, (len(d), 1)))).astype(np.float32)
    return reference, v, f


@pytest.mark.parametrize("crop", [False, True])
def test_exact_completeness_never_exceeds_the_sampled_one(device, crop, monkeypatch):
    """down_sample_res = 0: the estimate cloud is the samples themselves, points ON the faces, so every reference point's
    exact distance is at most its distance to the nearest sample (voxel-averaged samples leave a curved surface and carry
    no such guarantee)."""
    reference, v, f = sphere_scene()
    r, tv, tf = tt(reference, device), tt(v, device), tt(f, device)
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    got = evaluation.evaluate_recon(r, tv, tf, crop_to_reference=crop, seed=1, completeness="exact", error_map=True, **SETTINGS)
    monkeypatch.undo()
    print(f"host reads: {reads}")
    assert len(reads) == 2 and list(got) == KEYS + ["ErrorMap"]
    em = got["ErrorMap"]
    assert torch.equal(em["points"], r) and torch.equal(em["vertices"], tv)
    box = np.concatenate([reference.min(0), reference.max(0)]) if crop else None       # (the z padding is the voxel size: 0)
    kept = f[((v >= box[:3]) & (v <= box[3:])).all(1)[f].all(1)] if crop else f
    assert (len(kept) < len(f)) == crop
    sampled = evaluation.sample_mesh(tv, tf, SETTINGS["mesh_sample_point"], seed=1, crop_box=box)
    d_sampled = np.sqrt(evaluation.nearest(sampled, r, return_index=False)[0].double().cpu().numpy())
    d_exact = np.sqrt(em["point_dist2"].double().cpu().numpy())
    assert (d_exact <= d_sampled * (1 + 1e-5) + 1e-6).all()
    assert (d_exact < 0.5 * d_sampled).mean() > 0.01                    # ... and it is not the same number
    # the exact distances are point_to_mesh's against the kept faces, and the metric is the unchanged sls_nn_stats of them
    direct = evaluation.point_to_mesh(r, tv, tt(kept, device), return_face=False)
    assert torch.equal(direct.view(torch.int32), em["point_dist2"].view(torch.int32))
    tc = np.float32(SETTINGS["truncation_com"])
    terms = np.where(direct.cpu().numpy() < tc * tc, np.sqrt(direct.cpu().numpy()), tc).astype(np.float64)
    assert abs(got["MAE_completeness (cm)"] - 100 * terms.mean()) <= 1e-9 * 100 * terms.mean()
    assert got["Recall [Completeness] (%)"] == int((terms < np.float32(SETTINGS["threshold"])).sum()) / len(terms) * 100.0
    # the accuracy side stays sampled
    m = evaluation.cloud_metrics(r, sampled, threshold=SETTINGS["threshold"], truncation_acc=SETTINGS["truncation_acc"],
                                 truncation_com=SETTINGS["truncation_com"])
    assert got["MAE_accuracy (cm)"] == m["accuracy_m"] * 100 and got["Precision [Accuracy] (%)"] == m["precision"] * 100.0
    assert got["MAE_completeness (cm)"] < m["completeness_m"] * 100
    # the colours are the header's
    assert np.array_equal(em["point_colors"].cpu().numpy(), R.host().colors(em["point_dist2"].cpu().numpy(), SETTINGS["truncation_com"]))
    d_vert = evaluation.nearest(r, tv, return_index=False)[0]
    assert torch.equal(d_vert.view(torch.int32), em["vertex_dist2"].view(torch.int32))
    assert np.array_equal(em["vertex_colors"].cpu().numpy(), R.host().colors(d_vert.cpu().numpy(), SETTINGS["truncation_acc"]))
    assert len(np.unique(em["vertex_colors"].cpu().numpy(), axis=0)) > 20       # (the lower part of the sphere is red)


def test_exact_completeness_does_not_depend_on_the_seed(device):
    reference, v, f = sphere_scene()
    r, tv, tf = tt(reference, device), tt(v, device), tt(f, device)
    kw = dict(SETTINGS, down_sample_res=0.02, mesh_sample_point=5000)
    exact = [evaluation.evaluate_recon(r, tv, tf, seed=s, completeness="exact", **kw) for s in (1, 2)]
    sampled = [evaluation.evaluate_recon(r, tv, tf, seed=s, **kw) for s in (1, 2)]
    assert exact[0]["MAE_completeness (cm)"] == exact[1]["MAE_completeness (cm)"]
    assert exact[0]["Recall [Completeness] (%)"] == exact[1]["Recall [Completeness] (%)"]
    assert sampled[0]["MAE_completeness (cm)"] != sampled[1]["MAE_completeness (cm)"]
    assert exact[0]["MAE_accuracy (cm)"] == sampled[0]["MAE_accuracy (cm)"] != sampled[1]["MAE_accuracy (cm)"]
    assert exact[0]["MAE_completeness (cm)"] < min(s["MAE_completeness (cm)"] for s in sampled)
    assert list(exact[0]) == KEYS


@pytest.mark.parametrize("crop", [False, True])
def test_defaults_change_nothing(device, crop, monkeypatch):
    """The default call: the same two host reads and the metrics of cloud_metrics on the same sampled clouds, bit for bit —
    and error_map alone adds its key without touching a number."""
    reference, v, f = sphere_scene()
    r, tv, tf = tt(reference, device), tt(v, device), tt(f, device)
    kw = dict(SETTINGS, down_sample_res=0.02)
    reads, native = [], []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    monkeypatch.setattr(evaluation, "_mesh_distance_enqueue", lambda *a, **k: native.append(a) or 1 / 0)
    got = evaluation.evaluate_recon(r, tv, tf, crop_to_reference=crop, seed=4, **kw)
    explicit = evaluation.evaluate_recon(r, tv, tf, crop_to_reference=crop, seed=4, completeness="sampled", error_map=False, **kw)
    monkeypatch.undo()
    assert reads == [(12,), (8,), (12,), (8,)] and not native and got == explicit and list(got) == KEYS
    box = None
    if crop:
        box = np.concatenate([reference.min(0) - np.float32([0, 0, 0.02]), reference.max(0) + np.float32([0, 0, 0.02])])
    sampled = evaluation.sample_mesh(tv, tf, kw["mesh_sample_point"], seed=4, crop_box=box)
    m = evaluation.cloud_metrics(evaluation.voxel_down_sample(r, 0.02), evaluation.voxel_down_sample(sampled, 0.02),
                                 threshold=kw["threshold"], truncation_acc=kw["truncation_acc"], truncation_com=kw["truncation_com"])
    assert got == {
        "MAE_accuracy (cm)": m["accuracy_m"] * 100, "MAE_completeness (cm)": m["completeness_m"] * 100,
        "Chamfer_L1 (cm)": m["chamfer_l1_m"] * 100, "Precision [Accuracy] (%)": m["precision"] * 100.0,
        "Recall [Completeness] (%)": m["recall"] * 100.0, "F-score (%)": m["fscore"] * 100.0,
        "Inlier_threshold (m)": kw["threshold"], "Outlier_truncation_acc (m)": kw["truncation_acc"],
        "Outlier_truncation_com (m)": kw["truncation_com"]}
    mapped = evaluation.evaluate_recon(r, tv, tf, crop_to_reference=crop, seed=4, error_map=True, **kw)
    em = mapped.pop("ErrorMap")
    assert mapped == got and em["points"].shape[0] == m["n_completeness"] and em["vertex_colors"].shape == (len(v), 3)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_write_coloured_files(device, tmp_path, monkeypatch, capsys):
    reference, v, f = sphere_scene()
    ply_io.save_point_cloud(tmp_path / "reference.ply", reference, np.zeros_like(reference))
    ply_io.save_mesh(tmp_path / "mesh.ply", v, f)
    r, tv, tf = tt(reference, device), tt(v, device), tt(f, device)
    # tools/mesh_distance.py
    monkeypatch.setattr(sys, "argv", ["mesh_distance.py", str(tmp_path / "reference.ply"), str(tmp_path / "mesh.ply"),
                                      str(tmp_path / "out.ply"), "--truncation", "0.03", "--device", str(device)])
    _tool("mesh_distance").main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    d2 = evaluation.point_to_mesh(r, tv, tf, return_face=False)
    p, n, c = ply_io.load_point_cloud(tmp_path / "out.ply", return_colors=True)
    assert np.array_equal(p, reference) and np.array_equal(c, evaluation.error_colors(d2, 0.03).cpu().numpy())
    assert line["points"] == len(reference) and line["faces"] == len(f) and line["max_m"] == float(d2.double().sqrt().max())
    # tools/eval_recon.py --exact-completeness --error-map
    monkeypatch.setattr(sys, "argv", ["eval_recon.py", str(tmp_path / "reference.ply"), str(tmp_path / "mesh.ply"),
                                      "--down-sample-res", "0.02", "--threshold", "0.03", "--truncation-acc", "0.05",
                                      "--truncation-com", "0.06", "--mesh-sample-point", "20000", "--seed", "3",
                                      "--exact-completeness", "--error-map", str(tmp_path / "map"), "--device", str(device)])
    _tool("eval_recon").main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = evaluation.evaluate_recon(r, tv, tf, seed=3, completeness="exact", error_map=True, **dict(SETTINGS, down_sample_res=0.02))
    em = want.pop("ErrorMap")
    assert line == want
    mv, mf, mc = ply_io.load_mesh(str(tmp_path / "map_accuracy.ply"), return_colors=True)
    assert np.array_equal(mv, v) and np.array_equal(mf, f) and np.array_equal(mc, em["vertex_colors"].cpu().numpy())
    cp, _, cc = ply_io.load_point_cloud(str(tmp_path / "map_completeness.ply"), return_colors=True)
    assert np.array_equal(cp, em["points"].cpu().numpy()) and np.array_equal(cc, em["point_colors"].cpu().numpy())
