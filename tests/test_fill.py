"""Hole filling on the device (sls_mesh_boundary_loops, sls_mesh_fill_holes, mesh_ops.boundary_loops, mesh_ops.fill_holes, the
stage inside mesh_ops.clean_mesh and meshing.mesh_tsdf) against include/sls_fill_math.h run on the host (tests/fill_ref.py):
every case of the table and every setting bit for bit — half-edges, loop numbers, lengths, vertices, faces, the -1 padding and
all 16 status words; what lies beyond the written rows untouched; the same bytes on every run; the stage inside clean_mesh
equal to the composition of the public calls with one host read."""
import functools

import numpy as np
import pytest
import torch

import fill_ref as ref
import mesh_ref
from mesh_ref import bits
from splat_loam_amd import _abi, mesh_ops, meshing
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


def _counts(counts, device):
    return None if counts is None else torch.tensor(list(counts), dtype=torch.int32, device=device)


def _loops(device, f, V, counts):
    """the C entry with pre-filled outputs: (halfedges (3T,2), loop (3T,), loop_edges (T,), status (18,)), as NumPy"""
    lib, T = _abi.lib(), len(f)
    df, dc = _dev(f, device).contiguous(), _counts(counts, device)
    he = torch.full((max(3 * T, 1), 2), SENTINEL_N, dtype=torch.int32, device=device)
    loop = torch.full((max(3 * T, 1),), SENTINEL_N, dtype=torch.int32, device=device)
    edges = torch.full((max(T, 1),), SENTINEL_N, dtype=torch.int32, device=device)
    status = torch.full((18,), 9, dtype=torch.int32, device=device)
    nbytes = int(lib.sls_mesh_boundary_loops_scratch_bytes(V, T))
    hold, ptr = _aligned(nbytes, device)
    _abi.check(lib.sls_mesh_boundary_loops(V, T, df.data_ptr() if T else None, dc.data_ptr() if dc is not None else None, he.data_ptr(),
                                           loop.data_ptr(), edges.data_ptr(), status.data_ptr(), ptr, nbytes,
                                           torch.cuda.current_stream(device).cuda_stream), "sls_mesh_boundary_loops")
    return he.cpu().numpy(), loop.cpu().numpy(), edges.cpu().numpy(), status.cpu().numpy().tolist()


def _fill(device, dv, df, dc, V, T, max_edges, max_size, cap_v, cap_t):
    """the C entry with pre-filled outputs: (vertices (cap_v,3), faces (cap_t,3), status (18,)), as NumPy"""
    lib = _abi.lib()
    out_v = torch.full((max(cap_v, 1), 3), SENTINEL_V, dtype=torch.float32, device=device)
    out_f = torch.full((max(cap_t, 1), 3), SENTINEL_N, dtype=torch.int32, device=device)
    status = torch.full((18,), 9, dtype=torch.int32, device=device)
    nbytes = int(lib.sls_mesh_fill_holes_scratch_bytes(V, T))
    hold, ptr = _aligned(nbytes, device)
    _abi.check(lib.sls_mesh_fill_holes(V, dv.data_ptr() if V else None, T, df.data_ptr() if T else None, dc.data_ptr() if dc is not None else None,
                                       max_edges, max_size, cap_v, out_v.data_ptr(), cap_t, out_f.data_ptr(), status.data_ptr(), ptr, nbytes,
                                       torch.cuda.current_stream(device).cuda_stream), "sls_mesh_fill_holes")
    return out_v.cpu().numpy()[:cap_v], out_f.cpu().numpy()[:cap_t], status.cpu().numpy().tolist()


def _room(case):
    v, f, _ = CASES[case]
    return ref.room(len(v), len(f), 1.0)


@functools.lru_cache(maxsize=None)
def _host(case, setting, room=None):
    v, f, counts = CASES[case]
    return ref.host().fill(v, f, setting[0], setting[1], *(room or _room(case)), counts=counts)


def _check_fill(got, want, cap_v):
    got_v, got_f, status = got
    want_v, want_f, want_s = want
    assert status == want_s + [9, 9]
    nv = want_s[0]
    assert np.array_equal(bits(got_v[:nv]), bits(want_v)) and np.array_equal(got_f, want_f)     # the -1 padding included
    assert (got_v[nv:cap_v] == SENTINEL_V).all()                    # rows beyond V' are untouched


@pytest.mark.parametrize("case", sorted(CASES))
def test_boundary_loops_equal_header(device, case):
    v, f, counts = CASES[case]
    want_he, want_loop, want_edges, want_s = ref.host().loops(f, len(v), counts)
    got_he, got_loop, got_edges, status = _loops(device, f, len(v), counts)
    assert status == want_s + [9, 9], case
    B, L = status[2], status[3]
    assert np.array_equal(got_he[:B], want_he) and np.array_equal(got_loop[:B], want_loop) and np.array_equal(got_edges[:L], want_edges)
    assert (got_he[B:] == SENTINEL_N).all() and (got_loop[B:] == SENTINEL_N).all() and (got_edges[L:] == SENTINEL_N).all()
    again = _loops(device, f, len(v), counts)                       # the same on every run
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], (got_he, got_loop, got_edges))) and again[3] == status


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_equals_header(device, case):
    v, f, counts = CASES[case]
    V, T = len(v), len(f)
    cap_v, cap_t = _room(case)
    dv, df, dc = _dev(v, device).contiguous(), _dev(f, device).contiguous(), _counts(counts, device)
    for setting in SETTINGS:
        got = _fill(device, dv, df, dc, V, T, setting[0], setting[1], cap_v, cap_t)
        _check_fill(got, _host(case, setting), cap_v)
        again = _fill(device, dv, df, dc, V, T, setting[0], setting[1], cap_v, cap_t)     # the same bytes on every run
        assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(again[1], got[1]) and again[2] == got[2], (case, setting)


def test_no_room_fills_nothing(device):
    """cap_triangles (then cap_vertices) one short of the need: the live input copied, the overflow word 1, both needs reported"""
    v, f, _ = CASES["sphere_caps"]
    V, T = len(v), len(f)
    dv, df = _dev(v, device).contiguous(), _dev(f, device).contiguous()
    need = _host("sphere_caps", (128, 0.0))[2]
    for room in ((need[12], need[13] - 1), (need[12] - 1, need[13]), (need[12], need[13])):
        got = _fill(device, dv, df, None, V, T, 128, 0.0, *room)
        want = _host("sphere_caps", (128, 0.0), room)
        _check_fill(got, want, room[0])
        over = room != (need[12], need[13])
        assert got[2][14] == int(over) and got[2][12:14] == need[12:14] and got[2][4] == (0 if over else 6)
        if over:
            assert np.array_equal(bits(got[0][:V]), bits(v)) and np.array_equal(got[1][:T], f) and (got[1][T:] == -1).all()


def test_public_calls(device):
    v, f, _ = CASES["sphere_caps"]
    dv, df = _dev(v, device), _dev(f, device)
    he, loop, edges, det = mesh_ops.boundary_loops(df.long(), len(v), details=True)                 # int64 faces are converted
    want_he, want_loop, want_edges, want_s = ref.host().loops(f, len(v))
    assert he.dtype == loop.dtype == edges.dtype == torch.int32 and he.shape == (264, 2) and loop.shape == (264,) and edges.shape == (6,)
    assert np.array_equal(he.cpu().numpy(), want_he) and np.array_equal(loop.cpu().numpy(), want_loop)
    assert sorted(edges.tolist()) == sorted(ref.SPHERE_LOOPS) and np.array_equal(edges.cpu().numpy(), want_edges)
    assert det == dict(halfedges=264, loops=6, open_halfedges=0, complex_vertices=0, degenerate=0, out_of_range=0)
    assert len(mesh_ops.boundary_loops(df, len(v))) == 3
    out_v, out_f, det = mesh_ops.fill_holes(dv, df.long(), max_edges=128, details=True)
    want_v, want_f, want_s = ref.host().fill(v, f, 128, 0.0)
    assert out_v.dtype == torch.float32 and out_f.dtype == torch.int32 and out_v.shape == (len(v) + 5, 3) and out_f.shape == (want_s[1], 3)
    assert np.array_equal(bits(out_v.cpu().numpy()), bits(want_v)) and np.array_equal(out_f.cpu().numpy(), want_f[:want_s[1]])
    assert [det[k] for k in ref.STATUS] == want_s[:15] and set(det) == set(ref.STATUS)
    # the sphere closes: no boundary edge, no non-manifold edge, V - E + F = 2, every new vertex inside its loop's box
    closed = mesh_ops.cluster_triangles(out_f, out_v.shape[0], details=True)[2]
    assert closed["boundary_edges"] == 0 and closed["nonmanifold_edges"] == 0 and mesh_ref.euler(out_f.cpu().numpy()) == 2
    plain = mesh_ops.fill_holes(dv, df)                             # the defaults: 64 edges, no size limit
    assert len(plain) == 2 and mesh_ops.cluster_triangles(plain[1], plain[0].shape[0], details=True)[2]["boundary_edges"] == 154
    sized = mesh_ops.fill_holes(dv, df, max_edges=128, max_size=ref.SIZE_SPLIT, details=True)[2]
    assert (sized["filled"], sized["skipped_size"]) == (2, 4)
    # too little room: the error names what is needed, and a retry with that much gives the header's result
    mv, mf, _ = CASES["many_loops"]
    dmv, dmf = _dev(mv, device), _dev(mf, device)
    need = ref.host().fill(mv, mf, 64, 0.0, *ref.room(len(mv), len(mf), 1.0))
    with pytest.raises(ValueError, match=f"{need[2][13]} triangles and {need[2][12]} vertices"):
        mesh_ops.fill_holes(dmv, dmf)
    retry = mesh_ops.fill_holes(dmv, dmf, capacity=(need[2][13] - len(mf)) / len(mf), details=True)
    assert retry[2]["filled"] == ref.MANY_CELLS ** 2 and retry[2]["overflow"] == 0
    assert np.array_equal(bits(retry[0].cpu().numpy()), bits(need[0])) and np.array_equal(retry[1].cpu().numpy(), need[1][:need[2][1]])
    bv, bf = CASES["tet_open"][0], np.array([(0, 1, 2), (0, 9, 1)], np.int32)
    with pytest.raises(ValueError, match="outside the vertices"):
        mesh_ops.fill_holes(_dev(bv, device), _dev(bf, device))
    with pytest.raises(ValueError, match="outside the vertices"):
        mesh_ops.boundary_loops(_dev(bf, device), len(bv))
    with pytest.raises(ValueError, match="max_edges"):
        mesh_ops.fill_holes(dv, df, max_edges=2)
    empty = mesh_ops.fill_holes(dv, torch.zeros((0, 3), dtype=torch.int32, device=device), details=True)     # T = 0
    assert torch.equal(empty[0].view(torch.int32), dv.view(torch.int32)) and empty[1].shape == (0, 3) and empty[2]["halfedges"] == 0
    none = mesh_ops.boundary_loops(torch.zeros((0, 3), dtype=torch.int32, device=device), 5)
    assert none[0].shape == (0, 2) and none[1].shape == (0,) and none[2].shape == (0,)


def _scene():
    """the sphere with its caps as a soup, a far sphere and floaters: welded, the selection keeps the sphere with its six holes"""
    v, f, _ = CASES["sphere_caps"]
    soup = np.concatenate([v[f.reshape(-1)], mesh_ref.sphere_soup(0.5, mesh_ref.FAR), mesh_ref.floater_scene()[0][-15:]])
    return soup, np.arange(len(soup), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("kw", ({}, {"fill_max_size": ref.SIZE_SPLIT}, {"simplify": 0.25}, {"smooth": 2}, {"simplify": 0.25, "smooth": 2},
                                {"keep_clusters": None}))
def test_clean_mesh_with_fill_is_the_composition(device, kw, monkeypatch):
    """clean_mesh(fill_holes=n) = clean_mesh() -> fill_holes(n) -> [simplify] -> [smooth] -> vertex_normals, with ONE host read
    (counted the way test_smooth counts them: every Tensor.cpu() call)"""
    soup, faces = _scene()
    ds, df = _dev(soup, device), _dev(faces, device)
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    v, f, n, det = mesh_ops.clean_mesh(ds, df, fill_holes=128, details=True, **kw)
    monkeypatch.undo()
    print(f"host reads: {reads}")
    assert len(reads) == 1
    first = {k: x for k, x in kw.items() if k == "keep_clusters"}
    v0, f0, det0 = mesh_ops.clean_mesh(ds, df, normals=False, details=True, **first)
    v1, f1, det1 = mesh_ops.fill_holes(v0, f0, max_edges=128, max_size=kw.get("fill_max_size"), details=True)
    if "simplify" in kw:
        v1, f1 = mesh_ops.simplify_vertex_clustering(v1, f1, kw["simplify"])
    if "smooth" in kw:
        v1 = mesh_ops.smooth(v1, f1, kw["smooth"])
    n1 = mesh_ops.vertex_normals(v1, f1)
    assert torch.equal(f, f1) and torch.equal(v.view(torch.int32), v1.view(torch.int32)) and torch.equal(n.view(torch.int32), n1.view(torch.int32))
    # the stage ran at capacity behind the selection: its counts are those of the public call on the sliced mesh
    same = [k for k in ref.STATUS if k not in ("degenerate", "out_of_range")]
    assert {k: det["fill"][k] for k in same} == {k: det1[k] for k in same}
    # the sphere's six loops (two under the size limit); without the selection the five floating triangles are loops of three too
    assert det["fill"]["filled"] == (2 if "fill_max_size" in kw else 11 if "keep_clusters" in kw else 6) and det["fill"]["vertices"] > v0.shape[0]
    skip = ("cluster_count", "labels", "simplify", "smooth", "fill")
    assert {k: det[k] for k in det0 if k not in skip} == {k: det0[k] for k in det0 if k not in skip}
    if not kw:                                                      # ... and the header's, on the host
        want_v, want_f, want_s = ref.host().fill(v0.cpu().numpy(), f0.cpu().numpy(), 128, 0.0)
        assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f[:want_s[1]])
        assert mesh_ops.cluster_triangles(f, v.shape[0], details=True)[2]["boundary_edges"] == 0


def test_clean_mesh_without_fill_is_unchanged(device):
    """fill_holes=None: the stage-by-stage composition weld -> keep_clusters -> vertex_normals, and mesh_ref's restatement"""
    soup, faces = _scene()
    ds, df = _dev(soup, device), _dev(faces, device)
    wv, wf = mesh_ops.weld(ds)
    kv, kf = mesh_ops.keep_clusters(wv, wf, 1, 50)
    kn = mesh_ops.vertex_normals(kv, kf)
    want_v, want_f, _ = mesh_ref.clean(soup, faces, 1, 50)
    for kw in ({}, {"fill_holes": None, "fill_max_size": 0.1, "fill_capacity": 3.0}):
        v, f, n, det = mesh_ops.clean_mesh(ds, df, details=True, **kw)
        assert torch.equal(v.view(torch.int32), kv.view(torch.int32)) and torch.equal(f, kf) and torch.equal(n.view(torch.int32), kn.view(torch.int32))
        assert np.array_equal(bits(v.cpu().numpy()), bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
        assert "fill" not in det and "smooth" not in det and "simplify" not in det


def test_clean_mesh_reports_too_little_room(device):
    mv, mf, _ = CASES["many_loops"]
    with pytest.raises(ValueError, match="triangles and .* vertices are needed"):
        mesh_ops.clean_mesh(_dev(mv, device), _dev(mf, device), fill_holes=64, keep_clusters=None)
    v, f, n, det = mesh_ops.clean_mesh(_dev(mv, device), _dev(mf, device), fill_holes=64, fill_capacity=1.0, keep_clusters=None, details=True)
    assert det["fill"]["filled"] == ref.MANY_CELLS ** 2 and f.shape[0] == len(mf) + 4 * ref.MANY_CELLS ** 2


def test_mesh_tsdf_fill_end_to_end(device, tmp_path):
    """mesh_tsdf(fill_holes=) on the small synthetic graph = clean_mesh applied to its soup"""
    _write_room(tmp_path, True)
    sv, sf = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device)
    v, f, n, det = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True, keep_clusters=1, normals=True,
                                     fill_holes=64, fill_max_size=1.0)
    want = mesh_ops.clean_mesh(sv, sf, keep_clusters=1, fill_holes=64, fill_max_size=1.0, details=True)
    fill = det["clean"]["fill"]
    print(f"room: {int(sf.shape[0])} triangles in the soup, {fill['halfedges']} boundary half-edges, {fill['loops']} loops, {fill['filled']} filled, "
          f"{fill['skipped_edges']} too long, {fill['skipped_size']} too large, {fill['open_halfedges']} open half-edges; clean {det['stage_ms']['clean']:.2f} ms")
    assert torch.equal(v.view(torch.int32), want[0].view(torch.int32)) and torch.equal(f, want[1]) and torch.equal(n.view(torch.int32), want[2].view(torch.int32))
    assert fill == want[3]["fill"] and fill["overflow"] == 0 and fill["triangles"] == f.shape[0] and bool(torch.isfinite(v).all())
    only = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, fill_holes=64)          # the argument alone runs the clean stage
    assert only[0].shape[0] < sv.shape[0] and only[1].shape[0] >= sf.shape[0]
