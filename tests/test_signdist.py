"""sls_mesh_pseudonormals / sls_mesh_signed_distance / sls_signed_stats / sls_signed_error_colors and
splat_loam_amd.evaluation (mesh_pseudonormals, signed_distance, signed_error_colors, evaluate_recon(signed=)) on the device,
against include/sls_signdist_math.h compiled for the host (tests/signdist_ref.py: the tables, and a brute force over all
faces) bit for bit, and against analytic truth."""
import functools
import struct

import numpy as np
import pytest
import torch

import meshdist_ref
import nn_ref
import signdist_ref as R
from splat_loam_amd import _abi, evaluation

pytestmark = pytest.mark.gpu
f32 = np.float32


def tt(a, device):
    return torch.tensor(np.ascontiguousarray(a), device=device)


def _uniform(lo, hi, n, seed):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, queries, host tables, host query result): computed once per mesh"""
    if name == "blade":
        (v, f), q = R.blade(), R.blade_queries(4000, seed=3)
    elif name == "cube":
        (v, f), q = R.cube(), R.cube_queries()
    elif name == "l_prism":
        (v, f), q = R.l_prism(), _uniform([-0.5, -0.5, -0.5], [2.5, 2.5, 1.5], 4000, 4)
    elif name == "sheet":
        v, f = R.folded_sheet()
        q = np.concatenate([meshdist_ref.queries_for(v, f, 1000, seed=5), _uniform([-1, -0.5, -2.5], [1, 2, 0.5], 2000, 6)])
    elif name == "defects":
        v, f = R.defects()
        q = np.concatenate([meshdist_ref.queries_for(v, f, 1000, seed=7), _uniform([-0.5, -0.5, -0.5], [1.6, 1.6, 2.5], 2000, 8)])
    elif name == "icosphere":
        v, f = R.icosphere()
        q = np.concatenate([meshdist_ref.queries_for(v, f, 8000, seed=9), _uniform([-1.5] * 3, [1.5] * 3, 12000, 10)])
    else:
        raise KeyError(name)
    tables = R.host().tables(v, f)
    return v, f, q, tables, R.host().query(v, f, tables, q)


def run(device, v, f, q, pn=None):
    out = evaluation.signed_distance(tt(q, device), tt(v, device), tt(f, device), return_face=True, return_closest=True,
                                     return_feature=True, pseudonormals=pn)
    sd, face, closest, feature = out
    assert sd.dtype == torch.float32 and face.dtype == torch.int32 and closest.dtype == torch.float32 and feature.dtype == torch.uint8
    assert sd.shape == face.shape == feature.shape == (len(q),) and closest.shape == (len(q), 3)
    return tuple(x.cpu().numpy() for x in out)


@pytest.mark.parametrize("name", ["blade", "cube", "l_prism", "sheet", "defects", "icosphere"])
def test_device_equals_the_header_bit_for_bit(device, name):
    v, f, q, (hfn, hen, hvn, hstatus), (hsd, hface, hclosest, hfeature) = case(name)
    vt, ft = tt(v, device), tt(f, device)
    pn, details = evaluation.mesh_pseudonormals(vt, ft, return_details=True)
    status = pn.status.cpu().numpy().astype(np.uint32)
    print(f"{name}: F={len(f)} Mq={len(q)} status {status.tolist()} features {np.bincount(hfeature, minlength=7).tolist()}")
    assert status.tolist() == hstatus.tolist()
    assert details == {"degenerate_faces": hstatus[0], "zero_area_faces": hstatus[3], "boundary_edges": hstatus[4],
                       "nonmanifold_edges": hstatus[5], "inconsistent_edges": hstatus[6]}
    assert pn.face_normals.shape == (len(f), 3) and pn.edge_normals.shape == (len(f), 3, 3) and pn.vertex_normals.shape == (len(v), 3)
    assert pn.face_normals.cpu().numpy().tobytes() == hfn.tobytes()
    assert pn.edge_normals.cpu().numpy().tobytes() == hen.tobytes()
    assert pn.vertex_normals.cpu().numpy().tobytes() == hvn.tobytes()
    sd, face, closest, feature = run(device, v, f, q)
    assert np.array_equal(face, hface) and np.array_equal(feature, hfeature)
    assert sd.tobytes() == hsd.tobytes() and closest.tobytes() == hclosest.tobytes()
    assert len(f) < 300 or len(np.unique(feature)) == 7                 # (every kind of feature is met on the larger meshes)
    # consistency with point_to_mesh: the magnitude is the root of its dist2, the face and the closest point are its own
    d2, pface, pclosest = evaluation.point_to_mesh(tt(q, device), vt, ft, return_face=True, return_closest=True)
    assert np.abs(sd).tobytes() == np.sqrt(d2.cpu().numpy()).tobytes()
    assert np.array_equal(face, pface.cpu().numpy()) and closest.tobytes() == pclosest.cpu().numpy().tobytes()
    # repeatability, and tables built before give what building afresh gives
    again, reused = run(device, v, f, q), run(device, v, f, q, pn=pn)
    pn2 = evaluation.mesh_pseudonormals(vt, ft)
    for a, b in ((pn.face_normals, pn2.face_normals), (pn.edge_normals, pn2.edge_normals), (pn.vertex_normals, pn2.vertex_normals)):
        assert torch.equal(a, b)
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip((sd, face, closest, feature), again, reused))
    # the optional outputs are optional
    alone = evaluation.signed_distance(tt(q, device), vt, ft, pseudonormals=pn)
    assert isinstance(alone, torch.Tensor) and alone.cpu().numpy().tobytes() == sd.tobytes()
    if name == "cube":
        # queries ON the surface: the non-negative zero, its sign bit clear
        on = (np.abs(q - 9 / 16).max(1) == 0.5)
        assert on.sum() > 1000 and not sd[on].view(np.uint32).any()
        inside = np.abs(q - 9 / 16).max(1) < 0.5
        assert (sd[inside] < 0).all() and (sd[~inside & ~on] > 0).all()


@pytest.mark.parametrize("name", ["blade", "l_prism", "icosphere"])
def test_sign_equals_analytic_truth(device, name):
    """Every query at least 1e-3 m (float64, to the returned face: never less than the true distance, so no query the rule
    includes is left out) from the surface has the analytic sign; at most 0.5 % of the queries are nearer."""
    v, f, q, _, _ = case(name)
    if name == "icosphere":
        q = q[8000:]                                                    # the uniform ones: the others lie ON it by construction
    sd, face, closest, feature = run(device, v, f, q)
    inside = R.l_prism_inside(q) if name == "l_prism" else R.inside_convex(q, v, f)
    d64 = np.sqrt(meshdist_ref.triangle64(q, *(v[f[face, k]] for k in range(3)))[0])
    far = d64 >= 1e-3
    wrong = ((sd < 0) != inside) & far
    fn = R.host().tables(v, f)[0].astype(np.float64)[face]
    naive = ((((q.astype(np.float64) - closest) * fn).sum(1) < 0) != inside) & far
    print(f"{name}: {int((~far).sum())} of {len(q)} excluded ({(~far).mean():.3%}), wrong signs {int(wrong.sum())}, "
          f"by the face normal alone {int(naive.sum())}")
    assert (~far).mean() <= 0.005
    assert not wrong.any()
    assert 0 < inside.sum() < len(q)
    if name == "blade":
        assert naive.mean() > 0.05


def _signed_stats(device, sd, truncation):
    lib = _abi.lib()
    words = torch.empty((4,), dtype=torch.int64, device=device)
    scratch, aligned, nbytes = evaluation._scratch(32768, device)
    with torch.cuda.device(device):
        _abi.check(lib.sls_signed_stats(len(sd), sd.data_ptr() if len(sd) else None, truncation, words.data_ptr(), aligned, nbytes,
                                        torch.cuda.current_stream(device).cuda_stream), "sls_signed_stats")
    w = words.cpu().tolist()
    return w[0], w[1], struct.unpack("<d", struct.pack("<q", w[2]))[0], w[3]


@pytest.mark.parametrize("M", [0, 1, 255, 257, 300000])
def test_signed_stats(device, M):
    """n, the negative ones and the float64 sum within the truncation; 300 000 entries are more than the 1024 blocks of
    the partial sums hold at one entry a thread.  The same bits on every run."""
    rng = np.random.default_rng(M)
    sd = rng.normal(0, 0.4, M).astype(f32)
    if M > 16:
        sd[:8] = [np.nan, np.inf, -np.inf, 0.5, -0.5, 0.0, -0.0, np.nextafter(f32(0.5), f32(0))]
    t = tt(sd, device)
    n, neg, total, m = _signed_stats(device, t, 0.5)
    wn, wneg, wtotal = R.stats(sd, 0.5)
    assert (n, neg, m) == (wn, wneg, M)
    assert abs(total - wtotal) <= 1e-12 * max(1.0, float(np.abs(sd[np.isfinite(sd)]).sum()))
    assert _signed_stats(device, t, 0.5) == (n, neg, total, m)


@pytest.mark.parametrize("M", nn_ref.STATS_ORDER_SIZES)
def test_signed_stats_sum_is_the_documented_order(device, M):
    """Word 2 bit for bit: the float64 sum is taken in the order of sls_nn_stats (nn_ref.device_sum), on terms spread over
    thirty decades, seeded so that other orders give other bits (tests/test_nn_host.py shows that on this very data)."""
    sd = nn_ref.stats_order_signed(M)
    n, neg, total, m = _signed_stats(device, tt(sd, device), 0.5)
    wn, wneg, wtotal = R.stats_device_order(sd, 0.5)
    print(f"M={M}: n {n} negative {neg} sum {total!r} (restated {wtotal!r}, NumPy's order {R.stats(sd, 0.5)[2]!r})")
    assert (n, neg, m) == (wn, wneg, M) and 0 < n <= M
    assert struct.pack("<d", total) == struct.pack("<d", wtotal)


def test_signed_colours_are_the_headers(device):
    rng = np.random.default_rng(2)
    for trunc in (0.5, 0.40625, 3.3, 1e-3):
        sd = np.concatenate([rng.uniform(-1.5 * trunc, 1.5 * trunc, 20000), [0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -3e38],
                             np.arange(-300, 300) / 256.0 * trunc]).astype(f32)
        got = evaluation.signed_error_colors(tt(sd, device), trunc)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.host().colors(sd, trunc))
    assert evaluation.signed_error_colors(torch.zeros((0,), device=device), 0.5).shape == (0, 3)
    with pytest.raises(ValueError):
        evaluation.signed_error_colors(torch.zeros((3,), device=device), 0.0)


@functools.lru_cache(maxsize=None)
def _unit_sphere_points(n=20000):
    p = np.random.default_rng(21).normal(0, 1, (n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(f32)


def test_the_use_case_a_shrunk_and_an_inflated_sphere(device):
    """Points on the unit sphere against the icosphere scaled by 0.98 and by 1.02: the unsigned means cannot tell the two
    apart, the signed means are +0.02 and -0.02.
    The icosphere here is the one whose SURFACE has the mean radius 1 (signdist_ref.mean_radius: a property of the mesh
    alone, float64): with its vertices on the unit sphere instead, its facets lie 0.72 mm inside the sphere in the mean, at
    either scale, which moves BOTH unsigned means the same way — measured so: 0.02070 at 0.98 and 0.01926 at 1.02, apart
    by 1.44 mm, twice that sagitta and nothing the sign has a part in."""
    v, f = R.icosphere()
    v = v.astype(np.float64) / R.mean_radius(v, f)
    assert abs(R.mean_radius(v, f) - 1.0) <= 1e-12 and 1e-4 < np.linalg.norm(v, axis=1).min() - 1.0 < 1e-3
    p = tt(_unit_sphere_points(), device)
    res = {}
    for s in (0.98, 1.02):
        vt, ft = tt((v.astype(np.float64) * s).astype(f32), device), tt(f, device)
        sd = evaluation.signed_distance(p, vt, ft)
        d2 = evaluation.point_to_mesh(p, vt, ft, return_face=False)
        n, neg, total, m = _signed_stats(device, sd, 0.5)
        assert n == m == len(p)
        res[s] = (float(d2.sqrt().double().mean()), total / n, neg / n)
        print(f"scale {s}: unsigned mean {res[s][0]:.5f}, signed mean {res[s][1]:+.5f}, share behind {res[s][2]:.4f}")
    assert abs(res[0.98][0] - res[1.02][0]) <= 1e-3
    assert abs(res[0.98][1] - 0.02) <= 2e-3 and abs(res[1.02][1] + 0.02) <= 2e-3
    assert res[0.98][2] <= 0.001 and res[1.02][2] >= 0.999


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    return a == b or (isinstance(a, float) and a != a and b != b)


@pytest.mark.parametrize("completeness", ["sampled", "exact"])
def test_evaluate_recon_signed(device, completeness):
    v, f = R.icosphere(3)
    vt, ft = tt((v.astype(np.float64) * 0.98).astype(f32), device), tt(f, device)
    ref = tt(_unit_sphere_points(), device)
    kw = dict(down_sample_res=0.0, mesh_sample_point=20000, seed=3, completeness=completeness)
    for error_map in (False, True):
        base = evaluation.evaluate_recon(ref, vt, ft, error_map=error_map, **kw)
        off = evaluation.evaluate_recon(ref, vt, ft, error_map=error_map, signed=False, **kw)
        on = evaluation.evaluate_recon(ref, vt, ft, error_map=error_map, signed=True, **kw)
        assert "Signed" not in base and _same(base, off)                # signed=False: the dictionary it gave, every value
        s = on.pop("Signed")
        extra = {k: on["ErrorMap"].pop(k) for k in ("point_signed", "point_colors_signed")} if error_map else {}
        assert _same(on, base)                                          # ... and True adds to it, changing nothing else
        assert set(s) == {"mean_m", "share_behind", "n", "degenerate_faces", "zero_area_faces", "boundary_edges", "nonmanifold_edges",
                          "inconsistent_edges"}
        assert s["n"] == len(ref) and s["share_behind"] <= 0.001 and abs(s["mean_m"] - 0.02) <= 5e-3      # (1 280 facets: their sagitta adds up to 2.5 mm)
        assert (s["degenerate_faces"], s["zero_area_faces"], s["boundary_edges"], s["nonmanifold_edges"], s["inconsistent_edges"]) == (0,) * 5
        if error_map:
            sd = evaluation.signed_distance(ref, vt, ft)
            assert torch.equal(extra["point_signed"], sd)
            assert torch.equal(extra["point_colors_signed"], evaluation.signed_error_colors(sd, 0.5))
            assert np.array_equal(extra["point_colors_signed"].cpu().numpy(), R.host().colors(sd.cpu().numpy(), 0.5))
            assert np.abs(sd.cpu().numpy()).tobytes() == np.sqrt(on["ErrorMap"]["point_dist2"].cpu().numpy()).tobytes()
            wn, wneg, wtotal = R.stats(sd.cpu().numpy(), 0.5)
            assert s["n"] == wn and s["share_behind"] == wneg / wn and abs(s["mean_m"] - wtotal / wn) <= 1e-12


def test_bad_meshes_are_refused_with_point_to_meshs_messages(device):
    v, f = R.cube()
    p = tt(R.cube_queries()[:10], device)
    bad = np.array(f)
    bad[2, 1] = 99
    with pytest.raises(ValueError, match="1 faces have a vertex index outside the vertices"):
        evaluation.signed_distance(p, tt(v, device), tt(bad, device))
    with pytest.raises(ValueError, match="1 faces have a vertex index outside the vertices"):
        evaluation.mesh_pseudonormals(tt(v, device), tt(bad, device))
    nv = np.array(v)
    nv[0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        evaluation.signed_distance(p, tt(nv, device), tt(f, device))
    with pytest.raises(ValueError, match="at least one vertex and one face"):
        evaluation.signed_distance(p, tt(v, device), torch.zeros((0, 3), dtype=torch.int32, device=device))
    # no query is fine
    assert evaluation.signed_distance(torch.zeros((0, 3), device=device), tt(v, device), tt(f, device)).shape == (0,)


def test_a_fused_mesh_looks_to_the_observed_side(device):
    """The sphere tests/test_tsdf.py fuses (tsdf positive outside, where the sensor is): points moved 5 cm towards the sensor
    from the surface are positive, points moved 5 cm away from it negative — the documented meaning of the sign for this
    tree's own mesher."""
    import test_tsdf
    from tsdf_ref import CENTRE
    blocks, t, w, _, _ = test_tsdf._sphere()
    vertices, faces = test_tsdf._volume(device, blocks, t, w).extract(weld=True)
    pn, details = evaluation.mesh_pseudonormals(vertices, faces, return_details=True)
    print("fused sphere:", tuple(vertices.shape), tuple(faces.shape), details)
    assert details["boundary_edges"] == 0 and details["nonmanifold_edges"] == 0 and details["inconsistent_edges"] == 0
    d = _unit_sphere_points(4000).astype(np.float64)
    for radius, sign in ((1.05, 1.0), (0.95, -1.0)):
        sd = evaluation.signed_distance(tt((CENTRE + radius * d).astype(f32), device), vertices, faces, pseudonormals=pn).cpu().numpy()
        assert (np.sign(sd) == sign).all()
        assert np.abs(np.abs(sd) - 0.05).max() <= 0.01                  # (marching tetrahedra on a 12.5 cm lattice)
