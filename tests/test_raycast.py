"""The ray caster on the GPU (sls_mesh_rayindex_build, sls_mesh_raycast, evaluation.cast_rays / mesh_ray_index /
render_mesh, meshing.mesh_depth_check) against include/sls_raycast_math.h run on the host over ALL faces
(raycast_ref.host().cast), bit for bit: t, face and uv at the seams of the index and of the wave, with loose boxes,
duplicate faces, axis-parallel rays and a bounded range; closed meshes from inside with no miss; a box room against its
analytic distances; the range image's pixel convention; the depth check and the tools end to end."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshdist_ref
import raycast_ref as R
from splat_loam_amd import _abi, evaluation, meshing, ply_io, synth, traj_io
from splat_loam_amd.renderer import depth_to_points
from splat_loam_amd.scene import Camera

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tt(a, device):
    return torch.tensor(np.ascontiguousarray(a), device=device)


def run(device, o, d, v, f, **kw):
    t, face, uv = evaluation.cast_rays(tt(o, device), tt(d, device), tt(v, device), tt(f, device), return_face=True, return_uv=True, **kw)
    assert t.dtype == torch.float32 and face.dtype == torch.int32 and uv.dtype == torch.float32
    assert t.shape == face.shape == (len(o),) and uv.shape == (len(o), 2)
    return t.cpu().numpy(), face.cpu().numpy(), uv.cpu().numpy()


def same_bits(got, want):
    return all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def mesh(name, F):
    if name == "grid":                      # the first F faces of the 92 x 92 grid, in its seeded random face order
        v, f = meshdist_ref.grid_mesh()
        return v, f[:F]
    if name == "loose":                     # the grid plus ONE triangle spanning its whole bounding box: loose boxes
        v, f = meshdist_ref.grid_mesh()
        lo, hi = v.min(0), v.max(0)
        big = np.array([lo, [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]]], np.float32)
        return np.concatenate([v, big]), np.concatenate([f[:F - 1], [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def brute(name, F, Mr):
    """(o, d, v, f, the brute force's (t, face, uv)): computed once per case"""
    v, f = mesh(name, F)
    o, d = R.rays_for(v, f, Mr, seed=1000 * F + Mr)
    return o, d, v, f, R.host().cast(v, f, o, d)


def check(device, name, F, Mr):
    o, d, v, f, want = brute(name, F, Mr)
    got = run(device, o, d, v, f)
    assert np.array_equal(got[1], want[1]), f"{name} F={F} Mr={Mr}: {(got[1] != want[1]).sum()} faces differ"
    assert same_bits(got, want)
    assert same_bits(run(device, o, d, v, f), got)              # two runs give identical bytes
    return got


# the seams of the traversal: a single face; the run of 32; the box of 256 — against the wave's seams on the ray side
@pytest.mark.parametrize("Mr", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("F", [1, 31, 32, 33, 255, 256, 257])
def test_grid_at_the_seams(device, F, Mr):
    check(device, "grid", F, Mr)


@pytest.mark.parametrize("Mr", [1, 65, 256])
def test_grid_second_chunk_of_boxes(device, Mr):
    assert len(meshdist_ref.grid_mesh()[1]) == 16928 > 64 * 256
    t, face, _ = check(device, "grid", 16928, Mr)
    assert Mr == 1 or 0 < (face >= 0).sum() < Mr            # hits and misses both


@pytest.mark.parametrize("F,Mr", [(300, 65), (16928, 256)])
def test_one_huge_triangle_among_small_ones(device, F, Mr):
    t, face, _ = check(device, "loose", F, Mr)
    print(f"rays that hit the huge triangle first: {(face == F - 1).sum()} of {Mr}; others: {((face >= 0) & (face != F - 1)).sum()}")
    assert 0 < (face == F - 1).sum() < Mr


def test_duplicate_faces_lowest_index(device):
    """Every face twice, the copies in another order behind the originals: equal t BITS, so the lower index of the pair
    must be named whichever run or box each copy falls into."""
    v, f0 = meshdist_ref.grid_mesh()
    f0 = f0[:1500]
    perm = np.random.default_rng(3).permutation(len(f0))
    f = np.concatenate([f0, f0[perm]])
    first = np.concatenate([np.arange(len(f0)), perm])                   # the lowest index holding the same face
    o, d = R.rays_for(v, f0, 512, seed=77)
    t, face, uv = run(device, o, d, v, f)
    hit = face >= 0
    assert hit.sum() > 100 and np.array_equal(face[hit], first[face[hit]])
    single = run(device, o, d, v, f0)
    assert np.array_equal(face, single[1]) and t.tobytes() == single[0].tobytes()


def test_axis_parallel_rays_graze_box_faces(device):
    """Zero direction components, origins on the grid's own coordinates: the rays run IN the faces of the boxes and
    sub-boxes (whose faces lie on vertex coordinates) and through vertices and edges exactly."""
    v, f = mesh("grid", 16928)
    rng = np.random.default_rng(21)
    pick = v[rng.integers(0, len(v), 96)].astype(np.float64)
    o, d = [], []
    for axis in range(3):
        for sgn in (1.0, -1.0):
            p = pick[(2 * axis + (sgn > 0)) * 16:][:16].copy()
            p[:, axis] -= sgn * 16.0                                       # start outside, on the vertex's own line
            e = np.zeros(3)
            e[axis] = sgn
            o.append(p)
            d.append(np.broadcast_to(e, p.shape))
    one_zero = pick[:32].copy()
    one_zero[:, 0] -= 4.0
    one_zero[:, 2] += 4.0
    o.append(one_zero)
    d.append(np.broadcast_to(np.array([1.0, 0.0, -1.0]), one_zero.shape))
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)
    want = R.host().cast(v, f, o, d)
    got = run(device, o, d, v, f)
    print(f"axis-parallel rays: {(want[1] >= 0).sum()} of {len(o)} hit")
    assert (want[1] >= 0).sum() >= 64                                      # the rays along z and the slanted ones meet the sheet
    assert np.array_equal(got[1], want[1]) and same_bits(got, want)


def test_t_min_t_max(device):
    """Through a closed cube from outside: two walls.  A hit just outside either end of the range is not returned, and
    the next one is."""
    v, f = R.cube(8, seed=3)
    rng = np.random.default_rng(5)
    o = np.tile(np.array([[-9.0, 0.3, -0.2]], np.float32), (70, 1))
    d = np.concatenate([np.ones((70, 1)), rng.uniform(-0.3, 0.3, (70, 2))], 1).astype(np.float32)
    t_in, face_in, _ = run(device, o, d, v, f)
    assert (face_in >= 0).all()
    up = lambda x: np.nextafter(x, np.float32(np.inf))
    down = lambda x: np.nextafter(x, np.float32(0))
    # the per-ray ends differ, so rays go one range at a time in groups: use the extremes of the entries
    lo = float(up(t_in.max()))                                            # just beyond every entry: the exits
    t_out, face_out, _ = run(device, o, d, v, f, t_min=lo)
    assert (face_out >= 0).all() and (t_out > t_in).all() and (face_out != face_in).all()
    assert same_bits(run(device, o, d, v, f, t_min=lo), R.host().cast(v, f, o, d, t_min=lo))
    i = int(np.argmin(t_in))
    for k in (i, int(np.argmax(t_in))):
        ok, dk = o[k:k + 1], d[k:k + 1]
        assert run(device, ok, dk, v, f, t_min=float(t_in[k]))[1][0] == face_in[k]              # the end is inside
        assert run(device, ok, dk, v, f, t_max=float(t_in[k]))[1][0] == face_in[k]
        assert run(device, ok, dk, v, f, t_min=float(up(t_in[k])))[1][0] == face_out[k]         # just outside: the next one
        assert run(device, ok, dk, v, f, t_max=float(down(t_in[k])))[1][0] == -1
        assert run(device, ok, dk, v, f, t_min=float(up(t_in[k])), t_max=float(down(t_out[k])))[1][0] == -1
        t1, f1, _ = run(device, ok, dk, v, f, t_min=float(up(t_in[k])), t_max=float(t_out[k]))
        assert f1[0] == face_out[k] and t1[0] == t_out[k]


def _image_rays(H, W):
    az = (np.arange(W) + 0.5) / W * 2 * np.pi - np.pi
    el = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    ce = np.cos(el)[:, None]
    return np.stack([np.cos(az)[None] * ce, np.sin(az)[None] * ce, np.broadcast_to(np.sin(el)[:, None], (H, W))], -1).reshape(-1, 3)


def test_sphere_from_inside_has_no_miss(device):
    v, f = R.sphere()
    r = 3.0
    d = _image_rays(64, 256).astype(np.float32)
    o = np.zeros_like(d)
    t, face, _ = run(device, o, d, v, f)
    assert (face >= 0).all(), f"{(face < 0).sum()} rays left the closed sphere"         # the condition
    # every face lies between its plane's distance from the centre and the radius: the chord bound of this tessellation
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    plane = np.abs((n * a).sum(1)) / np.linalg.norm(n, axis=1)
    rng = t.astype(np.float64) * np.linalg.norm(d.astype(np.float64), axis=1)
    print(f"sphere: range in [{rng.min():.5f}, {rng.max():.5f}], planes from {plane.min():.5f}, radius {r}")
    assert rng.min() >= plane.min() * (1 - R.BAR) and rng.max() <= r * (1 + R.BAR)
    assert np.all(rng >= plane[face] * (1 - R.BAR))


def _room_distance(o, d, half):
    """The distance along d (unit or not: in units of |d|) from o inside the box [-half, half]^3 to its wall, float64."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf))
    return t.min(1)


def test_box_room_against_analytic_distances(device):
    v, f = R.cube(8, seed=3)
    rng = np.random.default_rng(8)
    d = rng.normal(0, 1, (4096, 3))
    d[:64, 0] = 0.0                                                       # some with a zero component
    d = (d * 10.0 ** rng.uniform(-1, 1, (len(d), 1))).astype(np.float32)
    o = np.tile(np.array([[1.25, -2.5, 0.75]], np.float32), (len(d), 1))
    t, face, _ = run(device, o, d, v, f)
    assert (face >= 0).all()
    want = _room_distance(o, d, 4.0)
    err = np.abs(t - want) / want
    print(f"box room: max |t - analytic| / t = {err.max():.3e}")
    assert np.all(err <= R.BAR)


def test_reuse_of_an_index(device):
    o, d, v, f, want = brute("grid", 16928, 256)
    o2, d2, _, _, want2 = brute("grid", 16928, 65)
    vt, ft = tt(v, device), tt(f, device)
    index = evaluation.mesh_ray_index(vt, ft)
    assert isinstance(index, evaluation.MeshRayIndex)
    a = evaluation.cast_rays(tt(o, device), tt(d, device), vt, ft, return_uv=True, index=index)
    b = evaluation.cast_rays(tt(o2, device), tt(d2, device), vt, ft, return_uv=True, index=index)
    assert same_bits([x.cpu().numpy() for x in a], want) and same_bits([x.cpu().numpy() for x in b], want2)
    with pytest.raises(ValueError, match="another mesh"):
        evaluation.cast_rays(tt(o, device), tt(d, device), vt, ft[:100], index=index)
    with pytest.raises(TypeError):
        evaluation.cast_rays(tt(o, device), tt(d, device), vt, ft, index="index")


def _raw(device, v, f, o, d, want_face=True, want_uv=True):
    """The C ABI directly: (t, face, uv, status words of the build, of the cast)."""
    lib = _abi.lib()
    vt, ft, ot, dt = tt(v, device), tt(f, device), tt(o, device), tt(d, device)
    V, F, M = len(v), len(f), len(o)
    nbytes = lib.sls_mesh_rayindex_bytes(V, F)
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    addr = (buf.data_ptr() + 255) & ~255
    s1, s2 = torch.full((4,), -7, dtype=torch.int32, device=device), torch.full((4,), -7, dtype=torch.int32, device=device)
    t = torch.full((M,), -7.0, device=device)
    face = torch.full((M,), -7, dtype=torch.int32, device=device)
    uv = torch.full((M, 2), -7.0, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    _abi.check(lib.sls_mesh_rayindex_build(V, vt.data_ptr(), F, ft.data_ptr(), addr, nbytes, s1.data_ptr(), st), "build")
    _abi.check(lib.sls_mesh_raycast(V, vt.data_ptr(), F, ft.data_ptr(), addr, nbytes, M, ot.data_ptr() if M else None,
                                    dt.data_ptr() if M else None, 0.0, math.inf, t.data_ptr() if M else None,
                                    face.data_ptr() if want_face else None, uv.data_ptr() if want_uv else None, s2.data_ptr(), st), "cast")
    torch.cuda.synchronize(device)
    return t.cpu().numpy(), face.cpu().numpy(), uv.cpu().numpy(), s1.cpu().tolist(), s2.cpu().tolist()


def test_outputs_are_optional_and_no_ray_is_fine(device):
    o, d, v, f, want = brute("grid", 257, 65)
    t, face, uv, s1, s2 = _raw(device, v, f, o, d, want_face=False, want_uv=False)
    assert t.tobytes() == want[0].tobytes() and (face == -7).all() and (uv == -7).all()
    assert s1 == [257, 0, 0, 0] and s2 == [257, 0, 0, 0]
    assert evaluation.cast_rays(tt(o, device), tt(d, device), tt(v, device), tt(f, device), return_face=False).shape == (65,)
    t0, face0, uv0, s1, s2 = _raw(device, v, f, o[:0], d[:0])
    assert s2 == [257, 0, 0, 0] and len(t0) == 0
    e = evaluation.cast_rays(tt(o[:0], device), tt(d[:0], device), tt(v, device), tt(f, device), return_uv=True)
    assert [tuple(x.shape) for x in e] == [(0,), (0,), (0, 2)]


def test_bad_faces_are_counted_not_dereferenced(device):
    o, d, v, f, _ = brute("grid", 300, 65)
    f = f.copy()
    f[7, 1], f[100, 0], f[200, 2] = len(v), -1, 2 ** 31 - 1
    vb = v.copy()
    vb[f[50, 0]] = np.nan
    n_nonfinite = int(((f >= 0) & (f < len(v))).all(1)[np.isnan(vb[np.clip(f, 0, len(v) - 1)]).any((1, 2))].sum())
    t, face, uv, s1, s2 = _raw(device, vb, f, o, d)
    assert s1 == [300, 3, n_nonfinite, 0] and s2 == s1 and n_nonfinite >= 1
    want = R.host().cast(vb, f, o, d)                                     # the bad faces never hit
    assert np.array_equal(face, want[1]) and t.tobytes() == want[0].tobytes()
    with pytest.raises(ValueError, match="3 faces have a vertex index outside"):
        evaluation.cast_rays(tt(o, device), tt(d, device), tt(v, device), tt(f, device))
    with pytest.raises(ValueError, match="non-finite"):
        evaluation.mesh_ray_index(tt(vb, device), tt(mesh("grid", 300)[1], device))


def test_refused_rays_are_counted_and_miss(device):
    o, d, v, f, _ = brute("grid", 257, 256)
    o, d = o.copy(), d.copy()
    d[3] = 0.0
    d[64] = [np.nan, 1.0, 0.0]
    o[65, 2] = np.inf
    d[130] = [1e-35, -1e-33, 0.0]
    d[192:256] = 0.0                                                      # a whole wave of them
    t, face, uv, s1, s2 = _raw(device, v, f, o, d)
    bad = np.zeros(len(o), bool)
    bad[[3, 64, 65, 130]] = True
    bad[192:256] = True
    assert s2 == [257, 0, 0, int(bad.sum())] and s1[3] == 0
    assert (face[bad] == -1).all() and np.isposinf(t[bad]).all() and (uv[bad] == 0).all()
    want = R.host().cast(v, f, o, d)
    assert np.array_equal(face, want[1]) and t.tobytes() == want[0].tobytes() and uv.tobytes() == want[2].tobytes()


# ---- the range image ------------------------------------------------------------------------------------------------------
def _pose():
    T = np.eye(4)
    yaw, pitch = math.radians(37.0), math.radians(-11.0)
    Rz = np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(pitch), 0, math.sin(pitch)], [0, 1, 0], [-math.sin(pitch), 0, math.cos(pitch)]])
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = [1.25, -2.5, 0.75]
    return T


def test_render_mesh_pixel_convention_matches_depth_to_points(device):
    v, f = R.cube(8, seed=3)
    H, W, half = 32, 128, 4.0
    pose = _pose()
    cam = Camera(synth.spherical_K(H, W), torch.zeros((1, H, W), device=device), world_T_lidar=pose, data_device=device)
    out = evaluation.render_mesh(tt(v, device), tt(f, device), cam)
    rng, face, normal = out["range"], out["face"], out["normal"]
    assert rng.shape == (H, W) and face.shape == (H, W) and face.dtype == torch.int32 and normal.shape == (3, H, W)
    assert bool((face >= 0).all()) and bool((rng > 0).all())
    pts = depth_to_points(cam, rng[None]).reshape(3, -1).T.cpu().numpy().astype(np.float64)      # world frame
    scale = np.linalg.norm(pts - pose[:3, 3], axis=1)
    off_wall = np.abs(np.abs(pts).max(1) - half)
    print(f"render_mesh: back-projected pixels off their wall by {np.max(off_wall / scale):.3e} of the range at most")
    assert np.all(off_wall <= 1e-5 * scale)
    # the analytic range of each pixel's ray
    from splat_loam_amd.renderer import pixel_rays
    rays_w = pixel_rays(cam).reshape(-1, 3).cpu().numpy().astype(np.float64) @ pose[:3, :3].T
    want = _room_distance(np.broadcast_to(pose[:3, 3], rays_w.shape), rays_w, half)
    assert np.all(np.abs(rng.reshape(-1).cpu().numpy() - want) <= 1e-5 * want)
    # the normal: unit, of the wall hit, towards the sensor, in the sensor frame
    n_world = normal.reshape(3, -1).T.cpu().numpy().astype(np.float64) @ pose[:3, :3].T
    axis = np.abs(pts).argmax(1)
    expect = np.zeros_like(n_world)
    expect[np.arange(len(pts)), axis] = -np.sign(pts[np.arange(len(pts)), axis])
    assert np.abs(n_world - expect).max() <= 1e-5
    # t_max: the walls beyond it are not seen, range 0 and normal 0 there; an index built before gives the same image
    index = evaluation.mesh_ray_index(tt(v, device), tt(f, device))
    near = evaluation.render_mesh(tt(v, device), tt(f, device), cam, t_max=5.0, index=index)
    seen = near["face"] >= 0
    assert bool(seen.any()) and bool((~seen).any()) and torch.equal(seen, rng <= 5.0)
    assert bool((near["range"][~seen] == 0).all()) and bool((near["normal"][:, ~seen] == 0).all())
    assert torch.equal(near["range"][seen], rng[seen]) and torch.equal(near["face"][seen], face[seen])


# ---- the depth check and the tools ------------------------------------------------------------------------------------------
H2, W2, VS2 = 64, 256, 0.1


@pytest.fixture(scope="module")
def room(device, tmp_path_factory):
    """A small results directory (one model, one keyframe: 6000 surfels on a shell of 2.4 - 2.6 m around the sensor, facing
    it) and the mesh `mesh_tsdf` makes of it, saved as a PLY."""
    d = tmp_path_factory.mktemp("raycast_room")
    K = synth.spherical_K(H2, W2)
    sc = synth.make_scene(6000, H2, W2, seed=77, range_lo=2.4, range_hi=2.6, scale_lo=0.06, scale_hi=0.15, opac_lo=0.6, max_tilt_deg=10.0)
    ply_io.save_ply(d / "models/model_0.ply", sc["means"], np.log(sc["opac"] / (1 - sc["opac"])), np.log(sc["scales"]), sc["rots"])
    world_T_model = np.eye(4)
    world_T_model[:3, :3] = _pose()[:3, :3]
    world_T_model[:3, 3] = [12.0, -7.0, 1.5]
    model = {"id": 0, "world_T_model": world_T_model, "filename": "models/model_0.ply", "frame_ids": [0]}
    frame = {"id": 0, "timestamp": 0.0, "model_T_frame": synth.keyframe_poses(2)[1],
             "projmatrix": [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])], "model_id": 0}
    traj_io.write_graph(d / "graph.yaml", [model], [frame])
    with open(d / "cfg.yaml", "w") as fh:
        fh.write(f"preprocessing:\n  image_height: {H2}\n  image_width: {W2}\n")
    vertices, faces = meshing.mesh_tsdf(d, VS2, kf_samples=2000, seed=0x5EED, device=device)
    ply_io.save_mesh(d / "mesh.ply", vertices, faces)
    return d, vertices, faces, world_T_model @ frame["model_T_frame"]


def test_mesh_depth_check(device, room):
    d, vertices, faces, world_T_frame = room
    res = meshing.mesh_depth_check(d, vertices, faces, device=device)
    print("mesh_depth_check:", {k: res[k] for k in ("valid", "covered", "mean", "median")})
    assert res["frame_ids"] == [0] and len(res["keyframes"]) == 1 and res["keyframes"][0]["valid"] == res["valid"]
    # most of the image is valid and the mesh covers most of that (a one-keyframe TSDF leaves holes where a voxel's corners
    # were not all observed: no figure is claimed beyond "the majority")
    assert res["valid"] > 0.5 * H2 * W2 and res["covered"] > 0.5 * res["valid"]
    # the fused surface lies within a voxel of the depth it was fused from
    assert res["mean"] < VS2 and res["median"] < VS2
    # the same mesh moved 0.2 m along the sensor's x axis: every wall the sensor faces along x is 0.2 m off
    shift = torch.tensor(world_T_frame[:3, 0] * 0.2, dtype=torch.float32, device=device)
    moved = meshing.mesh_depth_check(d, vertices + shift, faces, device=device)
    print("    moved 0.2 m:", {k: moved[k] for k in ("valid", "covered", "mean", "median")})
    assert moved["valid"] == res["valid"]
    assert moved["mean"] > res["mean"] and moved["median"] > res["median"]
    assert moved["mean"] <= 0.5                                            # (the truncation)
    # truncated at 1 cm nothing exceeds it; the options are sample_surface's
    tight = meshing.mesh_depth_check(d, vertices + shift, faces, device=device, truncation=0.01, min_opacity=0.9)
    assert tight["mean"] <= 0.01 and tight["valid"] < res["valid"]
    every_second = meshing.mesh_depth_check(d, vertices, faces, device=device, kf_interval=2)
    assert every_second["frame_ids"] == [] and every_second["valid"] == 0 and every_second["mean"] is None


def test_tools_run_and_write_their_files(device, room):
    d, vertices, faces, world_T_frame = room
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_depth_check.py"), str(d), str(d / "mesh.ply"), "--json",
                          str(d / "check.json")], check=True, capture_output=True, text=True, env=env).stdout
    assert "median" in out and "all" in out
    with open(d / "check.json") as fh:
        js = json.load(fh)
    ref = meshing.mesh_depth_check(d, vertices, faces, device=device)
    assert js["valid"] == ref["valid"] and js["covered"] == ref["covered"] and js["mean"] == pytest.approx(ref["mean"], rel=1e-9)
    pose = [str(x) for x in world_T_frame[:3].reshape(-1)]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_render.py"), str(d / "mesh.ply"), str(d / "image.npz"), "--pose",
                          *pose, "--height", "16", "--width", "64"], check=True, capture_output=True, text=True, env=env).stdout
    line = json.loads(out.strip().splitlines()[-1])
    z = np.load(d / "image.npz")
    assert z["range"].shape == (16, 64) and z["face"].shape == (16, 64) and z["normal"].shape == (3, 16, 64)
    assert line["hit"] == int((z["face"] >= 0).sum()) > 0.8 * 16 * 64
    assert 2.2 < line["mean_range_m"] < 2.8                                # the shell's radius
