"""The TSDF volume on the GPU (sls_tsdf_blocks, sls_tsdf_integrate, sls_tsdf_extract_count / _emit, splat_loam_amd/tsdf.py,
meshing.mesh_tsdf) against include/sls_tsdf_math.h run on the host (tsdf_ref.host()), bit for bit: block lists and status
words, both arrays of an integrated volume, the triangle soup in order.  The float64 restatement, the manifold, Euler and
radius checks of tests/test_tsdf_math.py run on the device output as well; a keyframe of a synthetic room goes through the
real rasterizer forward end to end."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import surface_ref
import tsdf_ref as ref
from splat_loam_amd import _abi, evaluation, meshing, ply_io, synth, traj_io, tsdf
from tsdf_ref import CENTRE, ORIGIN, TRUNC, VS, bits

pytestmark = pytest.mark.gpu


# ---- blocks ----------------------------------------------------------------------------------------------------------
def _block_cases():
    rng = np.random.default_rng(12)
    e = 8 * VS
    return {"one": np.array([[0.3, -0.2, 0.1]], np.float32),
            "adjacent": np.array([[0.5 * e, 0.5 * e, 0.5 * e], [1.5 * e, 0.5 * e, 0.5 * e]], np.float32),
            "random": rng.normal(0, 4, (3000, 3)).astype(np.float32),
            "edges": ref.key_points()}


@pytest.mark.parametrize("case", ["one", "adjacent", "random", "edges"])
def test_blocks(device, case):
    pts = _block_cases()[case]
    origin = ORIGIN if case != "one" else (0.0, 0.0, 0.0)
    want, n_nf, n_rng = ref.host().blocks_of_points(pts, VS, TRUNC, origin)
    got, det = tsdf.allocate_blocks(torch.from_numpy(pts).to(device), VS, TRUNC, origin, details=True)
    print(f"{case}: {len(pts)} points, {len(want)} blocks, non-finite {n_nf}, out of range {n_rng}")
    assert got.dtype == torch.int32 and got.device == device
    assert (det["n_nonfinite"], det["n_out_of_range"]) == (n_nf, n_rng)
    assert np.array_equal(got.cpu().numpy(), want)
    if case == "one":
        assert len(want) == 8
    if case == "adjacent":
        assert len(want) == 4 * 3 * 3 and [0, 0, 0] in want.tolist() and [1, 0, 0] in want.tolist()    # mid-block points: three per axis each
    again = tsdf.allocate_blocks(torch.from_numpy(pts).to(device), VS, TRUNC, origin)
    assert torch.equal(again, got)                                       # the same bytes on every run


def test_blocks_status_words_capacity_and_empty(device):
    lib = _abi.lib()
    pts = torch.from_numpy(_block_cases()["edges"]).to(device)
    M = int(pts.shape[0])
    want, n_nf, n_rng = ref.host().blocks_of_points(pts.cpu().numpy(), VS, TRUNC, ORIGIN)
    origin = (C.c_double * 3)(*ORIGIN)
    nbytes = int(lib.sls_tsdf_blocks_scratch_bytes(M))
    scratch = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    cap = 100                                                            # fewer rows than blocks: the rest is counted, not written
    out = torch.full((cap + 50, 3), -7, dtype=torch.int32, device=device)
    status = torch.full((4,), -7, dtype=torch.int32, device=device)
    _abi.check(lib.sls_tsdf_blocks(M, pts.data_ptr(), VS, TRUNC, origin, cap, out.data_ptr(), status.data_ptr(),
                                   (scratch.data_ptr() + 255) & ~255, nbytes, st), "sls_tsdf_blocks")
    assert status.cpu().tolist() == [len(want), n_nf, n_rng, 1] and len(want) > cap
    assert np.array_equal(out[:cap].cpu().numpy(), want[:cap]) and bool((out[cap:] == -7).all())
    status.fill_(-7)
    _abi.check(lib.sls_tsdf_blocks(0, None, VS, TRUNC, origin, 0, None, status.data_ptr(), None, 0, st), "sls_tsdf_blocks")
    assert status.cpu().tolist() == [0, 0, 0, 1]
    empty = tsdf.allocate_blocks(torch.zeros((0, 3), device=device), VS, TRUNC)
    assert empty.shape == (0, 3)


# ---- integrate -------------------------------------------------------------------------------------------------------
def _sls_camera(cam, H, W):
    c = _abi.SlsCamera()
    c.H, c.W, c.wrap = H, W, int(cam["wrap"])
    c.fx, c.fy, c.cx, c.cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    c.scale_modifier, c.near_cut, c.far_cut = 1.0, float(cam["near_cut"]), 100.0
    R = np.asarray(cam["R"], np.float32).reshape(9)
    for i in range(9):
        c.Rvw[i] = float(R[i])
    for i in range(3):
        c.tvw[i] = float(cam["t"][i])
    return c


@pytest.mark.parametrize("depth_ratio", [0.0, 1.0])
@pytest.mark.parametrize("hfov,vfov", [(360.0, 60.0), (120.0, 60.0)])
def test_integrate_two_keyframes(device, hfov, vfov, depth_ratio):
    lib = _abi.lib()
    blocks, cams, maps = ref.integration_case(hfov, vfov)
    B = len(blocks)
    vol = tsdf.TsdfVolume(torch.from_numpy(blocks).to(device), VS, TRUNC, ORIGIN)
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and vol.nbytes == B * 4096
    want_t, want_w = np.ones((B, 512), np.float32), np.zeros((B, 512), np.float32)
    origin = (C.c_double * 3)(*ORIGIN)
    st = torch.cuda.current_stream(device).cuda_stream
    for cam, am in zip(cams, maps):
        want_t, want_w, _ = ref.host().integrate(blocks, want_t, want_w, am, cam, VS, TRUNC, ORIGIN, 0.5, 0.1, depth_ratio)
        am_dev = torch.from_numpy(np.array(am)).to(device)
        _abi.check(lib.sls_tsdf_integrate(C.byref(_sls_camera(cam, ref.H, ref.W)), B, vol.blocks.data_ptr(), vol.tsdf.data_ptr(),
                                          vol.weight.data_ptr(), am_dev.data_ptr(), VS, TRUNC, origin, 0.5, 0.1, depth_ratio, st),
                   "sls_tsdf_integrate")
    got_t, got_w = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    print(f"{hfov:.0f} deg, depth_ratio {depth_ratio}: {B} blocks, {int((want_w > 0).sum())} voxels observed, {int((want_w > 1).sum())} twice")
    assert np.array_equal(bits(got_w), bits(want_w))                     # all voxels, both arrays, bit for bit
    assert np.array_equal(bits(got_t), bits(want_t))
    ref.compare_with_float64(blocks, cams, maps, depth_ratio, got_t, got_w, "device")


# ---- extract ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere():
    blocks, t, w = ref.sphere_volume(CENTRE, 1.0, VS, TRUNC, ORIGIN)
    tris, counts = ref.host().extract(blocks, t, w, VS, ORIGIN)
    for a in (blocks, t, w, tris, counts):
        a.setflags(write=False)
    return blocks, t, w, tris, counts


def _volume(device, blocks, t, w, vs=VS, origin=ORIGIN):
    vol = tsdf.TsdfVolume(torch.from_numpy(np.array(blocks)).to(device), vs, 4 * vs, origin)
    vol.tsdf.copy_(torch.from_numpy(np.array(t)))
    vol.weight.copy_(torch.from_numpy(np.array(w)))
    return vol


def test_extract_sphere(device):
    blocks, t, w, want, counts = _sphere()
    vol = _volume(device, blocks, t, w)
    vertices, faces, det = vol.extract(details=True)
    got = vertices.view(-1, 3, 3).cpu().numpy()
    print(f"sphere: {len(blocks)} blocks, {len(got)} triangles (host {len(want)})")
    assert np.array_equal(det["counts"].cpu().numpy(), counts) and len(got) == int(counts.sum()) == len(want)
    assert np.array_equal(bits(got), bits(want))                         # the soup, in order
    assert faces.dtype == torch.int32 and torch.equal(faces.view(-1), torch.arange(3 * len(want), dtype=torch.int32, device=device))
    ref.check_sphere_mesh(got)
    v2, f2 = vol.extract()                                               # the same bytes on every run
    assert torch.equal(v2, vertices)
    # welded: bit-equal vertices merged, the same triangles
    vw, fw = vol.extract(weld=True)
    rep = ref.manifold_report(got)
    assert vw.shape == (rep["V"], 3) and fw.shape == (len(want), 3)
    assert torch.equal(vw[fw.long()].view(-1, 3), vertices)
    assert rep["V"] - rep["E"] + rep["F"] == 2


def test_extract_missing_block_zero_weight_and_one_block(device):
    blocks, t, w, full, counts = _sphere()
    k = ref.drop_cases(blocks, counts)
    keep = np.arange(len(blocks)) != k
    part = _volume(device, blocks[keep], t[keep], w[keep]).extract()[0].view(-1, 3, 3).cpu().numpy()
    want, _ = ref.host().extract(blocks[keep], t[keep], w[keep], VS, ORIGIN)
    assert np.array_equal(bits(part), bits(want))
    ref.check_missing(full, part, blocks, k, VS, ORIGIN)
    w0 = np.array(w)
    w0[k] = 0.0
    part2 = _volume(device, blocks, t, w0).extract()[0].view(-1, 3, 3).cpu().numpy()
    assert np.array_equal(bits(part2), bits(part))
    # B = 1: no triangle across an absent neighbour
    one = _volume(device, blocks[k:k + 1], t[k:k + 1], w[k:k + 1]).extract()[0].view(-1, 3, 3).cpu().numpy()
    want1, _ = ref.host().extract(blocks[k:k + 1], t[k:k + 1], w[k:k + 1], VS, ORIGIN)
    assert len(one) > 0 and np.array_equal(bits(one), bits(want1))
    g = np.floor((one.astype(np.float64).min(1) - np.asarray(ORIGIN)) / VS - 0.5 + 1e-6).astype(np.int64) - 8 * blocks[k]
    assert (g >= 0).all() and (g <= 6).all()
    # nothing observed often enough, and no block at all
    assert _volume(device, blocks, t, w).extract(min_weight=2.0)[0].shape == (0, 3)
    v0, f0 = tsdf.TsdfVolume(torch.zeros((0, 3), dtype=torch.int32, device=device), VS, TRUNC).extract()
    assert v0.shape == (0, 3) and f0.shape == (0, 3)


def test_extract_random_volume(device):
    """Every case of every tetrahedron, zeros among the values, unobserved voxels, negative block coordinates."""
    import itertools
    rng = np.random.default_rng(3)
    b2 = np.array(sorted(itertools.product((0, 1), (-1, 0), (2, 3)), key=lambda b: int(ref.block_key(np.array(b)))), np.int32)
    t2 = rng.uniform(-1, 1, (len(b2), 512)).astype(np.float32)
    t2[rng.uniform(size=t2.shape) < 0.05] = 0.0
    w2 = (rng.uniform(size=t2.shape) < 0.97).astype(np.float32)
    want, wc = ref.host().extract(b2, t2, w2, 0.3, (1.0, 2.0, 3.0))
    vol = tsdf.TsdfVolume(torch.from_numpy(b2).to(device), 0.3, 1.2, (1.0, 2.0, 3.0))
    vol.tsdf.copy_(torch.from_numpy(t2))
    vol.weight.copy_(torch.from_numpy(w2))
    v, _, det = vol.extract(details=True)
    assert np.array_equal(det["counts"].cpu().numpy(), wc) and len(want) > 5000
    assert np.array_equal(bits(v.view(-1, 3, 3).cpu().numpy()), bits(want))


# ---- end to end ------------------------------------------------------------------------------------------------------
H2, W2, K2 = 64, 256, 2000
VS2 = 0.1
TRUNC2 = 4 * VS2
SEED = 0x5EED


def _world_T_model(identity):
    T = np.eye(4)
    if not identity:
        T[:3, :3] = ref.rot([0.1, 0.4, 1.0], 50.0)
        T[:3, 3] = [12.0, -7.0, 1.5]
    return T


def _write_room(d, identity):
    """One model, one keyframe: 6000 surfels on a shell of 2.4 - 2.6 m around the sensor, facing it: a closed room."""
    K = synth.spherical_K(H2, W2)
    sc = synth.make_scene(6000, H2, W2, seed=77, range_lo=2.4, range_hi=2.6, scale_lo=0.06, scale_hi=0.15, opac_lo=0.6, max_tilt_deg=10.0)
    ply_io.save_ply(d / "models/model_0.ply", sc["means"], np.log(sc["opac"] / (1 - sc["opac"])), np.log(sc["scales"]), sc["rots"])
    pose = synth.keyframe_poses(2)[1]
    model = {"id": 0, "world_T_model": _world_T_model(identity), "filename": "models/model_0.ply", "frame_ids": [0]}
    frame = {"id": 0, "timestamp": 0.0, "model_T_frame": pose, "projmatrix": [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])],
             "model_id": 0}
    traj_io.write_graph(d / "graph.yaml", [model], [frame])
    with open(d / "cfg.yaml", "w") as f:
        f.write(f"preprocessing:\n  image_height: {H2}\n  image_width: {W2}\n")
    return model, frame, K, pose


@pytest.mark.parametrize("identity", [True, False])
def test_mesh_tsdf_end_to_end(device, tmp_path, identity):
    model, frame, K, pose = _write_room(tmp_path, identity)
    vertices, faces, det = meshing.mesh_tsdf(tmp_path, VS2, kf_samples=K2, seed=SEED, device=device, details=True)
    T = int(faces.shape[0])
    print(f"world_T_model identity {identity}: {det['blocks']} blocks, {det['volume_bytes']} bytes, {T} triangles, stages {det['stage_ms']}")
    assert T > 1000 and det["blocks"] * 4096 == det["volume_bytes"] and det["frame_ids"] == [0]
    # the pieces composed by hand, bit for bit
    pts, nrm = meshing.sample_surface(tmp_path, kf_samples=K2, seed=SEED, device=device)
    blocks = tsdf.allocate_blocks(pts, VS2, TRUNC2)
    assert torch.equal(blocks, det["volume"].blocks)
    vol = tsdf.TsdfVolume(blocks, VS2, TRUNC2)
    used = [(0, 0)]
    for i, fid, cam, allmap in meshing._render_keyframes(tmp_path, traj_io.read_graph(tmp_path / "graph.yaml"), used, [pose], H2, W2, device):
        vol.integrate(allmap, cam, model["world_T_model"])
    assert torch.equal(vol.tsdf, det["volume"].tsdf) and torch.equal(vol.weight, det["volume"].weight)
    v2, f2 = vol.extract()
    assert torch.equal(v2, vertices) and torch.equal(f2, faces)
    # the volume the device integrated = the header on the host over the same allmap and the composed frame
    am = allmap.cpu().numpy()
    view32 = np.linalg.inv(pose).astype(np.float32)
    m = tsdf.compose_volume_to_view(model["world_T_model"], view32).reshape(3, 4)
    cam_d = {"fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2], "R": m[:, :3], "t": m[:, 3], "wrap": 1, "near_cut": np.float32(0.2)}
    B = int(blocks.shape[0])
    ht, hw, _ = ref.host().integrate(blocks.cpu().numpy(), np.ones((B, 512), np.float32), np.zeros((B, 512), np.float32), am, cam_d, VS2,
                                     TRUNC2, (0.0, 0.0, 0.0), 0.5, 0.1, 0.0)
    assert np.array_equal(bits(vol.weight.cpu().numpy()), bits(hw)) and np.array_equal(bits(vol.tsdf.cpu().numpy()), bits(ht))
    # every vertex within trunc + sqrt(3) voxel_size of the back-projected point of some valid pixel
    valid = np.flatnonzero(surface_ref.valid_mask(am, 0.5, 0.1))
    wp, _ = surface_ref.points_normals(am, valid, K, view32, model["world_T_model"], 0.0)
    d2, _ = evaluation.nearest(torch.from_numpy(wp.astype(np.float32)).to(device), vertices, return_index=False)
    far = float(d2.max().sqrt())
    bound = TRUNC2 + np.sqrt(3.0) * VS2
    print(f"    {len(valid)} valid pixels of {H2 * W2}; farthest vertex {far:.4f} m from a back-projected pixel (bound {bound:.4f} m)")
    assert len(valid) > 0.5 * H2 * W2 and far <= bound
    # the surface lies where the room is: the mesh against the sampled cloud
    metrics = evaluation.evaluate_recon(pts, vertices, faces, down_sample_res=0.02, mesh_sample_point=20000, seed=1)
    print("    evaluate_recon:", {k: round(float(v), 4) for k, v in metrics.items() if isinstance(v, (int, float))})
    assert all(np.isfinite(float(v)) for v in metrics.values() if isinstance(v, (int, float)))
    # written and read back
    ply_io.save_mesh(tmp_path / "mesh.ply", vertices, faces)
    lv, lf = ply_io.load_mesh(tmp_path / "mesh.ply")
    assert np.array_equal(bits(lv), bits(vertices.cpu().numpy())) and np.array_equal(lf, faces.cpu().numpy())
