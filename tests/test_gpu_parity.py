"""HIP path (through the C-ABI) vs the CPU checker on identical seeded inputs.

Bar (BASELINE.json north_star): tile/key integers bit-exact; rendered
depth/alpha/normal and all gradients <= 1e-5 relative (max-norm relative per
channel / tensor; per-surfel gradient records relative to the sum of |terms|).
Pixels where the checker flags a discrete decision within 1e-4 of its threshold
("fragile": alpha vs 1/255, T vs 1e-4, rho3d vs rho2d, ...) are compared with a
loose bound instead, because a 1-ulp different exp/rcp may legitimately decide
the other way there.  "parity unpinned": the checker is this repo's restatement
(oracle/sls_oracle.c header).
"""
import numpy as np
import pytest
import torch

from helpers import RTOL, hip_backward, hip_forward, rel_err, scene_and_camera, tangent, u32

pytestmark = pytest.mark.gpu


def test_selftest(device):
    from splat_loam_amd import _abi
    _abi.check(_abi.lib().sls_selftest(torch.cuda.current_stream(device).cuda_stream), "sls_selftest")


def _compare_forward(oracle32, st, ost, cam, name):
    pre = ost["pre"]
    # ---- integers: bit-exact -------------------------------------------------
    assert np.array_equal(st.radii.cpu().numpy(), pre["radii"]), f"{name}: radii"
    assert np.array_equal(st.rect.cpu().numpy(), pre["rect"]), f"{name}: rect"
    assert np.array_equal(u32(st.tiles), pre["tiles"]), f"{name}: tiles_touched"
    tested = (pre["rect"][:, 1] * pre["rect"][:, 3]) <= 64      # (beyond 64 tiles the mask carries no information)
    assert np.array_equal(st.tmask.cpu().numpy().view(np.uint64)[tested], pre["tmask"][tested]), f"{name}: D10 tile masks"
    assert np.array_equal(u32(st.depth), pre["depth"].view(np.uint32)), f"{name}: depth key bits"
    assert st.R == ost["binned"]["R"], f"{name}: R"
    order = u32(st.order)
    vis = pre["tiles"] > 0
    nvis = int(vis.sum())
    ref_order = np.lexsort((np.arange(len(vis)), pre["depth"].view(np.uint32)))        # (depth bits, index)
    ref_order = ref_order[vis[ref_order]]
    assert np.array_equal(order[vis[order]], ref_order.astype(np.uint32)), f"{name}: depth order of the visible surfels"
    assert np.array_equal(u32(st.offsets), np.cumsum(pre["tiles"][order], dtype=np.uint64).astype(np.uint32))
    assert np.array_equal(st.keys.cpu().numpy().view(np.uint64), ost["binned"]["keys"]), f"{name}: sorted keys"
    assert np.array_equal(u32(st.vals), ost["binned"]["vals"]), f"{name}: sorted values"
    assert np.array_equal(u32(st.ranges), ost["binned"]["ranges"]), f"{name}: tile ranges"
    # ---- surfel records ---------------------------------------------------------
    rec = st.rec.cpu().numpy()
    ref = pre["rec"]
    spec = [k for k in range(18) if k != 15]      # (15, 18, 19: kc, ex, ey — culling aids, not part of the contract)
    exact = np.array_equal(rec[:, spec].view(np.uint32), ref[:, spec].view(np.uint32))
    if not exact:
        e = rel_err(rec[:, spec], ref[:, spec], scale=np.abs(ref[:, spec]).max(axis=0, keepdims=True))
        assert e.max() <= 1e-6, f"{name}: record mismatch {e.max()}"
    # ---- allmap ---------------------------------------------------------------------
    am = st.allmap.cpu().numpy()
    oam = ost["allmap"]
    frag = ost["fwd"]["fragile"]
    ok = ~frag
    # "fragile" = a discrete decision of the pixel lies within 1e-4 of its threshold; such pixels are compared
    # loosely below, so their number is bounded: measured 0.3 .. 1.5 % on the test scenes
    assert frag.mean() <= 0.02, f"{name}: {frag.mean():.3%} of the pixels are flagged fragile"
    worst = {}
    for c in range(7):
        scale = max(np.abs(oam[c]).max(), 1e-12)
        if c == 6:
            # distortion = sum_i w_i (m_i^2 A_i + M2_i - 2 m_i M1_i): a difference of O(1)
            # terms (m, A in [0,1]) that nearly cancel; the error is relative to those
            # terms, not to the tiny result.
            scale = max(scale, 1.0)
        err = np.abs(am[c].astype(np.float64) - oam[c]) / scale
        worst[c] = err[ok].max() if ok.any() else 0.0
        tol = RTOL
        assert worst[c] <= tol, f"{name}: allmap ch{c} rel err {worst[c]:.3e} (non-fragile pixels)"
        if frag.any():
            assert err[frag].max() <= 5e-2, f"{name}: allmap ch{c} fragile pixel error {err[frag].max():.3e}"
    # saved per-pixel state
    ps = st.pix_state.cpu().numpy()
    pc = u32(st.pix_contrib).reshape(-1, 2)
    okf = ok.reshape(-1)
    assert np.array_equal(pc[okf, 0], ost["fwd"]["pixN"][okf]), f"{name}: n_contrib"
    assert np.array_equal(pc[okf, 1], ost["fwd"]["pixMed"][okf]), f"{name}: median_contrib"
    assert np.abs(ps[okf, 0] - ost["fwd"]["pixT"][okf]).max() <= 1e-5
    return worst, int(frag.sum())


def _compare_backward(oracle32, st, t, ost, sc, name, seed=3):
    H, W = ost["cam"].H, ost["cam"].W
    rng = np.random.default_rng(seed)
    dL = rng.normal(size=(7, H, W)).astype(np.float32)
    dL[:, ost["fwd"]["fragile"]] = 0.0
    dm, ds, dr, do, grec = hip_backward(st, t, dL)
    ob = oracle32.backward(ost, dL, threads=1, want_abs=True)
    # per-surfel gradient records relative to sum |terms|
    gabs = ob["gabs"].astype(np.float64)
    floor = 1e-3 * gabs.max(axis=0, keepdims=True)
    err = np.abs(grec.astype(np.float64) - ob["grec"]) / np.maximum(gabs, np.maximum(floor, 1e-30))
    i, k = np.unravel_index(err.argmax(), err.shape)
    print(f"\n[{name}] grec worst rel-to-abs-sum {err.max():.2e} at surfel {i} field {k}: hip {grec[i, k]:.6e} "
          f"ref {ob['grec'][i, k]:.6e} abs-sum {gabs[i, k]:.3e}; per-field worst "
          f"{[f'{v:.1e}' for v in err.max(axis=0)]}")
    assert err.max() <= 1e-4, f"{name}: grec rel-to-abs-sum err {err.max():.3e}"
    worst = {}
    for nm, a, ref in (("means", dm, ob["dmeans"]), ("scales", ds, ob["dscales"]), ("opac", do, ob["dopac"]),
                       ("rots", tangent(dr.astype(np.float64), sc["rots"].astype(np.float64)),
                        tangent(ob["drots"].astype(np.float64), sc["rots"].astype(np.float64)))):
        scale = max(np.abs(ref).max(), 1e-30)
        e = np.abs(a.astype(np.float64) - ref).max() / scale
        worst[nm] = e
        assert e <= RTOL, f"{name}: d{nm} max-norm rel err {e:.3e}"
        big = np.abs(ref) > 1e-3 * scale          # element-wise: entries above 1e-3 of the tensor's maximum
        er = (np.abs(a.astype(np.float64) - ref)[big] / np.abs(ref)[big]).max() if big.any() else 0.0
        worst[nm + "_elem"] = er
        assert er <= 2e-3, f"{name}: d{nm} element-wise rel err {er:.3e}"
    return worst


@pytest.mark.parametrize("kmin", [1, 2, 3])
def test_tile_cull_thresholds_parity(device, oracle32, kmin):
    """D10 at other thresholds than the default (SlsCamera.tile_cull_min: 1 = off, 2 and 3 = test nearly every / most
    rectangles): tile masks, tiles_touched, the sorted lists and the image stay bit-exact / within the bar against the
    checker at the same threshold, on a scene of large tilted footprints."""
    from splat_loam_amd import _abi
    N, H, W = 8000, 64, 1024
    sc, view, proj = scene_and_camera(N, H, W, seed=29, range_lo=1.5, range_hi=12.0, scale_lo=0.01, scale_hi=0.6, max_tilt_deg=80.0)
    st, t = hip_forward(device, sc, view, proj, H, W, tile_cull_min=kmin)
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size(), tile_cull=(0 if kmin == 1 else kmin))
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    _compare_forward(oracle32, st, ost, cam, f"tile_cull_min{kmin}")
    _compare_backward(oracle32, st, t, ost, sc, f"tile_cull_min{kmin}")


def _emission_counts_its_chunks(N, T, R):
    """launch_bin_sort's rule (sls_sort.hip, emit_hist) for a single-pass tile sort: the emission's workgroups of 256
    positions are the pass's chunks while their count table is small and fits the sorter's (sort_core_bytes)"""
    bins, nemit = max(256, 1 << (T - 1).bit_length()), (N + 255) // 256
    core = (2048 * max((R + 1023) // 1024, 1) + 2048) * 4
    return bins * nemit <= 400000 and (bins * nemit + bins + nemit + 1) * 4 <= core


SCATTER_CASES = [
    # name, W, hfov, scene, the emission's chunks?  (D10 on: the direct binning is out, emission + one radix pass)
    ("emission_chunks", 1024, 360.0, {}, True),                 # 256 bins x 79 chunks: sort_scatter_chunks_kernel
    ("fixed_chunks", 512, 60.0, dict(range_lo=8.0, scale_lo=0.005, scale_hi=0.02), False),   # five surfels in six are
]                                                               # out of view: the table outgrows the sorter's, sort_scatter_kernel


@pytest.mark.parametrize("list_pairs", [2, 1], ids=["u32-packed", "u64-pairs"])
@pytest.mark.parametrize("name,W,hfov,kw,chunks", SCATTER_CASES, ids=[c[0] for c in SCATTER_CASES])
def test_tile_sort_scatter_variants_parity(device, oracle32, name, W, hfov, kw, chunks, list_pairs):
    """Both scatter kernels of the radix sorter (sls_radix.hip) in the tile sort's single pass with ranges, each with
    packed 32-bit instances (plain list) and with 64-bit instances stored as (surfel, block mask) pairs: sorted lists,
    ranges and image against the checker.  Which kernel ran follows from N, the tile count and R by the launcher's rule."""
    from splat_loam_amd import _abi
    N, H = 20000, 64
    sc, view, proj = scene_and_camera(N, H, W, seed=31, hfov_deg=hfov, **kw)
    st, t = hip_forward(device, sc, view, proj, H, W, tile_cull_min=2, list_pairs=list_pairs)
    tw, th = _abi.tile_size()
    print(f"\n[{name}] R={st.R}")
    assert st.R > 0 and _emission_counts_its_chunks(N, (H // th) * (W // tw), st.R) == chunks
    assert st.vals_stride == (2 if list_pairs == 1 else 1)
    cam = oracle32.camera(H, W, view, proj, tile=(tw, th), tile_cull=2)
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    _compare_forward(oracle32, st, ost, cam, f"{name}-{list_pairs}")
    _compare_backward(oracle32, st, t, ost, sc, f"{name}-{list_pairs}")


@pytest.mark.parametrize("offset", [(-0.5, -0.5), (0.25, -0.125)])
def test_pixel_centre_offset_parity(device, oracle32, offset):
    """D1 as a parameter (SlsCamera.pix_offset): pixel (c, r) at image coordinate (c + ox, r + oy).  The reference's
    own back-projection uses (-0.5, -0.5) (utils/graphic_utils.py:46-49).  Forward integers bit-exact, allmap and
    gradients to the usual bar against the checker given the same offset — and the image really moves: rendered
    with the offset, the surfels land where the un-offset render puts them half a pixel further."""
    from splat_loam_amd import _abi
    N, H, W = 6000, 64, 512
    sc, view, proj = scene_and_camera(N, H, W, seed=23, range_lo=2.0, range_hi=25.0)
    st, t = hip_forward(device, sc, view, proj, H, W, pix_offset=offset)
    assert tuple(st.cam.cam.pix_offset) == offset
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size(), pix_offset=offset)
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    _compare_forward(oracle32, st, ost, cam, f"offset{offset}")
    _compare_backward(oracle32, st, t, ost, sc, f"offset{offset}")
    # the offset is not a no-op: centre pixels move by -offset
    st0, _ = hip_forward(device, sc, view, proj, H, W, pix_offset=(0.0, 0.0))
    vis = (st.radii > 0) & (st0.radii > 0)
    d = (st.rec[:, 16:18] - st0.rec[:, 16:18])[vis].cpu().numpy()
    assert np.abs(d[:, 0] + offset[0]).max() < 1e-3 and np.abs(d[:, 1] + offset[1]).max() < 1e-3


CASES = [
    # name, N, H, W, kwargs
    ("small_wrap", 3000, 32, 256, {}),
    ("c2_50k_64x1024", 50000, 64, 1024, {}),
    ("dense_near", 4000, 64, 512, dict(range_lo=1.0, range_hi=8.0, scale_lo=0.05, scale_hi=0.5)),
    ("ragged_size", 2500, 40, 200, dict(hfov_deg=120.0)),       # H, W not multiples of the tile, no wrap
    ("narrow_fov", 3000, 64, 512, dict(hfov_deg=90.0)),
    ("many_tiles", 20000, 128, 8192, {}),                       # 4096 tiles: two-pass tile sort + tile_ranges kernel
    ("aniso_tilted", 6000, 64, 1024, dict(range_lo=1.5, range_hi=12.0, scale_lo=0.01, scale_hi=0.6, max_tilt_deg=80.0)),   # thin, grazing surfels
]


@pytest.mark.parametrize("list_pairs", [2, 1], ids=["plain-list", "pairs-dense"])
@pytest.mark.parametrize("name,N,H,W,kw", CASES, ids=[c[0] for c in CASES])
def test_forward_backward_parity(device, oracle32, name, N, H, W, kw, list_pairs):
    """The drop-in interface (sls_forward_stage1/2 + sls_backward) against the checker, with the sorted list as a
    plain array (forward in rounds of 64 list entries) and as the tile sort's (surfel, block mask) pairs (forward in
    dense rounds: the kernels of sls_mapping_step; not possible beyond 2048 tiles, where the list stays plain)."""
    kw = dict(kw)
    hfov = kw.pop("hfov_deg", 360.0)
    sc, view, proj = scene_and_camera(N, H, W, seed=11, hfov_deg=hfov, **kw)
    if name == "dense_near":
        from splat_loam_amd import synth
        view, proj = synth.camera_matrices(sc["K"], synth.keyframe_poses(3)[2])
    st, t = hip_forward(device, sc, view, proj, H, W, list_pairs=list_pairs)
    assert st.vals_stride == (2 if (list_pairs == 1 and name != "many_tiles" and st.R > 0) else 1)
    from splat_loam_amd import _abi
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size())
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    assert cam.wrap == st.cam.cam.wrap
    wf, nfrag = _compare_forward(oracle32, st, ost, cam, name)
    wb = _compare_backward(oracle32, st, t, ost, sc, name)
    print(f"\n[{name}] R={st.R} fragile={nfrag} fwd worst={ {k: f'{v:.1e}' for k, v in wf.items()} } "
          f"bwd worst={ {k: f'{v:.1e}' for k, v in wb.items()} }")


@pytest.mark.parametrize("list_pairs", [2, 1], ids=["plain-list", "pairs-dense"])
def test_lean_allmap_through_the_drop_in_interface(device, oracle32, list_pairs):
    """The settings' extension `lean_allmap` (SlsCamera.flags bit 0, SLS_LEAN_ALLMAP=1): planes 5 and 6 are not
    tracked (zeros), planes 0-4 and the gradients for a dL/dallmap without those two channels are the checker's —
    the LEAN instantiations of the tile kernels, which sls_mapping_step runs, reached through GaussianRasterizer."""
    from splat_loam_amd import _abi
    N, H, W = 20000, 64, 512
    sc, view, proj = scene_and_camera(N, H, W, seed=27, range_lo=2.0, range_hi=30.0)
    st, t = hip_forward(device, sc, view, proj, H, W, list_pairs=list_pairs, lean_allmap=True)
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size())
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    am, oam, ok = st.allmap.cpu().numpy(), ost["allmap"], ~ost["fwd"]["fragile"]
    assert not am[5:7].any(), "lean: median / distortion planes are zeros"
    for c in range(5):
        e = np.abs(am[c].astype(np.float64) - oam[c]) / max(np.abs(oam[c]).max(), 1e-12)
        assert e[ok].max() <= RTOL, f"lean allmap ch{c}: {e[ok].max():.3e}"
    assert np.array_equal(u32(st.pix_contrib).reshape(-1, 2)[ok.reshape(-1), 0], ost["fwd"]["pixN"][ok.reshape(-1)])
    dL = np.random.default_rng(5).normal(size=(7, H, W)).astype(np.float32)
    dL[:, ~ok] = 0.0
    dL[5:7] = 0.0
    dm, ds, dr, do, _ = hip_backward(st, t, dL)
    ob = oracle32.backward(ost, dL, threads=1, want_abs=False)
    for nm, a, ref in (("means", dm, ob["dmeans"]), ("scales", ds, ob["dscales"]), ("opac", do, ob["dopac"]),
                       ("rots", tangent(dr.astype(np.float64), sc["rots"].astype(np.float64)),
                        tangent(ob["drots"].astype(np.float64), sc["rots"].astype(np.float64)))):
        e = np.abs(a.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30)
        assert e <= RTOL, f"lean d{nm}: {e:.3e}"


def test_tile_consumed_matches(device, oracle32):
    from splat_loam_amd import _abi
    N, H, W = 20000, 64, 512
    sc, view, proj = scene_and_camera(N, H, W, seed=5, range_lo=2.0, range_hi=20.0)
    st, _ = hip_forward(device, sc, view, proj, H, W)
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size())
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    a, b = u32(st.tile_consumed), ost["fwd"]["tile_consumed"]
    frag_tiles = ost["fwd"]["fragile"].reshape(cam.GY, cam.tile[1], cam.GX, cam.tile[0]).any(axis=(1, 3)).reshape(-1)
    assert np.array_equal(a[~frag_tiles], b[~frag_tiles])


def test_empty_and_culled(device):
    """N = 0, and every surfel behind the near cut: empty image, zero gradients."""
    from splat_loam_amd import synth
    H, W = 32, 128
    K = synth.spherical_K(H, W)
    view, proj = synth.camera_matrices(K)
    sc = dict(K=K, means=np.zeros((0, 3), np.float32), scales=np.zeros((0, 2), np.float32),
              rots=np.zeros((0, 4), np.float32), opac=np.zeros((0, 1), np.float32))
    st, t = hip_forward(device, sc, view, proj, H, W)
    assert st.R == 0 and float(st.allmap.abs().max()) == 0.0
    sc2 = synth.make_scene(100, H, W, seed=1, range_lo=0.01, range_hi=0.15)   # all nearer than 0.2 m
    st, t = hip_forward(device, sc2, view, proj, H, W)
    assert st.R == 0 and int((st.radii > 0).sum()) == 0
    assert float(st.allmap.abs().max()) == 0.0
    dm, ds, dr, do, _ = hip_backward(st, t, np.ones((7, H, W), np.float32))
    assert not dm.any() and not ds.any() and not dr.any() and not do.any()


def test_single_surfel_known_answer(device):
    """A fronto-parallel surfel centred on a pixel ray at range r:
    alpha = min(0.99, o), depth = r * alpha, normal = -ray (sensor frame)."""
    from splat_loam_amd import synth
    H, W = 32, 128
    K = synth.spherical_K(H, W).astype(np.float64)
    view, proj = synth.camera_matrices(K.astype(np.float32))
    c, r, rng_m, o = 40, 12, 7.5, 0.8
    az, el = (c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1]
    ray = np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
    tn = -ray
    helper = np.array([0.0, 0.0, 1.0])
    tu = np.cross(tn, helper); tu /= np.linalg.norm(tu)
    tv = np.cross(tn, tu)
    q = synth._quat_from_R(np.stack([tu, tv, tn], 1)[None])[0]
    sc = dict(K=K.astype(np.float32), means=(ray * rng_m)[None].astype(np.float32),
              scales=np.array([[0.3, 0.3]], np.float32), rots=q[None].astype(np.float32),
              opac=np.array([[o]], np.float32))
    st, _ = hip_forward(device, sc, view, proj, H, W)
    am = st.allmap.cpu().numpy()
    assert abs(am[1, r, c] - o) < 2e-5
    assert abs(am[0, r, c] - rng_m * o) < 2e-4
    assert np.abs(am[2:5, r, c] - (-ray) * o).max() < 2e-5
    assert abs(am[5, r, c] - rng_m) < 1e-4         # median depth = the only surfel
    assert int(st.radii[0]) > 0


def test_autograd_function_matches_raw_calls(device):
    """GaussianRasterizer (autograd) == rasterize_forward/backward, allmap may be
    overwritten in place by the caller before backward."""
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    N, H, W = 2000, 32, 256
    sc, view, proj = scene_and_camera(N, H, W, seed=2)
    st, t = hip_forward(device, sc, view, proj, H, W)
    dL = np.random.default_rng(0).normal(size=(7, H, W)).astype(np.float32)
    ref = hip_backward(st, t, dL)
    settings = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device),
                                             torch.tensor(proj, device=device), False, False)
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    radii, allmap = GaussianRasterizer(raster_settings=settings)(
        means3D=leaves["means"], means2D=torch.zeros_like(leaves["means"]), opacities=leaves["opac"],
        scales=leaves["scales"], rotations=leaves["rots"], cov3D_precomp=None)
    assert torch.equal(allmap, st.allmap) and torch.equal(radii, st.radii)
    loss = (allmap * torch.tensor(dL, device=device)).sum()
    allmap.data.mul_(0.0)          # caller scribbles over allmap before backward
    loss.backward()
    for k, r in (("means", ref[0]), ("scales", ref[1]), ("rots", ref[2]), ("opac", ref[3])):
        g = leaves[k].grad.cpu().numpy()
        scale = max(np.abs(r).max(), 1e-30)
        assert np.abs(g - r).max() / scale <= 1e-5, k   # float atomics reorder sums between runs


@pytest.mark.parametrize("N,H,W,kw,pairs", [(6000, 32, 256, dict(range_lo=2.0, range_hi=15.0, scale_hi=0.25), "1"),
                                            (6000, 32, 256, dict(range_lo=2.0, range_hi=15.0, scale_hi=0.25), "2"),
                                            (50000, 64, 1024, {}, "2"), (50000, 64, 1024, {}, "1"),
                                            (5000, 40, 200, dict(range_lo=2.0, range_hi=15.0, scale_hi=0.25), "2"),
                                            (500000, 64, 2048, {}, "0")],
                         ids=["small-pairs", "small-plain", "c2-plain", "c2-pairs", "ragged-plain", "c3-auto"])
def test_workspace_path_matches_staged_path(device, monkeypatch, N, H, W, kw, pairs):
    """VERDICT r04 item 1(c).  GaussianRasterizer's default path — sls_forward_ws / sls_backward_ws: one call each, a
    capacity instead of the host read of R, the camera's previous depth order repaired, gradient records cleared where
    they are read — against the staged calls on the same inputs: radii and allmap to the BIT (the forward has no
    atomics; the list is the same list whether sorted or repaired), gradients to 5e-6 of their scale (float atomics on both sides: two runs of ONE path differ by 1e-6 already).
    Five calls on one camera with the surfels moving in between: from-scratch sort, then repairs; then a capacity that
    is too small (the forward repeats itself with more room) and a graph dropped without a backward.  `pairs`: the list
    form (SLS_BLOCK_MASKS) — the automatic rule looks at the capacity here and at R there, and the two forward kernels
    it chooses between agree to rounding only, so the form is pinned except at C3, where both rules choose pairs."""
    monkeypatch.setenv("SLS_BLOCK_MASKS", pairs)
    from splat_loam_amd import rasterizer
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    sc, view, proj = scene_and_camera(N, H, W, seed=31, **kw)
    settings = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device), False, False)
    rng = np.random.default_rng(5)
    dL = torch.tensor(rng.normal(size=(7, H, W)).astype(np.float32), device=device)
    base = {k: torch.tensor(sc[k], device=device) for k in ("means", "scales", "rots", "opac")}
    rasterizer._WS_CACHE.clear()

    def run(t, staged):
        monkeypatch.setenv("SLS_STAGED_FORWARD", "1" if staged else "0")
        leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
        radii, allmap = GaussianRasterizer(raster_settings=settings)(
            means3D=leaves["means"], means2D=torch.zeros_like(leaves["means"]), opacities=leaves["opac"],
            scales=leaves["scales"], rotations=leaves["rots"], cov3D_precomp=None)
        out = (radii.clone(), allmap.clone())
        (allmap * dL).sum().backward()
        return out, {k: v.grad.clone() for k, v in leaves.items()}

    for it in range(5):
        t = dict(base)
        t["means"] = base["means"] + 3e-4 * it * torch.tensor(rng.normal(size=(N, 3)).astype(np.float32), device=device)
        (r_ws, a_ws), g_ws = run(t, staged=False)
        (r_st, a_st), g_st = run(t, staged=True)
        assert torch.equal(r_ws, r_st) and torch.equal(a_ws, a_st), f"call {it}"
        for k in g_st:
            scale = float(g_st[k].abs().max())
            assert float((g_ws[k] - g_st[k]).abs().max()) <= 5e-6 * scale, (it, k)
    ent = next(iter(rasterizer._WS_CACHE.values()))
    assert ent.stats["from_scratch"] >= 1 and ent.stats["repaired"] + ent.stats["repair_failed"] >= 4 and ent.stats["repaired"] >= 2 and not ent.busy, ent.stats
    # a capacity that is too small: the forward notices on the device, takes more room and repeats itself
    rasterizer._ws_alloc(ent, device, N, H, W, max(ent.stats["R"] // 2, 4096))
    (r_ws, a_ws), _ = run(base, staged=False)
    (r_st, a_st), _ = run(base, staged=True)
    assert ent.stats["too_small"] >= 1 and ent.cap >= ent.stats["R"] and torch.equal(a_ws, a_st) and torch.equal(r_ws, r_st)
    # no_grad takes no lease; a graph that is dropped without a backward gives the workspace back
    monkeypatch.setenv("SLS_STAGED_FORWARD", "0")
    with torch.no_grad():
        _, a_ng = GaussianRasterizer(raster_settings=settings)(means3D=base["means"], means2D=base["means"], opacities=base["opac"],
                                                             scales=base["scales"], rotations=base["rots"])
    assert torch.equal(a_ng, a_st) and not ent.busy
    m = base["means"].clone().requires_grad_(True)
    _, a_kept = GaussianRasterizer(raster_settings=settings)(means3D=m, means2D=m, opacities=base["opac"], scales=base["scales"], rotations=base["rots"])
    assert ent.busy
    # ... while it is held, another forward of the same size takes the staged path instead of waiting
    _, a_other = GaussianRasterizer(raster_settings=settings)(means3D=m, means2D=m, opacities=base["opac"], scales=base["scales"], rotations=base["rots"])
    assert torch.equal(a_other, a_st)
    del a_kept, a_other
    import gc; gc.collect()
    assert not ent.busy


@pytest.mark.parametrize("seed,yaw_deg,size", [(11, 0.0, (96, 32, 128)), (12, 171.0, (96, 32, 128)), (21, 0.0, (2000, 64, 512))],
                         ids=["seed11", "seed12-seam", "seed21-2000-64x512"])
def test_hip_against_the_float64_autograd_formulation(device, oracle64, oracle32, seed, yaw_deg, size):
    """VERDICT r04 item 2 (and weak #1): the HIP path against oracle/torch_ref.py directly — a dense float64 torch
    formulation that shares NO arithmetic with the kernels: the textbook ray-plane form x = t d, u = Tu.(x - p)/su instead
    of the kernels' cancellation-free one, torch's own sin / cos / atan2 / norm, gradients from autograd instead of
    hand-written derivatives.  The non-differentiable givens (tile rectangles, depth order, the centre pixel's value) are
    taken from the HIP forward's own buffers and the ray tables from NumPy, so nothing compiled from include/sls_*.h
    enters the reference value; the checker only says which pixels are fragile.  96 surfels on a
    32x128 image that wraps; `seed12-seam`: the sensor turned so that the surfels cluster at the azimuth seam.
    Bars (max-norm per plane / tensor, non-fragile pixels, rotations in the tangent space of the unit quaternion; fixed
    numbers, no alternatives): radii / rectangles equal; allmap 2e-5 in both scenes; gradients 2e-5 in the generic scene
    and 5e-4 in the seam scene.  These are float32 against EXACT arithmetic, not float32 against float32 as the north
    star's 1e-5.  The seam scene packs the 96 surfels into 80 degrees of azimuth: 30-40 mostly opaque surfels blended per
    pixel, and the backward recovers every transmittance by division ([LINEAGE], as the kernels and the checker both
    do) — there the float32 CHECKER itself is 1.3e-4 (seed 12; 2.4e-4 at seed 13) from float64 while the kernels sit on
    it to 1e-6, which the last assertion holds them to (1e-5).  Measured: generic scene 2e-6, seam scene 1.35e-4.
    `seed21-2000-64x512`: 2 000 surfels on 64x512 — 128 tiles, lists of a hundred entries, every
    kernel's wave / window / chunk granularity crossed — through torch_ref.dense_forward_tiled (the same formulation
    with the tiles as a batch; tests/test_oracle.py holds it to dense_forward): same bars as the generic scene."""
    F64_TOL, F64_TOL_GRAD = 2e-5, (5e-4 if yaw_deg else 2e-5)
    from oracle import torch_ref
    from splat_loam_amd import synth
    N, H, W = size
    big = N > 500
    sc = (synth.make_scene(N, H, W, seed=seed, range_lo=2.0, range_hi=15.0, scale_lo=0.05, scale_hi=0.3) if big else
          synth.make_scene(N, H, W, seed=seed, range_lo=2.0, range_hi=8.0, scale_lo=0.05, scale_hi=0.4))
    pose = np.eye(4)
    if yaw_deg:
        # everything behind the sensor: azimuths within +-40 degrees of the seam
        rng = np.random.default_rng(seed)
        rho = np.linalg.norm(sc["means"], axis=1)
        az = np.pi + np.radians(rng.uniform(-40, 40, N))
        el = np.arcsin(sc["means"][:, 2] / rho)
        sc["means"] = (rho[:, None] * np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], 1)).astype(np.float32)
    view, proj = synth.camera_matrices(sc["K"], pose)
    st, t = hip_forward(device, sc, view, proj, H, W)
    cam = oracle64.camera(H, W, view.astype(np.float64), proj)
    a64 = [np.asarray(sc[k], np.float64) for k in ("means", "scales", "rots", "opac")]
    ost = oracle64.forward(cam, *a64)
    pre = ost["pre"]
    assert np.array_equal(st.radii.cpu().numpy(), pre["radii"])
    vis = pre["radii"] > 0
    assert np.array_equal(st.rect.cpu().numpy()[vis], pre["rect"][vis])
    GX = W // 16
    assert cam.wrap == 1 and (not yaw_deg or ((pre["rect"][vis, 0] + pre["rect"][vis, 1]) > GX).sum() >= 5), "the seam case must have rectangles that wrap"
    leaves = [torch.tensor(a, requires_grad=True) for a in a64]
    # What the float64 formulation takes as given comes from the HIP forward ITSELF, not from the checker's C code: the
    # integer decisions (radii, rectangles, depth keys: just compared) and the surfels' centre pixels out of the kernels'
    # records; the pixel rays from NumPy (double, rounded once to float as sls_ray_tables defines them).  The checker
    # contributes the Camera container and the fragile-pixel mask — which pixels are compared, not what they hold.
    fx, fy, cx, cy = (float(np.float32(v)) for v in (sc["K"][0, 0], sc["K"][1, 1], sc["K"][0, 2], sc["K"][1, 2]))
    azc, elr = (np.arange(W, dtype=np.float64) - cx) / fx, (np.arange(H, dtype=np.float64) - cy) / fy
    tables = (np.stack([np.cos(azc), np.sin(azc)], 1).astype(np.float32).astype(np.float64),
              np.stack([np.cos(elr), np.sin(elr)], 1).astype(np.float32).astype(np.float64))
    assert np.abs(tables[0] - ost["tables"][0]).max() <= 1e-7 and np.abs(tables[1] - ost["tables"][1]).max() <= 1e-7
    pre_hip = {"rec": st.rec.cpu().numpy().astype(np.float64), "radii": st.radii.cpu().numpy(), "rect": st.rect.cpu().numpy(),
               "depth": st.depth.cpu().numpy()}
    am64 = (torch_ref.dense_forward_tiled if big else torch_ref.dense_forward)(cam, tables, pre_hip, *leaves)
    ok = ~ost["fwd"]["fragile"]
    am = st.allmap.cpu().numpy().astype(np.float64)
    ref = am64.detach().numpy()
    for c in range(7):
        scale = max(np.abs(ref[c]).max(), 1e-12)
        if c == 6:      # the distortion is a difference of O(1) terms that nearly cancel: the error is relative to those
            scale = max(scale, 1.0)
        assert (np.abs(am[c] - ref[c]) / scale)[ok].max() <= F64_TOL, f"allmap plane {c}"
    dL = np.random.default_rng(3).normal(size=(7, H, W))
    dL[5] = 0                      # the median plane is piecewise constant in the parameters
    dL[:, ~ok] = 0
    (am64 * torch.tensor(dL)).sum().backward()
    g = hip_backward(st, t, dL.astype(np.float32))
    q = a64[2]
    for name, got, want in (("means", g[0], leaves[0].grad.numpy()), ("scales", g[1], leaves[1].grad.numpy()),
                            ("rots", tangent(g[2].astype(np.float64), q), tangent(leaves[2].grad.numpy(), q)),
                            ("opac", g[3], leaves[3].grad.numpy())):
        scale = np.abs(want).max()
        print(f"[f64 {N}@{H}x{W} seed {seed}] {name}: {np.abs(got - want).max() / scale:.2e}")
        assert np.abs(got - want).max() <= F64_TOL_GRAD * scale, (name, np.abs(got - want).max() / scale)
    # ... and against the float32 checker on the same inputs and the same dL: the north star's bar
    ost32 = oracle32.forward(oracle32.camera(H, W, view, proj, tile=(16, 16)), sc["means"], sc["scales"], sc["rots"], sc["opac"])
    b32 = oracle32.backward(ost32, dL.astype(np.float32), want_abs=False)
    for name, got, want in (("means", g[0], b32["dmeans"]), ("scales", g[1], b32["dscales"]), ("opac", g[3], b32["dopac"]),
                            ("rots", tangent(g[2].astype(np.float64), q), tangent(b32["drots"].astype(np.float64), q))):
        assert np.abs(got - want).max() <= RTOL * np.abs(want).max(), (name, "float32 checker")


@pytest.mark.parametrize("N,H,W,shrink", [(1, 32, 256, 1.0), (3, 32, 256, 1.0), (64, 32, 256, 1.0), (2, 16, 16, 1.0), (7, 48, 80, 1.0),
                                          (300, 32, 256, 1e-3)], ids=["1", "3", "64", "one-tile", "ragged-7", "all-culled"])
def test_workspace_path_edge_sizes(device, monkeypatch, N, H, W, shrink):
    """The one-call path at the sizes where a chunk, a wave or a tile is not full — one surfel, fewer than a wave, a
    single tile, an image that is no multiple of the tile — and with EVERY surfel inside the near cut (R = 0, twice: the
    second call repairs an order of nothing): same radii and image as the staged calls, finite gradients."""
    from splat_loam_amd import rasterizer, synth
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    sc = synth.make_scene(N, H, W, seed=1, range_lo=2.0, range_hi=15.0, scale_hi=0.25)
    sc["means"] = (sc["means"] * shrink).astype(np.float32)
    view, proj = synth.camera_matrices(sc["K"], np.eye(4) if shrink != 1.0 else synth.keyframe_poses(2)[1])
    settings = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device), False, False)
    rasterizer._WS_CACHE.clear()
    out = {}
    for staged in ("0", "1"):
        monkeypatch.setenv("SLS_STAGED_FORWARD", staged)
        monkeypatch.setenv("SLS_BLOCK_MASKS", "2")
        for _ in range(2):
            t = {k: torch.tensor(sc[k], device=device).requires_grad_(True) for k in ("means", "scales", "rots", "opac")}
            radii, am = GaussianRasterizer(raster_settings=settings)(means3D=t["means"], means2D=t["means"], opacities=t["opac"],
                                                                    scales=t["scales"], rotations=t["rots"])
            am.sum().backward()
        out[staged] = (radii.clone(), am.detach().clone(), t["means"].grad.clone())
    ent = next(iter(rasterizer._WS_CACHE.values()))
    assert ent.stats["from_scratch"] + ent.stats["repaired"] == 2, "the one-call path was not taken"
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])
    assert bool(torch.isfinite(out["0"][2]).all())
    scale = float(out["1"][2].abs().max())
    assert float((out["0"][2] - out["1"][2]).abs().max()) <= 5e-6 * scale + 0.0
    if shrink != 1.0:
        assert ent.stats["R"] == 0 and not bool((out["0"][0] > 0).any()) and float(out["0"][1].abs().max()) == 0.0


def test_workspace_path_second_backward_and_held_graph(device, monkeypatch):
    """(a) a graph walked twice (retain_graph=True) — the second walk finds the workspace gone and repeats the
    forward through the staged calls instead of raising: same gradients both times; (b) a result that is kept alive
    without a backward holds the workspace: the next forward of that size takes the staged path AND says so once;
    (c) a new surfel count inherits the instances-per-surfel the old size saw (no overflow-and-repeat on its first call)."""
    import warnings
    from splat_loam_amd import rasterizer, synth
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    monkeypatch.setenv("SLS_STAGED_FORWARD", "0")
    N, H, W = 6000, 64, 512
    sc = synth.make_scene(N, H, W, seed=12, range_lo=2.0, range_hi=15.0, scale_hi=0.25)
    view, proj = synth.camera_matrices(sc["K"])
    settings = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device), False, False)
    dL = torch.tensor(np.random.default_rng(0).normal(size=(7, H, W)).astype(np.float32), device=device)
    rasterizer._WS_CACHE.clear()
    rasterizer._WARNED.clear()

    def render(n=N):
        t = {k: torch.tensor(sc[k][:n], device=device).requires_grad_(True) for k in ("means", "scales", "rots", "opac")}
        _, am = GaussianRasterizer(raster_settings=settings)(means3D=t["means"], means2D=t["means"], opacities=t["opac"],
                                                             scales=t["scales"], rotations=t["rots"])
        return t, am
    # (a)
    t, am = render()
    loss = (am * dL).sum()
    loss.backward(retain_graph=True)
    first = {k: v.grad.clone() for k, v in t.items()}
    for v in t.values():
        v.grad = None
    loss.backward()
    for k, v in t.items():
        scale = float(first[k].abs().max())
        assert float((v.grad - first[k]).abs().max()) <= 5e-6 * scale, k
    ent = next(iter(rasterizer._WS_CACHE.values()))
    assert not ent.busy
    # (b)
    t1, held = render()
    assert ent.busy
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        t2, am2 = render()
        render()
    assert sum("staged path" in str(x.message) for x in w) == 1, [str(x.message) for x in w]
    assert torch.equal(am2.detach(), held.detach())
    (held * dL).sum().backward()
    assert not ent.busy
    # (c)
    seen = ent.stats["R"]
    n2 = N - 500
    render(n2)[1].sum().backward()
    ent2 = next(v for k, v in rasterizer._WS_CACHE.items() if k[1] == n2)
    assert ent2.cap_hint >= seen * n2 // N and ent2.stats["too_small"] == 0 and ent2.cap >= ent2.stats["R"]


def test_binning_with_rectangles_that_cover_the_image(device, oracle32, monkeypatch):
    """VERDICT r04 item 4.  Surfels within a metre of the sensor have tile rectangles of hundreds of tiles (up to all 512
    at 64x2048) and sit together at the front of the depth order: one wave of bin_direct_kernel then has hundreds of
    rounds where the others have ten (profiles/r05a_bin_tail.txt).  The kernels count such rectangles with the whole
    wave and emit their single-owner rounds without ranking; this scene — 20 k surfels from 0.25 m out, 2 300 of them
    with more than 48 tiles — checks that the lists stay the checker's to the bit: staged calls (gather_count +
    bin_direct), the one-call path from scratch, and repaired (resort_merge's counting)."""
    from splat_loam_amd import _abi, rasterizer, synth
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    N, H, W = 20000, 64, 2048
    sc = synth.make_scene(N, H, W, seed=77, range_lo=0.25, range_hi=20.0, scale_lo=0.03, scale_hi=0.2)
    view, proj = synth.camera_matrices(sc["K"], synth.keyframe_poses(2)[1])
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size())
    oracle32.set_threads(oracle32.max_threads())
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    tiles = ost["pre"]["tiles"]
    assert (tiles > 48).sum() >= 1000 and tiles.max() >= 400, (int((tiles > 48).sum()), int(tiles.max()))
    for pairs in ("2", "1"):
        monkeypatch.setenv("SLS_BLOCK_MASKS", pairs)
        st, t = hip_forward(device, sc, view, proj, H, W, list_pairs=int(pairs))
        assert st.R == ost["binned"]["R"]
        assert np.array_equal(u32(st.vals), ost["binned"]["vals"]) and np.array_equal(u32(st.ranges), ost["binned"]["ranges"])
        assert np.array_equal(st.keys.cpu().numpy().view(np.uint64), ost["binned"]["keys"])
        # the one-call path: from scratch, then twice repaired (surfels nudged), against the staged image to the bit
        rasterizer._WS_CACHE.clear()
        monkeypatch.setenv("SLS_STAGED_FORWARD", "0")
        settings = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device), False, False)
        for it in range(3):
            means = t["means"] + 1e-4 * it
            with torch.no_grad():
                _, a_ws = GaussianRasterizer(raster_settings=settings)(means3D=means, means2D=means, opacities=t["opac"], scales=t["scales"], rotations=t["rots"])
            sc_it = dict(sc); sc_it["means"] = means.cpu().numpy()
            st_it, _ = hip_forward(device, sc_it, view, proj, H, W, list_pairs=int(pairs))
            assert torch.equal(a_ws, st_it.allmap), (pairs, it)
        ent = next(iter(rasterizer._WS_CACHE.values()))
        assert ent.stats["repaired"] >= 1, ent.stats


def test_cpu_tensors_are_refused():
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(8, 16, 1.0, torch.eye(4), torch.eye(4), False, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianRasterizer(raster_settings=s)(means3D=torch.zeros(1, 3), means2D=torch.zeros(1, 3),
                                              opacities=torch.zeros(1, 1), scales=torch.ones(1, 2),
                                              rotations=torch.tensor([[1.0, 0, 0, 0]]), cov3D_precomp=None)


def test_knn_bitexact(device, oracle32):
    from splat_loam_amd.knn import distCUDA2
    from splat_loam_amd import synth
    # sizes around the kernel's granularities: 32-point runs, 64-point waves, 256-point boxes, 64-box chunks
    for M, seed in ((1, 0), (3, 1), (4, 2), (31, 5), (63, 6), (64, 7), (65, 8), (255, 9), (256, 10), (257, 3), (513, 11),
                    (6000, 4), (20000, 12)):
        pts = synth.make_scene(M, 64, 1024, seed=seed)["means"]
        got = distCUDA2(torch.tensor(pts, device=device)).cpu().numpy()
        ref = oracle32.knn_dist2(pts)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"M={M}"
    # (M = 20 000 is two chunks of boxes) waves without a query leave early while the others sweep both chunks
    for first in (1, 64, 10000):
        part = distCUDA2(torch.tensor(pts, device=device), first=first).cpu().numpy()
        assert part.shape == (first,) and np.array_equal(part.view(np.uint32), ref[:first].view(np.uint32)), first
    # duplicates and collinear points
    pts = np.repeat(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 0, 0]], np.float32), 3, axis=0)
    got = distCUDA2(torch.tensor(pts, device=device)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), oracle32.knn_dist2(pts).view(np.uint32))
    # a LiDAR-like cloud: two walls, a dense cluster, isolated far returns and 300 copies of one point
    # (very different local densities in one wave, zero distances, bounds that must stay conservative)
    rng = np.random.default_rng(21)
    wall1 = np.stack([rng.uniform(-20, 20, 6000), np.full(6000, 8.0), rng.uniform(-2, 3, 6000)], 1)
    wall2 = np.stack([np.full(4000, -15.0), rng.uniform(-30, 30, 4000), rng.uniform(-2, 6, 4000)], 1)
    cluster = rng.normal(0, 0.02, (3000, 3)) + np.array([3.0, -2.0, 0.5])
    far = rng.uniform(-150, 150, (40, 3))
    same = np.tile(np.array([[1.25, 2.5, -0.75]]), (300, 1))
    pts = np.concatenate([wall1, wall2, cluster, far, same]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    got = distCUDA2(torch.tensor(pts, device=device)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), oracle32.knn_dist2(pts).view(np.uint32))
    # queries = the first `first` points only (what Mapper.densify keeps): the same bits as the full call's head
    full = torch.tensor(got, device=device)
    t = torch.tensor(pts, device=device)
    for first in (1, 63, 64, 700, len(pts) - 1, len(pts)):
        part = distCUDA2(t, first=first)
        assert part.shape == (first,) and torch.equal(part.view(torch.int32), full[:first].view(torch.int32)), first
    assert distCUDA2(t, first=0).shape == (0,)


def test_fused_adam_matches_torch(device):
    from splat_loam_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(0)
    shapes = [(1001, 3), (1001, 1), (1001, 2), (1001, 4)]
    lrs = [5e-4, 5e-2, 5e-3, 1e-3]
    p_ref = [torch.randn(s, generator=g) for s in shapes]
    p_hip = [p.clone().to(device).requires_grad_(True) for p in p_ref]
    p_ref = [p.clone().requires_grad_(True) for p in p_ref]
    o_ref = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(p_ref, lrs)], lr=0.0, eps=1e-15)
    o_hip = FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(p_hip, lrs)], lr=0.0, eps=1e-15)
    for it in range(5):
        for a, b in zip(p_ref, p_hip):
            gr = torch.randn(a.shape, generator=g) * (10.0 ** (it - 2))
            a.grad = gr.clone()
            b.grad = gr.clone().to(device)
        o_ref.step(); o_hip.step()
    for a, b in zip(p_ref, p_hip):
        # torch's CPU kernels fuse some multiply-adds (lerp/addcmul), ours do not: compare
        # relative to the tensor scale
        def close(x, y):
            return float((x - y).abs().max()) <= 2e-6 * float(x.abs().max())
        sa, sb = o_ref.state[a], o_hip.state[b]
        assert close(a.detach(), b.detach().cpu())
        assert close(sa["exp_avg"], sb["exp_avg"].cpu())
        assert close(sa["exp_avg_sq"], sb["exp_avg_sq"].cpu())
        assert int(sb["step"]) == 5


def test_mark_visible(device):
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    H, W = 32, 128
    sc, view, proj = scene_and_camera(500, H, W, seed=3, range_lo=0.05, range_hi=5.0)
    s = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device))
    vis = GaussianRasterizer(raster_settings=s).markVisible(torch.tensor(sc["means"], device=device)).cpu().numpy()
    rho = np.linalg.norm(sc["means"].astype(np.float64), axis=1)
    sure = np.abs(rho - 0.2) > 1e-5
    assert np.array_equal(vis[sure], (rho >= 0.2)[sure])


def test_full_size_properties(device):
    """BASELINE config 3 size (500k surfels, 64x2048): size-independent properties."""
    N, H, W = 500000, 64, 2048
    sc, view, proj = scene_and_camera(N, H, W, seed=0)
    st, t = hip_forward(device, sc, view, proj, H, W)
    keys = st.keys.cpu().numpy().view(np.uint64)
    vals = u32(st.vals)
    assert st.R == int(u32(st.tiles).sum())
    assert np.all(keys[1:] >= keys[:-1]), "keys sorted"
    same = keys[1:] == keys[:-1]
    assert np.all(vals[1:][same] > vals[:-1][same]), "stable: equal keys keep surfel order"
    # the sorted pairs are a permutation of the emitted pairs: checksum of (tile, surfel) pairs
    depth_bits = u32(st.depth)
    assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), depth_bits[vals]), "payload follows key"
    tiles_of = np.bincount(vals, minlength=N)
    assert np.array_equal(tiles_of.astype(np.uint32), u32(st.tiles)), "every surfel emitted tiles_touched times"
    rng = u32(st.ranges).reshape(-1, 2)
    tile_ids = (keys >> np.uint64(32)).astype(np.int64)
    cnt = np.bincount(tile_ids, minlength=rng.shape[0])
    assert np.array_equal((rng[:, 1] - rng[:, 0]).astype(np.int64), cnt), "ranges partition the list"
    # hip_forward IS the production path of the drop-in interface: ranges from the tile sort's digit bases, and at this
    # size (R >= 1500 instances per tile) the list as (surfel, block mask) pairs with the forward in dense rounds —
    # the kernels sls_mapping_step runs.  Against it: the same forward with plain lists and rounds of 64 entries.
    assert st.vals_stride == 2 and st.block_masks_shape == 3, "C3 through the staged API runs the dense forward"
    from splat_loam_amd.rasterizer import GaussianRasterizationSettings, rasterize_forward
    s2 = GaussianRasterizationSettings(H, W, 1.0, torch.tensor(view, device=device), torch.tensor(proj, device=device))
    st2 = rasterize_forward(s2, t["means"], t["opac"], t["scales"], t["rots"], list_pairs=2)
    assert st2.vals_stride == 1
    assert st2.R == st.R and np.array_equal(u32(st2.vals), vals), "plain-list path: same sorted list"
    assert np.array_equal(u32(st2.ranges).reshape(-1, 2), rng), "plain-list path: same ranges"
    # (same entries in the same order, but a pixel's four partial sums are split differently over the steps)
    scale = st.allmap.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-12)
    scale[6] = scale[6].clamp_min(1.0)      # (distortion: a difference of O(1) terms that nearly cancel, as in _compare_forward)
    assert ((st2.allmap - st.allmap).abs() / scale).max().item() <= 2e-6
    assert torch.equal(st2.pix_contrib, st.pix_contrib)
    am = st.allmap.cpu().numpy()
    assert np.isfinite(am).all()
    assert am[1].min() >= 0.0 and am[1].max() <= 1.0, "alpha in [0,1] (fed to BCE, slam/mapper.py:182)"
    nrm = np.linalg.norm(am[2:5], axis=0)
    assert np.all(nrm <= am[1] + 1e-4), "|sum w n| <= sum w"
    # forward is deterministic (no atomics): bit-identical on a second run
    st2, _ = hip_forward(device, sc, view, proj, H, W)
    assert torch.equal(st.allmap, st2.allmap) and torch.equal(st.vals, st2.vals)
    # backward: finite, linear in dL
    g = np.random.default_rng(1)
    d1 = g.normal(size=(7, H, W)).astype(np.float32)
    d2 = g.normal(size=(7, H, W)).astype(np.float32)
    b1, b2, b12 = hip_backward(st, t, d1), hip_backward(st, t, d2), hip_backward(st, t, d1 + d2)
    for x, y, z in zip(b1[:4], b2[:4], b12[:4]):
        assert np.isfinite(z).all()
        scale = np.abs(z).max()
        assert np.abs((x + y) - z).max() <= 2e-4 * scale, "backward is linear in dL/dallmap"


def test_fused_consumer_matches_torch_render_and_loss(device):
    """sls_consumer_fwd_bwd == the loss of render() + slam/mapper.py:158-187 in value and in dL/dallmap, on RENDERED
    images, against the float64 reference (oracle/consumer_ref.py with torch's BCE; tests/test_consumer_math.py pins it
    to mapping_loss(postprocess(allmap)), which G2/G5 pin to the reference project).  Per pixel, at the values where the
    kernels branch and at a bar that follows float32's own cost: tests/test_consumer_parity.py."""
    from oracle.consumer_ref import pixel_loss64
    from splat_loam_amd import synth
    from splat_loam_amd.fused import fused_pixel_loss
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera
    for (H, W, ratio, hfov) in ((32, 256, 0.0, 360.0), (40, 200, 0.3, 120.0)):
        sc, view, proj = scene_and_camera(6000, H, W, seed=8, hfov_deg=hfov, range_lo=2.0, range_hi=15.0)
        depth, valid = synth.make_targets(H, W, sc)
        valid = valid.copy(); valid[0, :3, :7] = 0; valid[0, H // 2, ::5] = 0
        cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[1], data_device=str(device))
        view, proj = synth.camera_matrices(sc["K"], synth.keyframe_poses(2)[1])
        st, _ = hip_forward(device, sc, view, proj, H, W)
        cfg = MappingConfig(depth_ratio=ratio, opt_scaling_max_penalty=0.0)
        am1 = st.allmap.cpu().double().requires_grad_(True)         # float64 from the image on: no .float() on the way
        l_ref = pixel_loss64(am1, sc["K"], depth[0], valid[0] == 1, ratio, cfg.opt_lambda_normal, cfg.opt_lambda_alpha, bce="torch")[0]
        l_ref.backward()
        am2 = st.allmap.clone().requires_grad_(True)
        l_hip = fused_pixel_loss(am2, cam, cfg)
        (3.0 * l_hip).backward()
        assert abs(float(l_hip.detach()) - float(l_ref.detach())) <= 2e-5 * abs(float(l_ref.detach()))
        g_ref, g_hip = am1.grad.numpy(), am2.grad.cpu().numpy() / 3.0
        for c in range(7):
            scale = max(np.abs(g_ref[c]).max(), 1e-30)
            assert np.abs(g_hip[c] - g_ref[c]).max() <= 2e-4 * scale + 1e-12, (H, W, c)


def test_fused_step_matches_unfused_step(device):
    """optimize_step_fused (HIP consumer + fused Adam) tracks optimize_step (torch
    render/loss + torch Adam) over 3 iterations."""
    from splat_loam_amd import synth
    from splat_loam_amd.mapping import MappingConfig, optimize_step, optimize_step_fused
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 5000, 32, 256
    sc = synth.make_scene(N, H, W, seed=12, range_lo=2.0, range_hi=15.0, scale_hi=0.2)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, None, data_device=str(device))
    cfg = MappingConfig()
    a = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
    b = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
    a.training_setup(fused=False); b.training_setup(fused=True)
    names = ("_xyz", "_scaling", "_rotation", "_opacity")
    init = {k: getattr(a, k).detach().clone() for k in names}
    for _ in range(3):
        la = float(optimize_step(a, cam, cfg)); lb = float(optimize_step_fused(b, cam, cfg))
        assert abs(la - lb) <= 1e-4 * abs(la)
    for k in names:
        pa, pb = getattr(a, k).detach(), getattr(b, k).detach()
        moved = float((pa - init[k]).abs().max())
        # Adam normalises every gradient to a step of about lr, so surfels with a
        # near-zero gradient amplify rounding differences; bound the drift by a
        # fraction of the distance actually travelled
        assert moved > 0 and float((pa - pb).abs().max()) <= 0.05 * moved, k


def test_mapping_engine_matches_unfused_step(device):
    """sls_mapping_step (one native call per iteration, raw parameters, no host
    sync inside) == optimize_step (torch activations + torch render/loss + torch
    Adam): same loss, same gradients, same parameter trajectory; the instance
    buffers overflow once on purpose and the iteration is repeated."""
    _mapping_engine_matches_unfused_step(device, 0.0)


def test_mapping_engine_matches_unfused_step_depth_ratio_1(device):
    """The same at depth_ratio 1 — the median depth, as meshing renders it: the torch path render(cam, model, 1.0) +
    mapping_loss is the reference; the engine leaves its lean / fused path (kernels B and C launched, the tile backward
    carrying the median's gradient)."""
    _mapping_engine_matches_unfused_step(device, 1.0)


def _mapping_engine_matches_unfused_step(device, depth_ratio):
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig, mapping_loss
    from splat_loam_amd.renderer import render
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 6000, 32, 256
    sc = synth.make_scene(N, H, W, seed=14, range_lo=2.0, range_hi=15.0, scale_hi=0.25)
    depth, valid = synth.make_targets(H, W, sc)
    valid = valid.copy(); valid[0, :2, :9] = 0
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[1], data_device=str(device))
    cfg = MappingConfig(depth_ratio=depth_ratio)
    a = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"] * 1.7, sc["opac"], device=str(device))
    b = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"] * 1.7, sc["opac"], device=str(device))
    a.training_setup(fused=False)
    eng = MappingEngine(b, cfg)
    eng.keep_grads = True          # the test looks at the gradient bucket
    eng.capacity = 2048            # far too small: forces the overflow / retry path
    names = ("_xyz", "_scaling", "_rotation", "_opacity")
    init = {k: getattr(a, k).detach().clone() for k in names}
    for it in range(3):
        a.optimizer.zero_grad(set_to_none=True)
        loss = mapping_loss(render(cam, a, cfg.depth_ratio), cam, a, cfg)
        loss.backward()
        st = eng.step(cam)
        assert not st["overflow"] and st["R"] > 2048
        assert abs(st["loss"] - float(loss)) <= 1e-4 * abs(float(loss)), (it, st, float(loss))
        gv = eng.grad_views()
        for k, p in (("xyz", a._xyz), ("opacity", a._opacity), ("scaling", a._scaling), ("rotation", a._rotation)):
            ref = p.grad
            scale = float(ref.abs().max())
            assert float((gv[k] - ref).abs().max()) <= 2e-4 * scale, (it, k)
        with torch.no_grad():
            a.optimizer.step()
    for k in names:
        pa, pb = getattr(a, k).detach(), getattr(b, k).detach()
        moved = float((pa - init[k]).abs().max())
        assert moved > 0 and float((pa - pb).abs().max()) <= 0.05 * moved, k
    am = eng.allmap(H, W)
    assert torch.isfinite(am).all() and float(am[1].max()) <= 1.0


@pytest.mark.parametrize("deterministic", [False, True, 2], ids=["float-atomics", "deterministic", "deterministic-one-launch"])
def test_mapping_engine_lagged_status_read(device, deterministic):
    """sync="lagged" (status of iteration k read after iteration k+1 was enqueued)
    walks the same parameter trajectory and reports the same losses as the
    synchronous mode, also across an overflow of the instance buffers.  With deterministic accumulation
    (SlsMappingConfig.deterministic) "the same" is meant to the bit."""
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 6000, 32, 256
    sc = synth.make_scene(N, H, W, seed=15, range_lo=2.0, range_hi=15.0, scale_hi=0.25)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[1], data_device=str(device))
    cfg = MappingConfig()
    models = [SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
              for _ in range(2)]
    init = {k: getattr(models[0], k).detach().clone() for k in ("_xyz", "_scaling", "_rotation", "_opacity")}
    ref, lag = MappingEngine(models[0], cfg), MappingEngine(models[1], cfg)
    ref.deterministic = lag.deterministic = deterministic
    # (which forward kernel runs follows the instance capacity — dense rounds from 1500 instances per tile on — and the
    #  two engines end with different capacities; the two forwards agree to ~1e-7, not to the bit: pin the choice)
    ref.block_masks = lag.block_masks = 1
    lag.capacity = 2048            # overflows on the first two (pipelined) iterations
    n_it = 6
    ref_losses = [ref.step(cam)["loss"] for _ in range(n_it)]
    lag_losses = []
    for _ in range(n_it):
        st = lag.step(cam, sync="lagged")
        if st is not None:
            lag_losses.append(st["loss"])
    lag_losses.append(lag.flush()["loss"])
    assert lag.flush() is None and lag.t == ref.t == n_it and lag.capacity > 2048
    assert len(lag_losses) == n_it
    for a, b in zip(ref_losses, lag_losses):
        assert abs(a - b) <= 1e-5 * abs(a), (ref_losses, lag_losses)
    # (float atomics order the gradient sums differently from run to run and Adam amplifies that where
    # a gradient is ~0: compare against the distance travelled, as the engine-vs-torch test does)
    for k in ("_xyz", "_scaling", "_rotation", "_opacity"):
        pa, pb = getattr(models[0], k).detach(), getattr(models[1], k).detach()
        moved = float((pa - init[k]).abs().max())
        assert moved > 0 and float((pa - pb).abs().max()) <= 0.02 * moved, k
        if deterministic:
            assert torch.equal(pa, pb), f"deterministic accumulation: lagged and synchronous trajectories differ in {k}"


@pytest.mark.parametrize("deterministic", [False, True, 2], ids=["float-atomics", "deterministic", "deterministic-one-launch"])
@pytest.mark.parametrize("N", [30000, 4999], ids=["even-n", "odd-n"])   # odd N: separate optimiser kernel, unaligned scratch views
def test_mapping_engine_depth_order_repair(device, N, deterministic):
    """reuse_depth_order: repairing the previous iteration's depth order (windowed re-sort +
    exactness check) gives the same iterations as sorting from scratch; when the surfels are
    moved so far that the repair cannot reach the exact order, the iteration is flagged,
    its Adam update skipped, and it is repeated with the full sort."""
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    H, W = 32, 512
    sc = synth.make_scene(N, H, W, seed=16, range_lo=2.0, range_hi=25.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[1], data_device=str(device))
    cfg = MappingConfig()
    models = [SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
              for _ in range(2)]
    init = {k: getattr(models[0], k).detach().clone() for k in ("_xyz", "_scaling", "_rotation", "_opacity")}
    full, rep = MappingEngine(models[0], cfg), MappingEngine(models[1], cfg)
    full.deterministic = rep.deterministic = deterministic     # (then the two trajectories are compared to the bit)
    full.block_masks = rep.block_masks = 1
    full.reuse_depth_order = False
    losses = [[], []]
    for phase in range(2):
        for it in range(4):
            losses[0].append(full.step(cam)["loss"])
            mode = "lagged" if phase == 0 else True
            st = rep.step(cam, sync=mode)
            if st is not None:
                losses[1].append(st["loss"])
        st = rep.flush()
        if st is not None:
            losses[1].append(st["loss"])
        if phase == 0:
            assert rep.stats["repeated_resort"] == 0, "small Adam steps must be repairable"
            g = torch.Generator(device="cpu").manual_seed(5)
            f = (0.6 + 0.8 * torch.rand((N, 1), generator=g)).to(device)      # reshuffles the depth order
            with torch.no_grad():
                for m in models:
                    m._xyz.mul_(f)
    assert rep.stats["repeated_resort"] == 1 and full.stats["repeated_resort"] == 0
    assert rep.t == full.t == 8 and len(losses[0]) == len(losses[1]) == 8
    # keyframes sampled in turn (slam/mapper.py:152-156 samples at random): every keyframe keeps its own order
    cam2 = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(3)[2], data_device=str(device))
    for it in range(6):
        c = cam if it % 2 == 0 else cam2
        losses[0].append(full.step(c)["loss"])
        losses[1].append(rep.step(c)["loss"])
    assert rep.stats["repeated_resort"] == 1, "orders two iterations old are still repairable"
    assert len(rep._orders) == 2
    for a, b in zip(*losses):
        assert abs(a - b) <= 1e-5 * abs(a), losses
    # (float atomics order the gradient sums differently from run to run and Adam amplifies that where
    # a gradient is ~0: compare against the distance travelled, as the engine-vs-torch test does)
    for k in ("_xyz", "_scaling", "_rotation", "_opacity"):
        pa, pb = getattr(models[0], k).detach(), getattr(models[1], k).detach()
        moved = float((pa - init[k]).abs().max())
        assert moved > 0 and float((pa - pb).abs().max()) <= 0.02 * moved, k
        if deterministic:
            assert torch.equal(pa, pb), f"deterministic accumulation: repaired and from-scratch trajectories differ in {k}"


def test_mapping_engine_remap_after_prune_and_densify(device):
    """Between keyframes the reference prunes and densifies (scene/gaussian_model.py:223-316): the engine carries
    the Adam moments of the surviving surfels over, starts the new ones at zero and keeps counting steps —
    checked against torch.optim.Adam over the torch pipeline going through the same surgery."""
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig, optimize_step
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 6000, 32, 256
    sc = synth.make_scene(N, H, W, seed=41, range_lo=2.0, range_hi=15.0)
    extra = synth.make_scene(500, H, W, seed=42, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, None, data_device=str(device))
    cfg = MappingConfig()
    a = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
    b = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
    eng = MappingEngine(a, cfg)
    b.training_setup(fused=False)                       # torch.optim.Adam, one group per tensor
    for _ in range(3):
        eng.step(cam)
        optimize_step(b, cam, cfg)
    keep = torch.rand(N, generator=torch.Generator().manual_seed(1)) > 0.3
    new = SurfelModel.from_activated(extra["means"], extra["scales"], extra["rots"], extra["opac"], device=str(device))

    def surgery(m, opt):
        for name in ("_xyz", "_scaling", "_rotation", "_opacity"):
            old = getattr(m, name)
            p = torch.nn.Parameter(torch.cat([old.detach()[keep.to(device)], getattr(new, name).detach()]).contiguous())
            if opt is not None:                         # what cat_tensors_to_optimizer / _prune_optimizer do
                grp = next(g for g in opt.param_groups if g["params"][0] is old)
                st = opt.state.pop(old)
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = torch.cat([st[k][keep.to(device)], torch.zeros_like(getattr(new, name))])
                grp["params"][0] = p
                opt.state[p] = st
            setattr(m, name, p)

    moments_before = eng.exp_avg[:3 * N].view(N, 3)[keep.to(device)].clone()
    surgery(a, None)
    eng.remap(keep, appended=500, reset_state=False)
    surgery(b, b.optimizer)
    n2 = int(keep.sum()) + 500
    assert eng.N == n2 and torch.equal(eng.exp_avg[:3 * n2].view(n2, 3)[:n2 - 500], moments_before)
    assert float(eng.exp_avg[:3 * n2].view(n2, 3)[n2 - 500:].abs().max()) == 0.0
    start = a._xyz.detach().clone()
    for _ in range(3):
        st = eng.step(cam)
        optimize_step(b, cam, cfg)
    assert eng.t == 6 and np.isfinite(st["loss"])
    moved = float((a._xyz.detach() - start).abs().max())
    for name in ("_xyz", "_scaling", "_rotation", "_opacity"):
        diff = (getattr(a, name).detach() - getattr(b, name).detach()).abs()
        # Adam turns ANY non-zero gradient into a step of ~lr (eps = 1e-15): an element whose gradient is pure
        # rounding noise (1e-15 in one pipeline, exactly 0 in the other) may differ by a whole step, so a
        # handful of such elements is tolerated; everything else must agree to 5 % of the distance travelled
        off = diff > 0.05 * moved + 1e-6
        assert float(off.float().mean()) <= 3e-3 and float(diff.max()) <= 3.5 * 5e-2, (name, float(diff.max()))
    with pytest.raises(RuntimeError):
        eng.remap(None, appended=7)                     # the model was not resized accordingly
    # the reference's own behaviour (scene/gaussian_model.py:237-256 drops the state on every prune): Adam restarts
    eng.remap(None, appended=0)
    assert eng.t == 0 and float(eng.exp_avg.abs().max()) == 0.0 and float(eng.exp_avg_sq.abs().max()) == 0.0
    before = a._xyz.detach().clone()
    eng.step(cam)
    step = (a._xyz.detach() - before).abs()
    assert eng.t == 1 and float(step.max()) <= 5e-4 * 1.001     # first Adam step: |update| = lr wherever g != 0


@pytest.mark.parametrize("N,H,W", [(1, 16, 64), (2, 16, 64), (3, 16, 64), (100, 16, 64), (500, 48, 80), (1000, 128, 1024),
                                   (50_000, 16, 16), (4096, 64, 8192), (300_000, 128, 4096)])
def test_engine_edge_sizes(device, N, H, W):
    """Whole iterations at the corners of the size space: fewer surfels than a wave / a sort chunk / an Adam
    vector, a single tile, tile counts that are not a multiple of the XCD interleave, 2048 tiles (two-pass tile
    sort), a capacity that has to grow; lagged status read throughout."""
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    sc = synth.make_scene(N, H, W, seed=N % 97)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, None, data_device=str(device))
    model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
    eng = MappingEngine(model, MappingConfig())
    losses = []
    for it in range(6):
        st = eng.step(cam, sync="lagged")
        if st is not None:
            losses.append(st["loss"])
    losses.append(eng.flush()["loss"])
    assert len(losses) == 6 and eng.t == 6 and all(np.isfinite(losses))
    for p in (model._xyz, model._scaling, model._rotation, model._opacity):
        assert bool(torch.isfinite(p).all())
    assert eng.stats["repeated_resort"] == 0


def test_depth_order_repair_rounds(device):
    """A surfel that has to travel more than half a window (512 positions) defeats one repair round — the
    iteration is voided and repeated — but not two; the engine switches to two rounds after such a failure."""
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    N, H, W = 30000, 32, 512
    sc = synth.make_scene(N, H, W, seed=16, range_lo=2.0, range_hi=25.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, None, data_device=str(device))
    # a radial perturbation that moves the worst surfel 600..1400 positions in the depth order
    rng = np.random.default_rng(3)
    r0 = np.linalg.norm(sc["means"], axis=1)
    noise = rng.uniform(-1.0, 1.0, N)
    rank0 = np.argsort(np.argsort(r0, kind="stable"), kind="stable")
    amp = None
    for a in np.geomspace(1e-4, 0.2, 60):
        disp = np.abs(np.argsort(np.argsort(r0 * (1 + a * noise), kind="stable"), kind="stable") - rank0).max()
        if 600 <= disp <= 1400:
            amp = a
            break
    assert amp is not None
    f = torch.tensor(1 + amp * noise, dtype=torch.float32, device=device)[:, None]
    engines = []
    for rounds in (0, 1, 2, 3, 4):      # (3, 4: the further rounds' pairs ping-pong between two buffers)
        m = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
        e = MappingEngine(m, MappingConfig())
        e.reuse_depth_order = rounds > 0
        # (deterministic accumulation: the engines walk the same trajectory to the bit — with float atomics their
        #  parameters differ in the last bits after an update, and two surfels of nearly equal range may swap places)
        e.deterministic = True
        e._repair_rounds, e._repair_until = max(rounds, 1), 10 ** 9
        engines.append((e, m))
    losses = []
    for e, m in engines:
        ls = [e.step(cam)["loss"], e.step(cam)["loss"]]
        with torch.no_grad():
            m._xyz.mul_(f)
        ls += [e.step(cam)["loss"], e.step(cam)["loss"]]
        losses.append(ls)
    assert engines[0][0].stats["repeated_resort"] == 0
    assert engines[1][0].stats["repeated_resort"] == 1, "one round cannot reach: void + repeat with the full sort"
    assert engines[1][0]._repair_rounds == 2, "and the engine repairs with two rounds from then on"
    for k in (2, 3, 4):
        assert engines[k][0].stats["repeated_resort"] == 0, "two (and more) rounds reach"
    for ls in losses[1:]:
        for a, b in zip(losses[0], ls):
            assert abs(a - b) <= 1e-5 * abs(a), losses
    o0 = engines[0][0]._orders[id(cam)].order.cpu().numpy()
    for e, _ in engines[1:]:          # the exact (key, index) order, bit for bit
        assert np.array_equal(e._orders[id(cam)].order.cpu().numpy(), o0)


def test_depth_order_repair_at_awkward_sizes(device):
    """tools/repair_fuzz.py: below one window, at window edges, odd counts — one to four repair rounds (the further
    ones in one launch each, their pairs ping-ponging between two buffers), the loss stage inside the tile backward and
    apart: under deterministic accumulation every configuration walks the SAME trajectory, orders and parameters bit
    for bit."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location(
        "repair_fuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "repair_fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(dev=str(device), verbose=False) == 0


@pytest.mark.parametrize("walk", [True, False], ids=["walk", "cull"])
@pytest.mark.parametrize("list_pairs", [1, 2], ids=["pairs", "plain"])
def test_tile_kernel_paths_agree_with_checker(device, oracle32, list_pairs, walk):
    """The tile backward's paths pass the same parity bar: the dense rounds on the forward's compact lists (walk) and
    the culling rounds over the tile's list (cull: the state names no hand-over), each on the tile sort's (surfel,
    block mask) pairs (vals_stride 2) and on plain lists (vals_stride 1)."""
    from splat_loam_amd import _abi
    lib = _abi.lib()
    # the 8x2 pixel blocks are the only tile kernels: sls_debug_variant keeps its ABI slot and accepts nothing else
    assert lib.sls_debug_variant(2, 2) != 0
    assert lib.sls_debug_variant(3, 3) == 0 and lib.sls_debug_variant(-1, -1) == 0
    N, H, W = 20000, 64, 512
    sc, view, proj = scene_and_camera(N, H, W, seed=21, range_lo=2.0, range_hi=30.0)
    st, t = hip_forward(device, sc, view, proj, H, W, list_pairs=list_pairs)
    assert st.vals_stride == (2 if list_pairs == 1 else 1) and st.block_masks_shape == 3
    cam = oracle32.camera(H, W, view, proj, tile=_abi.tile_size())
    ost = oracle32.forward(cam, sc["means"], sc["scales"], sc["rots"], sc["opac"])
    _compare_forward(oracle32, st, ost, cam, f"list_pairs{list_pairs}")
    if not walk:
        st.block_masks_shape = 0
    _compare_backward(oracle32, st, t, ost, sc, f"list_pairs{list_pairs}-{'walk' if walk else 'cull'}")


def _engine_rank(rank, world, port, out_dir, mode="sync", dp_mode="rs_ag"):
    import os
    import torch.distributed as dist
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)     # both ranks share cuda:0 in this test
    N, H, W = 5000, 32, 256
    sc = synth.make_scene(N, H, W, seed=31, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[rank], data_device="cuda:0")
    model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
    eng = MappingEngine(model, MappingConfig())
    eng.dp_mode = dp_mode
    if rank == 1:
        eng.capacity = 1024           # one rank overflows: BOTH must skip Adam and repeat
    if mode == "lagged":
        # the status of iteration k is read after k+1 was enqueued; the verdict of the GROUP guards Adam on
        # the device, so both ranks void / repeat the same iterations without an extra collective
        seen = [eng.step(cam, sync="lagged") for _ in range(4)]
        assert seen[0] is None
        st = eng.flush()
        assert eng.stats["repeated_too_small"] >= 1 and not st["overflow"]
        ref = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
        eng2 = MappingEngine(ref, MappingConfig())
        for _ in range(4):
            eng2.step(cam)
        moved = (ref._xyz.detach() - torch.tensor(sc["means"], device="cuda:0")).abs().max().item()
        assert moved > 0
        assert (ref._xyz.detach() - model._xyz.detach()).abs().max().item() <= 0.02 * moved
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), xyz=model._xyz.detach().cpu().numpy(),
                 rot=model._rotation.detach().cpu().numpy(), sc=model._scaling.detach().cpu().numpy(),
                 op=model._opacity.detach().cpu().numpy(), t=eng.t)
        dist.destroy_process_group()
        return

    def reduced():
        # the summed gradient as this rank holds it: the whole bucket (all-reduce), its own chunk (reduce-scatter) or
        # the union's rows scattered back into the flat layout (sparse)
        if eng._sx is not None:
            sx, n = eng._sx, eng.N
            bits = np.unpackbits(sx["bitmap"][:-2].cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
            rows = np.zeros((n, 10), np.float32)
            k = int(bits.sum())
            rows[bits] = sx["compact"][:10 * k].cpu().numpy().reshape(k, 10)
            return np.concatenate([rows[:, 0:3].reshape(-1), rows[:, 3], rows[:, 4:6].reshape(-1), rows[:, 6:10].reshape(-1)]), 0
        if eng._dp is None:
            return eng.grads[:-2].cpu().numpy(), 0
        d = eng._dp
        return d["gshard"][:d["hi"] - d["lo"]].cpu().numpy(), d["lo"]
    st = eng.step(cam)
    g1, lo = reduced()
    st = eng.step(cam)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), xyz=model._xyz.detach().cpu().numpy(),
             rot=model._rotation.detach().cpu().numpy(), sc=model._scaling.detach().cpu().numpy(),
             op=model._opacity.detach().cpu().numpy(), g1=g1, lo=lo, R=st["R"], t=eng.t,
             sharded_state=int(eng._dp is not None), state_len=int(eng.exp_avg.numel()),
             rows=st["exchange_count"], xbytes=eng.exchanged_bytes)
    dist.destroy_process_group()


def test_engine_keyframe_parallel_lagged_two_ranks(device, tmp_path):
    """Keyframe-parallel engine, lagged status read (2 ranks, gloo, one GPU): an overflow on one rank voids
    the iteration on both, both repeat it, replicas stay bit-identical and agree with the synchronous mode."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_engine_rank, args=(2, port, str(tmp_path), "lagged"), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "r1.npz")
    assert int(r0["t"]) == int(r1["t"]) == 4
    for k in ("xyz", "rot", "sc", "op"):
        assert np.array_equal(r0[k], r1[k]), f"replicas diverged: {k}"


@pytest.mark.parametrize("dp_mode", ["rs_ag", "allreduce", "sparse"])
def test_engine_keyframe_parallel_two_ranks(device, tmp_path, dp_mode):
    """Keyframe-parallel engine with 2 ranks (gloo, one GPU), both exchange schemes (reduce-scatter -> Adam on the
    rank's half -> all-gather of the parameters / one all-reduce -> Adam everywhere): the reduced gradient equals
    the sum of the two keyframes' gradients (regulariser once), replicas stay bit-identical, an overflow on
    one rank makes every rank repeat the iteration."""
    import socket
    import torch.multiprocessing as mp
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_engine_rank, args=(2, port, str(tmp_path), "sync", dp_mode), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "r1.npz")
    assert int(r0["t"]) == int(r1["t"]) == 2
    for k in ("xyz", "rot", "sc", "op"):
        assert np.array_equal(r0[k], r1[k]), f"replicas diverged: {k}"
    if dp_mode == "rs_ag":
        assert int(r0["sharded_state"]) == 1 and int(r0["state_len"]) < 10 * 5000, "optimiser state is sharded"
        assert int(r0["lo"]) == 0 and int(r1["lo"]) == len(r0["g1"])
        reduced = np.concatenate([r0["g1"], r1["g1"]])
    elif dp_mode == "sparse":
        # the reduced rows of the union, scattered back to the flat bucket layout by the worker
        # (the two keyframes reach nearly every surfel of this small scene: the volume saving shows on real sizes,
        #  bench.py --gpus 2 --dp-mode sparse: 2.7 MB instead of 20 MB per rank at 500k surfels)
        assert np.array_equal(r0["g1"], r1["g1"]) and 0 < int(r0["rows"]) <= 5000
        assert int(r0["xbytes"]) <= 40 * 5000 + 8 * (5000 // 64 + 3)
        reduced = r0["g1"]
    else:
        assert np.array_equal(r0["g1"], r1["g1"])
        reduced = r0["g1"]
    N, H, W = 5000, 32, 256
    sc = synth.make_scene(N, H, W, seed=31, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    total = 0.0
    for rank in range(2):
        cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[rank], data_device=str(device))
        model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
        eng = MappingEngine(model, MappingConfig())
        eng._enqueue(cam, apply_adam=False, with_regulariser=(rank == 0))
        torch.cuda.synchronize()
        total = total + eng.grads[:-2].cpu().numpy().astype(np.float64)
    scale = np.abs(total).max()
    assert np.abs(reduced - total).max() <= 1e-5 * scale


def test_engine_sparse_exchange_equals_the_all_reduce_two_ranks(device, tmp_path, monkeypatch):
    """VERDICT r05 item 4.  The touched-set exchange as the engine runs it since round 6 — early bitmaps all-gathered and
    OR-ed behind the tile backward, the projection's backward writing the union's rows straight into the collective's
    buffer and applying Adam to every surfel outside the union, one SUM of the rows, Adam on the union — against the
    dense all-reduce: two ranks (gloo, one GPU), lagged status read, one rank overflowing its instance buffers so that
    an iteration is voided and repeated on both.  With deterministic accumulation the parameters after four iterations
    are the all-reduce path's to the bit, on both ranks."""
    import socket
    import torch.multiprocessing as mp
    monkeypatch.setenv("SLS_DETERMINISTIC", "1")
    out = {}
    for tag in ("allreduce", "sparse"):
        d = tmp_path / tag
        d.mkdir()
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        mp.spawn(_engine_rank, args=(2, port, str(d), "lagged", tag), nprocs=2, join=True)
        out[tag] = [np.load(d / "r0.npz"), np.load(d / "r1.npz")]
    for tag, (r0, r1) in out.items():
        assert int(r0["t"]) == int(r1["t"]) == 4
        for k in ("xyz", "rot", "sc", "op"):
            assert np.array_equal(r0[k], r1[k]), f"{tag}: replicas diverged: {k}"
    for k in ("xyz", "rot", "sc", "op"):
        assert np.array_equal(out["allreduce"][0][k], out["sparse"][0][k]), f"the touched-set exchange changed the parameters: {k}"


def _engine_rccl_rank(rank, port, out_dir, dp_mode):
    import os
    import torch.distributed as dist
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))   # "nccl" IS RCCL on ROCm
    N, H, W = 5000, 32, 256
    sc = synth.make_scene(N, H, W, seed=31, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[0], data_device="cuda:0")

    def run(exchange, lagged):
        model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
        eng = MappingEngine(model, MappingConfig())
        eng.dp_mode = dp_mode
        eng.exchange_at_world_1 = exchange
        eng.deterministic = True           # integer-atomic accumulation: both paths must then agree to the bit
        losses = []
        if lagged:
            sts = [eng.step(cam, sync="lagged") for _ in range(4)]
            eng.flush()
            losses = [s["loss"] for s in sts[1:]] + [s["loss"] for s in eng.flushed]
        else:
            losses = [eng.step(cam)["loss"] for _ in range(4)]
        return model, eng, losses
    ref, _, l_ref = run(False, False)
    got, eng, l_got = run(True, False)
    lag, eng_l, l_lag = run(True, True)
    np.savez(os.path.join(out_dir, "rccl.npz"),
             **{f"ref_{k}": getattr(ref, k).detach().cpu().numpy() for k in ("_xyz", "_rotation", "_scaling", "_opacity")},
             **{f"got_{k}": getattr(got, k).detach().cpu().numpy() for k in ("_xyz", "_rotation", "_scaling", "_opacity")},
             **{f"lag_{k}": getattr(lag, k).detach().cpu().numpy() for k in ("_xyz", "_rotation", "_scaling", "_opacity")},
             l_ref=np.array(l_ref), l_got=np.array(l_got), l_lag=np.array(l_lag), sharded=int(eng._dp is not None),
             in_place=int(eng._dp.get("ag_in_place", True)) if eng._dp else -1, t=eng.t, backend=dist.get_backend())
    dist.destroy_process_group()


def _det2_misprediction_rank(rank, port, out_dir):
    import os
    import torch.distributed as dist
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    N, H, W = 5000, 32, 256
    sc = synth.make_scene(N, H, W, seed=31, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[0], data_device="cuda:0")
    out = {}
    for tag, exchange, dp_mode, sync in (("single", False, "allreduce", True), ("single_lagged", False, "allreduce", "lagged"),
                                         ("allreduce", True, "allreduce", True), ("sparse", True, "sparse", True),
                                         ("rs_ag_lagged", True, "rs_ag", "lagged")):
        model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
        eng = MappingEngine(model, MappingConfig())
        eng.dp_mode, eng.exchange_at_world_1, eng.deterministic = dp_mode, exchange, 2
        for _ in range(3):
            eng.step(cam)
        before = sum(eng.stats.values())
        eng._orders[id(cam)].det_prev.fill_(1)       # predictions 2^100 too small: every field of every surfel overflows its scale
        if sync == "lagged":
            eng.step(cam, sync="lagged"); eng.step(cam, sync="lagged"); eng.flush()
        else:
            eng.step(cam); eng.step(cam)
        out[tag + "_repeats"] = sum(eng.stats.values()) - before
        out[tag + "_t"] = eng.t
        out[tag + "_xyz"] = model._xyz.detach().cpu().numpy()
    np.savez(os.path.join(out_dir, "det2.npz"), **out)
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_one_launch_deterministic_mode_survives_a_misprediction(device, tmp_path):
    """ADVICE r04 (medium).  SLS_DETERMINISTIC=2 predicts every field's fixed-point scale from the keyframe's previous
    iteration; a misprediction voids the iteration (bit 3).  The keyframe-parallel verdicts fold that bit into bit 1, so
    the host could not tell it from a failed repair and repeated the iteration in ONE launch again — same parameters,
    same predictions, same misprediction: step() never returned.  Now the repeat of any voided deterministic iteration
    takes two launches.  Forced here by overwriting the predictions, on one GPU and through the three exchange
    schemes in a one-rank RCCL group, synchronous and lagged: five iterations each, one of them repeated, and the
    same parameters whichever way the gradients travelled."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_det2_misprediction_rank, args=(port, str(tmp_path)), nprocs=1, join=True)
    r = np.load(tmp_path / "det2.npz")
    for tag in ("single", "single_lagged", "allreduce", "sparse", "rs_ag_lagged"):
        assert int(r[tag + "_t"]) == 5, tag
        assert int(r[tag + "_repeats"]) >= 1, f"{tag}: the poisoned predictions did not void an iteration"
        assert np.isfinite(r[tag + "_xyz"]).all()
        assert np.abs(r[tag + "_xyz"] - r["single_xyz"]).max() <= 1e-6 * np.abs(r["single_xyz"]).max(), tag


@pytest.mark.parametrize("dp_mode", ["rs_ag", "allreduce", "sparse"])
def test_engine_exchange_through_rccl_world_1(device, tmp_path, dp_mode, monkeypatch):
    """The keyframe-parallel exchange executed by RCCL itself (backend "nccl", one rank, one GPU): reduce_scatter_tensor
    -> Adam on the shard -> all_gather_into_tensor in place (rs_ag), or all_reduce -> Adam (allreduce).  With one
    rank the collectives are identities, so — with deterministic accumulation — the parameters after 4 iterations
    must equal the single-GPU path's (fused Adam inside the backward) to the bit, in the synchronous and in the
    lagged mode."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_engine_rccl_rank, args=(port, str(tmp_path), dp_mode), nprocs=1, join=True)
    r = np.load(tmp_path / "rccl.npz")
    assert str(r["backend"]) == "nccl" and int(r["t"]) == 4
    assert int(r["sharded"]) == (1 if dp_mode == "rs_ag" else 0)
    assert np.allclose(r["l_ref"], r["l_got"], rtol=1e-6) and np.allclose(r["l_ref"], r["l_lag"], rtol=1e-6)
    for k in ("_xyz", "_rotation", "_scaling", "_opacity"):
        assert np.array_equal(r["ref_" + k], r["got_" + k]), f"RCCL path differs from the single-GPU path: {k}"
        assert np.array_equal(r["ref_" + k], r["lag_" + k]), f"RCCL path (lagged) differs: {k}"
