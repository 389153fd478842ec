"""From a saved map to the oriented point cloud Poisson reconstruction eats: steps 1-4 of the reference's
`mesh_poisson` (scene/postprocessing.py:93-190) — for every keyframe of the results graph render the model it belongs
to, filter by `rend_alpha` / `rend_dist`, back-project, sample `kf_samples` pixels, move them to the world frame and
merge.  The Poisson solve itself (Open3D, on the CPU) is not part of this tree: `ply_io.save_point_cloud` writes the
cloud in the form Open3D's `read_point_cloud` loads.

Per keyframe, after the rasterizer forward, everything is ONE native call of two launches (sls_surface_samples,
csrc/sls_surface.hip): no boolean gather, no copy to the host, no host read — the keyframes' status words live in one
device array that is read once at the end.  The reference draws with an unseeded `np.random.choice`; here the sample is
a pure function of (allmap, thresholds, seed, frame id, kf_samples): DESIGN.md section 2, "Surface samples".

`mesh_tsdf` makes a mesh here, without the Poisson solve: the same keyframes fused into a sparse TSDF volume around the
sampled cloud and the zero surface extracted by marching tetrahedra (splat_loam_amd/tsdf.py; DESIGN.md section 2, "TSDF
volume").

`mesh_poisson` itself could not be run where this was written (Open3D is not installed there), so the sampling
semantics are restated from reading postprocessing.py:161-188, not pinned by a reference-generated fixture; what it
shares with `render()` (the maps, the back-projection) is pinned by goldens G1 / G2.
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import torch

from . import _abi

_SURFACE_BUFFERS = {}                   # (device, H, W) -> scratch (the validity words)


def frames_to_sample(graph: dict, kf_interval: int = -1) -> list:
    """[(index of the model in graph["models"], frame id)] of the keyframes `mesh_poisson` processes
    (postprocessing.py:126-140): one counter of processed frames runs across all models, starts at 1 with the first
    frame, and a frame is skipped when `kf_interval > 0 and counter % kf_interval != 0`."""
    used, processed = [], 0
    for mi, rmodel in enumerate(graph["models"]):
        for fid in rmodel["frame_ids"]:
            processed += 1
            if kf_interval is not None and kf_interval > 0 and processed % kf_interval:
                continue
            used.append((mi, int(fid)))
    return used


def _pose44(v) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64)
    if a.size == 16:
        return a.reshape(4, 4).copy()
    return np.vstack([a.reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def compose_cam_to_world(world_T_model, view32) -> np.ndarray:
    """M = world_T_model inv(world_view_transform^T) as 12 float32 (3x4 row-major): composed in float64 from the float32
    view matrix the rasterizer renders with (`view32` = world_view_transform^T, i.e. inv(model_T_frame) rounded), rounded
    once."""
    c2w = np.linalg.inv(np.asarray(view32, dtype=np.float32).astype(np.float64).reshape(4, 4))
    return np.ascontiguousarray((_pose44(world_T_model) @ c2w)[:3].reshape(12), dtype=np.float32)


def _host(world_T_model):
    return world_T_model.detach().cpu().numpy() if isinstance(world_T_model, torch.Tensor) else world_T_model


@torch.no_grad()
def sample_keyframe(allmap: torch.Tensor, camera, world_T_model, *, kf_samples: int = 5000, min_opacity: float = 0.5,
                    max_depth_dist: float = 0.1, use_median_depth: bool = False, seed: int = 0, frame_id: int = 0, out=None,
                    details: bool = False, cam_to_world: torch.Tensor = None):
    """`kf_samples` oriented world-frame points of one rendered keyframe through sls_surface_samples.

    allmap: the rasterizer forward's raw (7,H,W) device tensor, the FULL one (`lean_allmap=False`: plane 6 is read);
    camera: the `scene.Camera` it was rendered with; world_T_model: 4x4 (or 3x4 / 12 floats) on the host.
    out: None, or (points (k,3) f32, normals (k,3) f32, pixels (k,) i32 or None, status (4,) i32) — contiguous device
        tensors, e.g. slices of a run's slabs, that the call fills.  With `out` NOTHING is read back: the tuple is
        returned as it is and the caller reads status = [n_valid, rows written (k, or 0 for a keyframe without a valid
        pixel, whose rows stay untouched), 0, 1] when it wants to.
        Without `out` the status is read once: returns (points, normals), empty (0,3) where no pixel is valid;
        `details=True` adds dict(n_valid, pixels (the selected row-major pixels, int32), status).
    cam_to_world (extension): the composed M = world_T_model inv(world_view_transform^T) as a (12,) float32 device tensor
        when the caller holds it already (`sample_surface` uploads every keyframe's in one copy); world_T_model is not
        read then.
    Device tensors only; there is no CPU fall-back."""
    from .rasterizer import GaussianRasterizationSettings, _stream, get_camera, half_pixel_tables
    if not isinstance(allmap, torch.Tensor) or not allmap.is_cuda:
        raise RuntimeError("sample_keyframe needs the allmap on a ROCm device; there is no CPU fallback")
    if allmap.dim() != 3 or allmap.shape[0] != 7:
        raise ValueError("allmap must be (7, H, W)")
    if int(kf_samples) < 1:
        raise ValueError("kf_samples must be at least 1")
    dev = allmap.device
    am = allmap.detach()
    if am.dtype != torch.float32 or not am.is_contiguous():
        am = am.float().contiguous()
    _, H, W = am.shape
    k = int(kf_samples)
    lib = _abi.lib()
    ce = get_camera(GaussianRasterizationSettings(H, W, 1.0, camera.world_view_transform, camera.projection_matrix), dev)
    col_h, row_h = half_pixel_tables(ce, dev)
    if cam_to_world is None:
        view = np.eye(4, dtype=np.float32)            # world_view_transform^T from the camera entry's host copy: no device read
        view[:3, :3] = np.asarray(ce.cam.Rvw, dtype=np.float32).reshape(3, 3)
        view[:3, 3] = np.asarray(ce.cam.tvw, dtype=np.float32)
        cam_to_world = torch.from_numpy(compose_cam_to_world(_host(world_T_model), view)).to(dev)
    elif (not cam_to_world.is_cuda or cam_to_world.dtype != torch.float32 or cam_to_world.numel() != 12
          or not cam_to_world.is_contiguous()):
        raise ValueError("cam_to_world must be a contiguous (12,) float32 device tensor")
    key = (str(dev), H, W)
    scratch = _SURFACE_BUFFERS.get(key)
    if scratch is None:
        need = int(lib.sls_surface_scratch_bytes(H, W))
        scratch = _SURFACE_BUFFERS[key] = torch.empty((max(need, 8) + 7) // 8, dtype=torch.int64, device=dev)
    own = out is None
    if own:
        points = torch.empty((k, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((k, 3), dtype=torch.float32, device=dev)
        pixels = torch.empty((k,), dtype=torch.int32, device=dev) if details else None
        status = torch.empty((4,), dtype=torch.int32, device=dev)
    else:
        points, normals, pixels, status = out
        for name, t, shape, dt in (("points", points, (k, 3), torch.float32), ("normals", normals, (k, 3), torch.float32),
                                   ("pixels", pixels, (k,), torch.int32), ("status", status, (4,), torch.int32)):
            if t is None and name == "pixels":
                continue
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape
                    and t.is_contiguous()):
                raise ValueError(f"out: {name} must be a contiguous {shape} {dt} tensor on {dev}")
    _abi.check(lib.sls_surface_samples(H, W, am.data_ptr(), col_h.data_ptr(), row_h.data_ptr(), cam_to_world.data_ptr(),
                                       float(min_opacity), float(max_depth_dist), 1.0 if use_median_depth else 0.0, k,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame_id) & 0xFFFFFFFF, points.data_ptr(),
                                       normals.data_ptr(), None if pixels is None else pixels.data_ptr(), status.data_ptr(),
                                       scratch.data_ptr(), int(scratch.numel()) * 8, _stream(dev)), "sls_surface_samples")
    if not own:
        return out
    words = status.cpu().numpy().view(np.uint32).copy()         # the one host read of a stand-alone call
    rows = int(words[1])
    if details:
        return points[:rows], normals[:rows], {"n_valid": int(words[0]), "pixels": pixels[:rows], "status": words}
    return points[:rows], normals[:rows]


def _image_size(graph_dir: Path, image_height, image_width):
    cfg_file = graph_dir / "cfg.yaml"
    if cfg_file.exists():
        import yaml
        pre = (yaml.safe_load(open(cfg_file)) or {}).get("preprocessing") or {}
        if "image_height" in pre and "image_width" in pre:
            return int(pre["image_height"]), int(pre["image_width"])
    if image_height is None or image_width is None:
        raise ValueError(f"the image size is neither in {cfg_file} (preprocessing.image_height / image_width) nor given "
                         "as image_height= / image_width=")
    return int(image_height), int(image_width)


def _render_keyframes(graph_dir: Path, graph: dict, used: list, poses: list, H: int, W: int, dev):
    """Yields (i, frame id, camera, the full (7,H,W) allmap) for the keyframes `used` ([(model index, frame id)], as
    `frames_to_sample` lists them) with `poses[i]` their model_T_frame: renders each with the model it belongs to."""
    from . import ply_io
    from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from .scene import Camera, SurfelModel
    frames = {int(fr["id"]): fr for fr in graph["frames"]}
    zeros = {"d": torch.zeros((1, H, W), dtype=torch.float32, device=dev), "n": torch.zeros((3, H, W), dtype=torch.float32, device=dev),
             "v": torch.zeros((1, H, W), dtype=torch.uint8, device=dev)}
    loaded = (None, None)
    for i, (mi, fid) in enumerate(used):
        if loaded[0] != mi:                             # the frames of a model are consecutive: one load per model
            raw = ply_io.load_ply(graph_dir / graph["models"][mi]["filename"])
            gm = SurfelModel(*(np.array(raw[n]) for n in ("xyz", "scaling", "rotation", "opacity")), device=dev)   # (writable copies)
            loaded = (mi, (gm.get_xyz.detach(), gm.get_opacity.detach(), gm.get_scaling.detach(), gm.get_rotation.detach()))
        xyz, opac, scal, rot = loaded[1]
        fr = frames[fid]
        if int(fr["model_id"]) != int(graph["models"][mi]["id"]):
            raise ValueError(f"frame {fid} is listed by model {graph['models'][mi]['id']} but belongs to model {fr['model_id']}")
        fx, fy, cx, cy = (float(v) for v in fr["projmatrix"])
        cam = Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32), zeros["d"], zeros["n"], zeros["v"],
                     world_T_lidar=poses[i], data_device=dev)
        settings = GaussianRasterizationSettings(H, W, 1.0, cam.world_view_transform, cam.projection_matrix, lean_allmap=False)
        _, allmap = GaussianRasterizer(raster_settings=settings)(means3D=xyz, means2D=xyz, opacities=opac, scales=scal,
                                                                 rotations=rot)
        yield i, fid, cam, allmap


def _check_outlier(outlier_nb, outlier_std):
    """None, or (nb_neighbors, std_ratio) checked as evaluation.remove_statistical_outlier checks them — before any work."""
    if outlier_nb is None:
        return None
    from . import evaluation
    return evaluation._check_stat_args(outlier_nb, outlier_std)


def _check_cluster(cluster_eps, cluster_min_points, cluster_keep, cluster_min_size):
    """None, or (eps, min_points, keep, min_cluster_points) checked as evaluation.keep_clusters checks them — before any work."""
    if cluster_eps is None:
        return None
    from . import evaluation
    return evaluation._check_cluster_args(cluster_eps, cluster_min_points) + evaluation._check_select_args(cluster_keep, cluster_min_size)


def _resolve_device(caller: str, device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{caller} runs on a ROCm device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def sample_surface(graph_dir_or_yaml, *, kf_interval: int = -1, kf_samples: int = 5000, min_opacity: float = 0.5,
                   max_depth_dist: float = 0.1, use_median_depth: bool = False, seed=None, device="cuda",
                   details: bool = False, image_height=None, image_width=None, outlier_nb=None, outlier_std: float = 2.0,
                   cluster_eps=None, cluster_min_points: int = 10, cluster_keep: int = 1, cluster_min_size: int = 0):
    """`mesh_poisson`'s steps 1-4 (postprocessing.py:122-190) over a results directory (`graph.yaml`, `models/*.ply`,
    optionally `cfg.yaml` for the image size): returns (points (M,3), normals (M,3)), float32 device tensors in keyframe
    order, `kf_samples` rows per keyframe that has a valid pixel (the reference raises on one that has none; here it
    contributes no rows).  `details=True` adds dict(frame_ids: the frames used, n_valid: their counts of valid pixels,
    pixels: (frames used, kf_samples) int32, the selected row-major pixels, -1 in the rows of an empty keyframe, kept:
    which of the frames used contributed rows).  seed=None: torch.initial_seed().  Sample j of frame f depends on
    (seed, f, j) and the render alone — not on kf_interval or the order of processing.

    `outlier_nb=k` filters the merged cloud with `evaluation.remove_statistical_outlier(k, outlier_std)`: what the
    reference's `remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0)` (postprocessing.py:192) meant to do, at its
    place in the sequence — the reference discards that call's result.  One more host read; the rows keep their order
    and `details` gains `outlier` (the filter's statistics and `index`, the surviving rows of the unfiltered cloud).
    The default None leaves the cloud as it always was, to the bit.

    `cluster_eps=e` then keeps the large pieces of the cloud, after the outlier stage:
    `evaluation.keep_clusters(e, cluster_min_points, cluster_keep, cluster_min_size)` — DBSCAN over exact radius
    neighbours, the `cluster_keep` largest clusters and those of at least `cluster_min_size` points kept — which removes
    what the outlier filters cannot, a floater whose points have each other for neighbours.  One more host read; `details`
    gains `cluster` (its statistics and `index`, the surviving rows of the cloud that entered the stage).  Default None: off,
    and the cloud is what it was, to the bit."""
    points, normals, det, _ = _sample_surface(graph_dir_or_yaml, device, details, kf_interval=kf_interval, kf_samples=kf_samples,
                                              min_opacity=min_opacity, max_depth_dist=max_depth_dist, use_median_depth=use_median_depth,
                                              seed=seed, image_height=image_height, image_width=image_width, outlier_nb=outlier_nb,
                                              outlier_std=outlier_std, cluster_eps=cluster_eps, cluster_min_points=cluster_min_points,
                                              cluster_keep=cluster_keep, cluster_min_size=cluster_min_size)
    return (points, normals, det) if details else (points, normals)


@torch.no_grad()
def _sample_surface(graph_dir_or_yaml, device, details, *, kf_interval, kf_samples, min_opacity, max_depth_dist, use_median_depth, seed,
                    image_height, image_width, outlier_nb, outlier_std, cluster_eps, cluster_min_points, cluster_keep, cluster_min_size):
    """The work of `sample_surface`, whose options these are: (points, normals, its `details` dict or None, context).  The
    context is what the pass read and derived, for a second pass over the same keyframes (`mesh_tsdf`): dict(graph_dir, graph:
    the parsed graph.yaml, size: (H, W), used: [(model index, frame id)], poses: their model_T_frame, kept: which of them
    contributed rows)."""
    from . import traj_io
    outlier = _check_outlier(outlier_nb, outlier_std)
    cluster = _check_cluster(cluster_eps, cluster_min_points, cluster_keep, cluster_min_size)
    path = Path(graph_dir_or_yaml)
    graph_file = path / "graph.yaml" if path.is_dir() else path
    graph_dir = graph_file.parent
    graph = traj_io.read_graph(graph_file)
    H, W = _image_size(graph_dir, image_height, image_width)
    dev = _resolve_device("sample_surface", device)
    used_seed = int(torch.initial_seed() if seed is None else seed)
    k = int(kf_samples)
    if k < 1:
        raise ValueError("kf_samples must be at least 1")
    used = frames_to_sample(graph, kf_interval)
    frames = {int(fr["id"]): fr for fr in graph["frames"]}
    F = len(used)
    points = torch.empty((F * k, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((F * k, 3), dtype=torch.float32, device=dev)
    pixels = torch.full((F, k), -1, dtype=torch.int32, device=dev) if details else None
    status = torch.zeros((max(F, 1), 4), dtype=torch.int32, device=dev)
    # every keyframe's view matrix (as scene.Camera rounds it) and composed M on the host, one upload of the latter
    poses = [_pose44(frames[fid]["model_T_frame"]) for _, fid in used]
    views = [np.linalg.inv(p).astype(np.float32) for p in poses]
    Ms = np.stack([compose_cam_to_world(graph["models"][mi]["world_T_model"], v) for (mi, _), v in zip(used, views)]) \
        if F else np.zeros((0, 12), np.float32)
    Ms_dev = torch.from_numpy(np.ascontiguousarray(Ms)).to(dev)
    for i, fid, cam, allmap in _render_keyframes(graph_dir, graph, used, poses, H, W, dev):
        sample_keyframe(allmap, cam, None, kf_samples=k, min_opacity=min_opacity, max_depth_dist=max_depth_dist,
                        use_median_depth=use_median_depth, seed=used_seed, frame_id=fid, cam_to_world=Ms_dev[i],
                        out=(points[i * k:(i + 1) * k], normals[i * k:(i + 1) * k], None if pixels is None else pixels[i],
                             status[i]))
    words = status.cpu().numpy().view(np.uint32)[:F]            # the run's one host read
    kept = words[:, 1] > 0
    if not kept.all():                                          # empty keyframes leave: one gather over whole blocks
        idx = torch.from_numpy(np.flatnonzero(kept)).to(dev)
        points = points.view(F, k, 3).index_select(0, idx).reshape(-1, 3)
        normals = normals.view(F, k, 3).index_select(0, idx).reshape(-1, 3)
    outlier_det = None
    if outlier is not None:
        from . import evaluation
        points, normals, index, outlier_det = evaluation.remove_statistical_outlier(points, outlier[0], outlier[1], normals=normals,
                                                                                    return_index=True, details=True)
        outlier_det["index"] = index
    cluster_det = None
    if cluster is not None:
        from . import evaluation
        points, normals, index, cluster_det = evaluation.keep_clusters(points, cluster[0], cluster[1], cluster[2], cluster[3],
                                                                       normals=normals, return_index=True, details=True)
        cluster_det["index"] = index
    det = None
    if details:
        det = {"frame_ids": [fid for _, fid in used], "n_valid": words[:, 0].astype(np.int64), "pixels": pixels,
               "kept": kept.copy(), "seed": used_seed}
        _add_stages(det, None, outlier_det, cluster_det)
    return points, normals, det, {"graph_dir": graph_dir, "graph": graph, "size": (H, W), "used": used, "poses": poses, "kept": kept}


# What `mesh_tsdf` and `mesh_poisson` take as **options, by the function an option goes to.  That function's signature is
# the one place that gives the option its default, and its docstring the one that describes it.
_SAMPLE_OPTIONS = ("kf_interval", "kf_samples", "min_opacity", "max_depth_dist", "use_median_depth", "seed", "image_height", "image_width",
                   "outlier_nb", "outlier_std", "cluster_eps", "cluster_min_points", "cluster_keep", "cluster_min_size")   # sample_surface
_CLEAN_OPTIONS = ("keep_clusters", "min_triangles", "normals", "simplify", "contraction", "regularisation", "smooth", "smooth_method",
                  "smooth_weights", "smooth_lambda", "smooth_mu", "fix_boundary", "fill_holes", "fill_max_size")         # mesh_ops.clean_mesh


def _route_options(caller: str, options: dict):
    """A front end's **options as (the keyword arguments of `_sample_surface`: `sample_surface`'s defaults under what the
    caller gave, the keyword arguments the caller gave for `clean_mesh`) — checked before any work: a name in neither tuple
    is a TypeError, then the outlier and the cluster arguments as `sample_surface` checks them."""
    for name in options:
        if name not in _SAMPLE_OPTIONS and name not in _CLEAN_OPTIONS:
            raise TypeError(f"{caller}() got an unexpected keyword argument '{name}'")
    defaults = sample_surface.__kwdefaults__                    # (of its keyword-only parameters, as its signature states them)
    sample = {k: options.get(k, defaults[k]) for k in _SAMPLE_OPTIONS}
    _check_outlier(sample["outlier_nb"], sample["outlier_std"])
    _check_cluster(sample["cluster_eps"], sample["cluster_min_points"], sample["cluster_keep"], sample["cluster_min_size"])
    return sample, {k: v for k, v in options.items() if k in _CLEAN_OPTIONS}


def _lap_timer(dev, on: bool):
    """(stage_ms, lap): with `on`, `lap(name)` synchronises and puts the milliseconds since the last lap under `name`."""
    import time
    stage_ms, t0 = {}, time.perf_counter()

    def lap(name):
        nonlocal t0
        if on:
            torch.cuda.synchronize(dev)
            stage_ms[name], t0 = (time.perf_counter() - t0) * 1e3, time.perf_counter()
    return stage_ms, lap


def _clean_stage(vertices, faces, clean: dict, lap):
    """(the mesh, the statistics of `mesh_ops.clean_mesh` or None) after a front end's extraction.  The stage runs only when
    one of `keep_clusters`, `normals`, `simplify`, `smooth`, `fill_holes` was given: with none of them the soup is returned as
    it always was.  Where it runs, a front end differs from `clean_mesh`'s own defaults on purpose: `keep_clusters=None`
    (every cluster stays) and `normals=False` (two tensors) unless the caller says otherwise.  One more host read."""
    if not clean.get("normals") and all(clean.get(k) is None for k in ("keep_clusters", "simplify", "smooth", "fill_holes")):
        return (vertices, faces), None
    from . import mesh_ops
    *mesh, det = mesh_ops.clean_mesh(vertices, faces, weld=True, details=True, **{"keep_clusters": None, "normals": False, **clean})
    lap("clean")
    return tuple(mesh), det


def _add_stages(det: dict, clean, outlier, cluster) -> dict:
    """`det` with the statistics of the optional stages that ran, under `clean`, `outlier` and `cluster`."""
    det.update({k: v for k, v in (("clean", clean), ("outlier", outlier), ("cluster", cluster)) if v is not None})
    return det


@torch.no_grad()
def mesh_tsdf(graph_dir_or_yaml, voxel_size: float, trunc: float = None, *, min_weight: float = 1.0, device="cuda",
              details: bool = False, **options):
    """A results directory to a triangle mesh, on the device: `(vertices (3T,3) float32, faces (T,3) int32)` in the world
    frame, a triangle soup in the fixed order of `tsdf.TsdfVolume.extract`.

    `**options` are those of `sample_surface` named in `_SAMPLE_OPTIONS` and those of `mesh_ops.clean_mesh` named in
    `_CLEAN_OPTIONS`, passed on unchanged: the two functions give them their defaults and describe them, `_clean_stage` says
    when the clean stage runs (with `normals=True` the return value is `(vertices, faces, normals)`).  Any other name is a
    TypeError.  Here `outlier_nb` and `cluster_eps` filter the samples that name the TSDF blocks, so a block that only stray
    samples at a depth discontinuity, or a floater's, would have named is never allocated; the clean stage removes the
    floaters a fused LiDAR volume leaves there all the same, closes what a voxel no keyframe observed leaves open
    (`fill_holes`), and takes out the terraces and the per-voxel jitter of a nearest-pixel fusion (`smooth`).

    Pass 1 is `sample_surface` and `tsdf.allocate_blocks` around its cloud: blocks of 8^3 voxels of edge `voxel_size`,
    truncation `trunc` (default 4 voxel_size).  Pass 2 renders every keyframe that contributed samples again (the full
    allmap; the graph, the image size and the poses are those pass 1 read) and fuses it (`TsdfVolume.integrate`, nearest
    pixel, weight 1 per observation); then the zero surface of the voxels seen at least `min_weight` times is extracted.
    Host reads: those of `sample_surface`, one for the number of blocks, one for the number of triangles, one of the clean
    stage.  `details=True` adds dict(blocks, volume_bytes, triangles, samples, frame_ids, stage_ms, volume: the TsdfVolume;
    `clean`, `outlier`, `cluster`: the statistics of the optional stages that ran) and synchronises between the stages to
    time them."""
    from . import tsdf
    sample, clean = _route_options("mesh_tsdf", options)
    dev = _resolve_device("mesh_tsdf", device)
    voxel_size = float(voxel_size)
    trunc = 4.0 * voxel_size if trunc is None else float(trunc)
    stage_ms, lap = _lap_timer(dev, details)
    points, _, sampled, ctx = _sample_surface(graph_dir_or_yaml, dev, True, **sample)
    lap("sample")
    volume = tsdf.TsdfVolume(tsdf.allocate_blocks(points, voxel_size, trunc), voxel_size, trunc)
    lap("allocate")
    graph = ctx["graph"]
    used = [u for u, kept in zip(ctx["used"], ctx["kept"]) if kept]
    poses = [p for p, kept in zip(ctx["poses"], ctx["kept"]) if kept]
    for i, fid, cam, allmap in _render_keyframes(ctx["graph_dir"], graph, used, poses, *ctx["size"], dev):
        volume.integrate(allmap, cam, graph["models"][used[i][0]]["world_T_model"], min_opacity=sample["min_opacity"],
                         max_depth_dist=sample["max_depth_dist"], depth_ratio=1.0 if sample["use_median_depth"] else 0.0)
    lap("integrate")
    vertices, faces = volume.extract(min_weight=min_weight)
    lap("extract")
    mesh, cleaned = _clean_stage(vertices, faces, clean, lap)
    if details:
        det = {"blocks": int(volume.blocks.shape[0]), "volume_bytes": volume.nbytes, "triangles": int(faces.shape[0]),
               "samples": int(points.shape[0]), "frame_ids": [fid for _, fid in used], "stage_ms": stage_ms, "volume": volume}
        return mesh + (_add_stages(det, cleaned, sampled.get("outlier"), sampled.get("cluster")),)
    return mesh


# the options of `sample_surface` that `mesh_depth_check` takes: which keyframes, which of their pixels, which depth
_DEPTH_CHECK_OPTIONS = ("kf_interval", "min_opacity", "max_depth_dist", "use_median_depth", "image_height", "image_width")


@torch.no_grad()
def mesh_depth_check(graph_dir_or_yaml, vertices: torch.Tensor, faces: torch.Tensor, *, truncation: float = 0.5, device="cuda", **options):
    """Does a mesh agree, pixel by pixel, with what the map renders from its own keyframes?  A check that needs no reference
    cloud: for every keyframe of the results graph (those `frames_to_sample` lists) the map is rendered as `sample_surface`
    renders it, the sampler's validity rule is applied (`!(alpha < min_opacity) && !(dist > max_depth_dist)`), and the mesh
    (world frame, e.g. `mesh_tsdf`'s) is rendered from the same pose by `evaluation.render_mesh`'s rays against an index
    built once.  It catches what a cloud-free look cannot otherwise: surface the mesher extrapolated where nothing was
    observed shows as valid pixels whose mesh range is off, and holes as valid pixels the mesh does not cover.

    `**options`: `kf_interval`, `min_opacity`, `max_depth_dist`, `use_median_depth` (the map's depth is the median depth
    instead of the expected one: depth_ratio 1 instead of 0), `image_height`, `image_width` — `sample_surface`'s, with its
    defaults; any other name is a TypeError.  Returns dict(frame_ids, keyframes: per keyframe dict(valid: valid pixels,
    covered: those of them the mesh covers, mean, median: of min(|range_mesh - depth_map|, truncation) over the covered
    ones, None where there is none), and the same four over all keyframes' pixels together).  One host read, at the end:
    the mesh's status words ride with the figures.  ValueError as `evaluation.cast_rays` raises it."""
    from . import evaluation, traj_io
    from .rasterizer import GaussianRasterizationSettings, _stream, get_camera, half_pixel_tables
    for name in options:
        if name not in _DEPTH_CHECK_OPTIONS:
            raise TypeError(f"mesh_depth_check() got an unexpected keyword argument '{name}'")
    defaults = sample_surface.__kwdefaults__
    opt = {k: options.get(k, defaults[k]) for k in _DEPTH_CHECK_OPTIONS}
    truncation = evaluation._check_truncation(truncation)
    dev = _resolve_device("mesh_depth_check", device)
    vertices, faces = evaluation._mesh(vertices, faces)
    if vertices.device != dev:
        raise ValueError(f"the mesh lives on {vertices.device}, not on {dev}")
    path = Path(graph_dir_or_yaml)
    graph_file = path / "graph.yaml" if path.is_dir() else path
    graph_dir = graph_file.parent
    graph = traj_io.read_graph(graph_file)
    H, W = _image_size(graph_dir, opt["image_height"], opt["image_width"])
    used = frames_to_sample(graph, opt["kf_interval"])
    frames = {int(fr["id"]): fr for fr in graph["frames"]}
    poses = [_pose44(frames[fid]["model_T_frame"]) for _, fid in used]
    # sensor frame -> world, per keyframe: composed on the host in float64 from the view matrix the map is rendered with
    Ms = [np.vstack([compose_cam_to_world(graph["models"][mi]["world_T_model"], np.linalg.inv(p).astype(np.float32)).reshape(3, 4),
                     np.array([[0, 0, 0, 1]], np.float32)]) for (mi, _), p in zip(used, poses)]
    Ms_dev = torch.from_numpy(np.ascontiguousarray(np.stack(Ms) if Ms else np.zeros((0, 4, 4), np.float32))).to(dev)
    ratio = 1.0 if opt["use_median_depth"] else 0.0
    lib = _abi.lib()
    F = len(used)
    stats = torch.zeros((F + 1, 4), dtype=torch.float64, device=dev)
    residuals = torch.full((max(F, 1), H * W), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        index = evaluation._ray_index_enqueue(lib, vertices, faces, _stream(dev))
        status = index.status
        for i, fid, cam, allmap in _render_keyframes(graph_dir, graph, used, poses, H, W, dev):
            ce = get_camera(GaussianRasterizationSettings(H, W, 1.0, cam.world_view_transform, cam.projection_matrix), dev)
            col_half, row_half = half_pixel_tables(ce, dev)
            rng, face, _, status = evaluation._render_mesh_enqueue(lib, index, col_half, row_half, Ms_dev[i], math.inf, _stream(dev))
            alpha, dist = allmap[1], allmap[6]
            valid = ~(alpha < opt["min_opacity"]) & ~(dist > opt["max_depth_dist"])
            expected = torch.where(alpha > 0, allmap[0] / torch.where(alpha > 0, alpha, torch.ones_like(alpha)), allmap[0])
            depth = expected * (1.0 - ratio) + allmap[5] * ratio
            covered = valid & (face >= 0)
            res = torch.where(covered, (rng - depth).abs().clamp(max=truncation), torch.full_like(rng, float("nan")))
            residuals[i] = res.reshape(-1)
            stats[i, 0], stats[i, 1] = valid.sum(), covered.sum()
            stats[i, 2] = torch.nansum(res.double())
            stats[i, 3] = torch.nanmedian(res)
        stats[F, :3] = stats[:F, :3].sum(0)
        stats[F, 3] = torch.nanmedian(residuals)
        words = torch.cat([stats.reshape(-1), status.double()]).cpu().numpy()      # the one host read
    evaluation._mesh_distance_status([int(w) for w in words[-4:]], "mesh_depth_check")
    table = words[:-4].reshape(F + 1, 4)

    def row(r):
        n = int(r[1])
        return {"valid": int(r[0]), "covered": n, "mean": float(r[2] / n) if n else None, "median": float(r[3]) if n else None}
    return dict(row(table[F]), frame_ids=[fid for _, fid in used], keyframes=[dict(row(table[i]), frame_id=used[i][1]) for i in range(F)],
                truncation=truncation)


@torch.no_grad()
def mesh_poisson(graph_dir_or_yaml, voxel_size: float, *, margin: float = None, screening: float = 4.0, iterations: int = 300,
                 tol: float = 1e-4, min_density=None, min_density_quantile=None, density_sweeps: int = 2, device="cuda",
                 details: bool = False, **options):
    """The reference's `mesh_poisson` (scene/postprocessing.py) to its end, on the device: `sample_surface`, then
    `poisson.reconstruct` on the merged oriented cloud — blocks `margin` around the samples, the splat, the screened solve,
    marching tetrahedra — the density trim, and the clean stage of `mesh_tsdf`.  `**options` are those of `mesh_tsdf`: the
    names in `_SAMPLE_OPTIONS` go to `sample_surface` and those in `_CLEAN_OPTIONS` to `mesh_ops.clean_mesh`, unchanged
    (`normals=True` returns `(vertices, faces, normals)`); any other name is a TypeError.

    What it IS NOT: Open3D's octree solver.  It is a uniform band of `voxel_size` voxels with trilinear splats (see
    `poisson.py`); `voxel_size` takes the place of the reference's octree `depth`.  `min_density=t` trims by an absolute
    smoothed density; `min_density_quantile=q` takes t as the q-quantile of the smoothed density over the voxels with
    W > 0 (torch on the device, over an even stride of them beyond 4 M: plumbing, one more host read).  That is NOT the reference's `poisson_min_density`, which is
    a quantile of the vertex densities of Open3D's octree: no parity is claimed.  `margin`, `screening`, `iterations`, `tol`
    and `density_sweeps` are judgements (`poisson.py` says why).

    Host reads: those of `sample_surface`, one for the blocks, one for the solve, one for the triangles.  `details=True` adds
    dict(blocks, triangles, samples, solve, min_density, stage_ms, volume: the PoissonVolume; `clean`, `outlier`, `cluster` as
    `mesh_tsdf` adds them) and synchronises between the stages to time them."""
    from . import poisson, tsdf
    sample, clean = _route_options("mesh_poisson", options)
    if min_density is not None and min_density_quantile is not None:
        raise ValueError("give min_density or min_density_quantile, not both")
    if min_density_quantile is not None and not (0.0 <= float(min_density_quantile) <= 1.0):
        raise ValueError("min_density_quantile must lie in [0, 1]")
    dev = _resolve_device("mesh_poisson", device)
    voxel_size = float(voxel_size)
    margin = poisson.DEFAULT_MARGIN_VOXELS * voxel_size if margin is None else float(margin)
    stage_ms, lap = _lap_timer(dev, details)
    points, cloud_normals, sampled, _ = _sample_surface(graph_dir_or_yaml, dev, True, **sample)
    lap("sample")
    volume = poisson.PoissonVolume(tsdf.allocate_blocks(points, voxel_size, margin), voxel_size)
    lap("allocate")
    volume.splat(points, cloud_normals)
    lap("splat")
    solved = volume.solve(screening=screening, iterations=iterations, tol=tol)
    lap("solve")
    threshold = None if min_density is None else float(min_density)
    if min_density_quantile is not None:
        dens = volume.density(density_sweeps)
        seen = dens[volume.field[..., 3] > 0]
        threshold = float(torch.quantile(seen[:: max(1, seen.numel() // (1 << 22))], float(min_density_quantile))) if seen.numel() else 0.0
    vertices, faces = volume.extract(min_density=threshold, density_sweeps=density_sweeps)
    lap("extract")
    mesh, cleaned = _clean_stage(vertices, faces, clean, lap)
    if details:
        det = {"blocks": int(volume.blocks.shape[0]), "triangles": int(faces.shape[0]), "samples": int(points.shape[0]), "solve": solved,
               "min_density": threshold, "frame_ids": sampled["frame_ids"], "stage_ms": stage_ms, "volume": volume}
        return mesh + (_add_stages(det, cleaned, sampled.get("outlier"), sampled.get("cluster")),)
    return mesh
