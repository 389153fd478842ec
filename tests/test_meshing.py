"""The meshing front ends (meshing.mesh_tsdf, meshing.mesh_poisson) with every optional stage on, against the same
stages composed by hand with the same values, bit for bit, `details` included: an option that reached the wrong stage, or
none, shows as other bits.  One keyframe of the synthetic room of tests/helpers.py, sampled once for all tests."""
import numpy as np
import pytest
import torch

from helpers import write_room
from splat_loam_amd import mesh_ops, meshing, poisson, traj_io

pytestmark = pytest.mark.gpu

VS, BASE = 0.1, dict(kf_samples=4000, seed=0x5EED)
# every stage on, and beside the switches a value that is not the default wherever the bits can depend on it.  The room's
# 4000 samples lie about 0.14 m apart (a shell of 2.5 m): a radius of 0.5 m holds some forty of them.
SAMPLE = dict(BASE, outlier_nb=20, outlier_std=1.5, cluster_eps=0.5, cluster_min_points=5, cluster_keep=2, cluster_min_size=100)
CLEAN = dict(keep_clusters=1, min_triangles=20, normals=True, simplify=2 * VS, contraction="quadric", regularisation=1e-2, smooth=2,
             smooth_method="laplacian", smooth_weights="uniform", smooth_lambda=0.4, fix_boundary=True, fill_holes=16, fill_max_size=1.0)
# the same values without the switches: nothing of this may run a stage or move a bit
DORMANT = {k: v for k, v in {**SAMPLE, **CLEAN}.items() if k not in ("outlier_nb", "cluster_eps", "keep_clusters", "normals", "simplify",
                                                                     "smooth", "fill_holes")}


@pytest.fixture(scope="module")
def room(device, tmp_path_factory):
    """(the results directory, `sample_surface(**SAMPLE, details=True)` of it)"""
    d = tmp_path_factory.mktemp("room")
    write_room(d)
    return d, meshing.sample_surface(d, device=device, details=True, **SAMPLE)


def _same(a, b, what):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b))
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    else:
        assert a == b, (what, a, b)


def test_mesh_poisson_with_every_stage_on(device, room):
    d, (pts, nrm, sdet) = room
    *mesh, det = meshing.mesh_poisson(d, VS, device=device, details=True, **SAMPLE, **CLEAN)
    *want, clean = mesh_ops.clean_mesh(*poisson.reconstruct(pts, nrm, VS), weld=True, details=True, **CLEAN)
    print(f"{det['samples']} samples, {det['triangles']} triangles -> {mesh[1].shape[0]}; outlier {det['outlier']['removed']}, "
          f"cluster {det['cluster']['removed']}, clean {sorted(det['clean'])}")
    assert len(mesh) == len(want) == 3 and det["samples"] == pts.shape[0] > 0 and mesh[1].shape[0] > 100
    for got, ref, name in zip(mesh, want, ("vertices", "faces", "normals")):
        assert torch.equal(got, ref), name
    assert "index" in det["outlier"] and "index" in det["cluster"] and "vmap" in det["clean"]["simplify"]
    assert {"smooth", "fill"} <= set(det["clean"]) and "clean" in det["stage_ms"]
    _same(det["outlier"], sdet["outlier"], "outlier")
    _same(det["cluster"], sdet["cluster"], "cluster")
    _same(det["clean"], clean, "clean")


def test_mesh_tsdf_with_every_stage_on(device, room):
    d, (pts, _, sdet) = room
    *mesh, det = meshing.mesh_tsdf(d, VS, device=device, details=True, **SAMPLE, **CLEAN)
    *want, clean = mesh_ops.clean_mesh(*meshing.mesh_tsdf(d, VS, device=device, **SAMPLE), weld=True, details=True, **CLEAN)
    assert len(mesh) == len(want) == 3 and mesh[1].shape[0] > 100
    for got, ref, name in zip(mesh, want, ("vertices", "faces", "normals")):
        assert torch.equal(got, ref), name
    assert det["samples"] == pts.shape[0] and det["frame_ids"] == sdet["frame_ids"] and "clean" in det["stage_ms"]
    _same(det["outlier"], sdet["outlier"], "outlier")
    _same(det["cluster"], sdet["cluster"], "cluster")
    _same(det["clean"], clean, "clean")


@pytest.mark.parametrize("front_end", ["mesh_tsdf", "mesh_poisson"])
def test_defaults_run_no_optional_stage(device, room, front_end):
    """Two tensors, no `clean`, `outlier` or `cluster` in `details`; the dependent options of a stage that is off change nothing."""
    d, fn = room[0], getattr(meshing, front_end)
    plain = fn(d, VS, device=device, **BASE)
    assert len(plain) == 2 and plain[0].shape == (3 * plain[1].shape[0], 3) and plain[1].shape[0] > 100
    *mesh, det = fn(d, VS, device=device, details=True, **DORMANT)
    assert len(mesh) == 2 and torch.equal(mesh[0], plain[0]) and torch.equal(mesh[1], plain[1])
    assert not {"clean", "outlier", "cluster"} & set(det) and "clean" not in det["stage_ms"]


def test_mesh_tsdf_reads_the_graph_once(device, room, monkeypatch):
    """The fusion pass takes the graph, the image size, the frames and their poses from the sampling pass."""
    calls, read_graph = [], traj_io.read_graph
    monkeypatch.setattr(traj_io, "read_graph", lambda *a, **kw: calls.append(a) or read_graph(*a, **kw))
    meshing.mesh_tsdf(room[0], VS, device=device, **BASE)
    assert len(calls) == 1
