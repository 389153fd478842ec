"""Host side of the meshing front ends (splat_loam_amd/meshing.py: mesh_tsdf, mesh_poisson) and of the three tools over
them (tools/mesh_cli.py): the two tuples that route the options against the functions they go to, what is rejected before
any file is opened or any device is named, and the tools' flags against the library's options.  No device needed."""
import argparse
import inspect
import json
import os
import sys

import pytest
import torch

from splat_loam_amd import mesh_ops, meshing

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
FRONT_ENDS = (meshing.mesh_tsdf, meshing.mesh_poisson)
FRONT_END_DEFAULTS = {"keep_clusters": None, "normals": False}      # where the front ends differ from clean_mesh, on purpose


def _keywords(fn):
    return {n: p.default for n, p in inspect.signature(fn).parameters.items() if p.kind is p.KEYWORD_ONLY}


def _tools():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import mesh_cli
    import mesh_poisson
    import mesh_tsdf
    import sample_surface
    return mesh_cli, {"mesh_tsdf": (mesh_tsdf, ["RESULTS", "OUT.ply", "--voxel", "0.1"]),
                      "mesh_poisson": (mesh_poisson, ["RESULTS", "OUT.ply", "--voxel", "0.1"]),
                      "sample_surface": (sample_surface, ["RESULTS", "OUT.ply"])}


def test_the_tuples_name_parameters_of_the_functions_they_go_to():
    sample, clean = set(meshing._SAMPLE_OPTIONS), set(meshing._CLEAN_OPTIONS)
    assert len(sample) == len(meshing._SAMPLE_OPTIONS) == 14 and len(clean) == len(meshing._CLEAN_OPTIONS) == 14
    assert sample <= set(_keywords(meshing.sample_surface)) and clean <= set(_keywords(mesh_ops.clean_mesh))
    assert not sample & clean
    for fn in FRONT_ENDS:
        own = set(inspect.signature(fn).parameters)
        assert not own & (sample | clean), fn.__name__
        assert {"device", "details"} <= own and "options" in own


@pytest.mark.parametrize("fn", FRONT_ENDS)
def test_an_unknown_option_is_a_type_error(fn, tmp_path):
    with pytest.raises(TypeError, match="no_such_option"):
        fn(tmp_path / "no_such_results", 0.1, no_such_option=1)
    with pytest.raises(TypeError, match="no_such_option"):          # ... the first check: before the outlier arguments
        fn(tmp_path / "no_such_results", 0.1, no_such_option=1, outlier_nb=0, device="cpu")
    for unexposed in ("fill_capacity", "weld"):                     # of clean_mesh: not options of a front end
        with pytest.raises(TypeError, match=unexposed):
            fn(tmp_path / "no_such_results", 0.1, **{unexposed: 1})


@pytest.mark.parametrize("fn", FRONT_ENDS)
def test_the_options_are_checked_before_the_device_and_the_device_before_any_file(fn, tmp_path):
    missing = tmp_path / "no_such_results"
    with pytest.raises(ValueError, match="nb_neighbors"):
        fn(missing, 0.1, outlier_nb=0, device="cpu")
    with pytest.raises(ValueError, match="std_ratio"):
        fn(missing, 0.1, outlier_nb=20, outlier_std=0.0, device="cpu")
    with pytest.raises(ValueError, match="nb_neighbors"):           # the outlier arguments before the cluster arguments
        fn(missing, 0.1, outlier_nb=0, cluster_eps=-1.0, device="cpu")
    with pytest.raises(ValueError, match="eps"):
        fn(missing, 0.1, cluster_eps=-1.0, device="cpu")
    with pytest.raises(ValueError, match="min_points"):
        fn(missing, 0.1, cluster_eps=0.5, cluster_min_points=0, device="cpu")
    with pytest.raises(ValueError, match="keep must be an integer"):
        fn(missing, 0.1, cluster_eps=0.5, cluster_keep=1.5, device="cpu")
    with pytest.raises(RuntimeError, match=f"{fn.__name__} runs on a ROCm device"):
        fn(missing, 0.1, outlier_nb=20, cluster_eps=0.5, keep_clusters=1, device="cpu")
    assert meshing._check_cluster(None, "ignored", "ignored", "ignored") is None
    assert meshing._check_cluster(0.5, 10, 1, 0) == (0.5, 10, 1, 0)


def test_mesh_poisson_checks_its_own_arguments_between_the_two(tmp_path):
    missing = tmp_path / "no_such_results"
    with pytest.raises(ValueError, match="not both"):
        meshing.mesh_poisson(missing, 0.1, min_density=1.0, min_density_quantile=0.1, device="cpu")
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        meshing.mesh_poisson(missing, 0.1, min_density_quantile=1.5, device="cpu")
    with pytest.raises(ValueError, match="eps"):                    # the cluster arguments come first
        meshing.mesh_poisson(missing, 0.1, min_density=1.0, min_density_quantile=0.1, cluster_eps=0.0)


def test_the_tools_flags_are_the_librarys_options():
    """The drift guard: a stage that gains an option in the library alone, or in one tool alone, fails here."""
    mesh_cli, tools = _tools()
    library_only = set(mesh_cli.LIBRARY_ONLY)
    assert library_only == {"cluster_keep", "cluster_min_size", "smooth_lambda", "smooth_mu"}
    sample_defaults, clean_defaults = _keywords(meshing.sample_surface), dict(_keywords(mesh_ops.clean_mesh), **FRONT_END_DEFAULTS)
    parsed = {}
    for name, (module, argv) in tools.items():
        a = module.build_parser().parse_args(argv)
        sample = mesh_cli.sample_options(a)
        assert set(sample) == set(meshing._SAMPLE_OPTIONS) - library_only, name
        assert sample == {k: sample_defaults[k] for k in sample}, name
        assert a.device == sample_defaults["device"]
        parsed[name] = (sample, None)
        if name != "sample_surface":
            clean = mesh_cli.clean_options(a)
            assert set(clean) == set(meshing._CLEAN_OPTIONS) - library_only, name
            assert clean == {k: clean_defaults[k] for k in clean}, name
            parsed[name] = (sample, clean)
    assert parsed["mesh_tsdf"] == parsed["mesh_poisson"] and parsed["sample_surface"][0] == parsed["mesh_tsdf"][0]
    # the same flags, with the same types, defaults, choices and help, in all three: each is declared once
    def shared(module):
        return {s: (act.type, act.default, act.choices, act.help, type(act)) for act in module.build_parser()._actions
                for s in act.option_strings if "--" + act.dest.replace("_", "-") == s}
    flags = {name: shared(module) for name, (module, _) in tools.items()}
    cloud = {"--" + k.replace("_", "-") for k in set(meshing._SAMPLE_OPTIONS) - library_only} | {"--device"}
    cleanup = {"--" + k.replace("_", "-") for k in set(meshing._CLEAN_OPTIONS) - library_only}
    for name in tools:
        assert cloud <= set(flags[name]), name
        assert all(flags[name][s] == flags["mesh_tsdf"][s] for s in cloud), name
    assert cleanup <= set(flags["mesh_poisson"]) and all(flags["mesh_poisson"][s] == flags["mesh_tsdf"][s] for s in cleanup)
    assert not cleanup & set(flags["sample_surface"])
    # a value given on the command line arrives under the option's name
    a = tools["mesh_poisson"][0].build_parser().parse_args(["R", "O.ply", "--voxel", "0.1", "--outlier-nb", "20", "--cluster-eps", "0.5",
                                                            "--normals", "--smooth", "3", "--smooth-method", "laplacian", "--kf-samples", "7"])
    sample, clean = mesh_cli.sample_options(a), mesh_cli.clean_options(a)
    assert (sample["outlier_nb"], sample["cluster_eps"], sample["kf_samples"]) == (20, 0.5, 7)
    assert (clean["normals"], clean["smooth"], clean["smooth_method"], clean["keep_clusters"]) == (True, 3, "laplacian", None)


def test_the_report_fragments_hold_no_tensor():
    mesh_cli, _ = _tools()
    a = argparse.Namespace(outlier_nb=20, outlier_std=2.0, cluster_eps=0.5, cluster_min_points=10, normals=True, simplify=0.2,
                           contraction="quadric", smooth=3, smooth_method="taubin", smooth_weights="uniform", fix_boundary=False,
                           fill_holes=16, fill_max_size=None)
    index = torch.arange(4)
    clean = {"welded_vertices": 90, "clusters": 3, "degenerate": 0, "boundary_edges": 12, "nonmanifold_edges": 0, "n_min": 50, "kept": 2,
             "simplify": {"vertices": 40, "collapsed": 50, "vmap": index}, "smooth": {"live": 40, "boundary": 6, "nonfinite": 0},
             "fill": {"loops": 2, "filled": 1}}
    det = {"outlier": {"removed": 3, "threshold": 0.25, "index": index}, "cluster": {"clusters": 2, "removed": 1, "index": index},
           "clean": clean}
    faces = torch.zeros((70, 3), dtype=torch.int32)
    line = dict(mesh_cli.cloud_report(det, a), clean=mesh_cli.clean_report(det, a, faces))
    text = json.dumps(line)
    assert "index" not in text and "vmap" not in text
    assert line["outlier"] == {"removed": 3, "threshold": 0.25, "nb_neighbors": 20, "std_ratio": 2.0}
    assert line["cluster"] == {"clusters": 2, "removed": 1, "eps": 0.5, "min_points": 10}
    assert line["clean"] == {"welded_vertices": 90, "clusters": 3, "degenerate": 0, "boundary_edges": 12, "nonmanifold_edges": 0, "n_min": 50,
                             "triangles_kept": 70, "normals": True,
                             "simplify": {"vertices": 40, "collapsed": 50, "voxel": 0.2, "contraction": "quadric"},
                             "smooth": {"live": 40, "boundary": 6, "nonfinite": 0, "iterations": 3, "method": "taubin", "weights": "uniform",
                                        "fix_boundary": False},
                             "fill": {"loops": 2, "filled": 1, "max_edges": 16, "max_size": None}}
    # a stage that did not run leaves no fragment
    bare = {k: v for k, v in clean.items() if k not in ("simplify", "smooth", "fill")}
    assert mesh_cli.cloud_report({"blocks": 1}, a) == {}
    assert not {"simplify", "smooth", "fill"} & set(mesh_cli.clean_report({"clean": bare}, a, faces))
