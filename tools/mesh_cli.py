"""What tools/mesh_tsdf.py, tools/mesh_poisson.py and tools/sample_surface.py share: the flags of the options that
`splat_loam_amd.meshing` routes by `_SAMPLE_OPTIONS` (to `sample_surface`) and `_CLEAN_OPTIONS` (to `mesh_ops.clean_mesh`),
each declared once; the parsed flags as the keyword arguments of those functions; and the fragments of the tools' JSON line
that report the optional stages.  A stage that gains an option gains its flag here (tests/test_meshing_host.py compares)."""
from splat_loam_amd import meshing

# library-only: options of the two tuples that have no flag, on purpose (whoever gives one a flag below takes its name out here)
LIBRARY_ONLY = ("cluster_keep", "cluster_min_size", "smooth_lambda", "smooth_mu")


def add_sample_arguments(ap):
    """The sampling thresholds, the seed, the image size and the device."""
    ap.add_argument("--kf-interval", type=int, default=-1)
    ap.add_argument("--kf-samples", type=int, default=5000)
    ap.add_argument("--min-opacity", type=float, default=0.5)
    ap.add_argument("--max-depth-dist", type=float, default=0.1)
    ap.add_argument("--use-median-depth", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--image-height", type=int, default=None)
    ap.add_argument("--image-width", type=int, default=None)
    ap.add_argument("--device", default="cuda")


def add_cloud_arguments(ap):
    """The outlier filter and the cluster selection of the sampled cloud."""
    ap.add_argument("--outlier-nb", type=int, default=None, help="statistical outlier removal of the surface samples: neighbours (1..32)")
    ap.add_argument("--outlier-std", type=float, default=2.0, help="... and the threshold in standard deviations (with --outlier-nb)")
    ap.add_argument("--cluster-eps", type=float, default=None, help="keep the largest DBSCAN cluster of the surface samples: the radius, a few sample spacings")
    ap.add_argument("--cluster-min-points", type=int, default=10, help="... and the neighbours, itself included, that make a sample core (with --cluster-eps)")


def add_clean_arguments(ap):
    """The clean-up of the extracted mesh."""
    ap.add_argument("--keep-clusters", type=int, default=None, help="weld, then keep the K largest clusters of triangles")
    ap.add_argument("--min-triangles", type=int, default=50, help="... and every cluster of at least N triangles (with --keep-clusters)")
    ap.add_argument("--normals", action="store_true", help="weld and write area-weighted vertex normals")
    ap.add_argument("--simplify", type=float, default=None, help="weld, then merge the vertices of every voxel of this edge (metres)")
    ap.add_argument("--contraction", choices=("average", "quadric"), default="average", help="where a merged vertex goes (with --simplify)")
    ap.add_argument("--regularisation", type=float, default=1e-3, help="pull of the quadric placement towards the mean (with --simplify)")
    ap.add_argument("--smooth", type=int, default=None, help="weld, then run N smoothing sweeps over the edge graph")
    ap.add_argument("--smooth-method", choices=("taubin", "laplacian", "simple"), default="taubin", help="the sweep (with --smooth)")
    ap.add_argument("--smooth-weights", choices=("inverse_distance", "uniform"), default="inverse_distance", help="neighbour weights (with --smooth)")
    ap.add_argument("--fix-boundary", action="store_true", help="leave the boundary vertices where they are (with --smooth)")
    ap.add_argument("--fill-holes", type=int, default=None, help="weld, then fill the boundary loops of at most N edges")
    ap.add_argument("--fill-max-size", type=float, default=None, help="... whose bounding box has at most this diagonal (with --fill-holes)")


def _options(a, names):
    return {k: getattr(a, k) for k in names if k not in LIBRARY_ONLY}


def sample_options(a):
    """The parsed flags of `add_sample_arguments` and `add_cloud_arguments` as keyword arguments of `meshing.sample_surface`."""
    return _options(a, meshing._SAMPLE_OPTIONS)


def clean_options(a):
    """The parsed flags of `add_clean_arguments` as the clean-up keyword arguments of `meshing.mesh_tsdf` / `mesh_poisson`."""
    return _options(a, meshing._CLEAN_OPTIONS)


def cloud_report(det, a):
    """The statistics of the outlier and cluster stages that ran, with their arguments: no row index."""
    line = {}
    if "outlier" in det:
        line["outlier"] = dict({k: v for k, v in det["outlier"].items() if k != "index"}, nb_neighbors=a.outlier_nb, std_ratio=a.outlier_std)
    if "cluster" in det:
        line["cluster"] = dict({k: v for k, v in det["cluster"].items() if k != "index"}, eps=a.cluster_eps, min_points=a.cluster_min_points)
    return line


def clean_report(det, a, faces):
    """The statistics of the clean stage (of the welded mesh) and of those of its parts that ran, with their arguments: no vertex map."""
    clean = det["clean"]
    line = {k: clean[k] for k in ("welded_vertices", "clusters", "degenerate", "boundary_edges", "nonmanifold_edges", "n_min")}
    line["triangles_kept"] = int(faces.shape[0])
    line["normals"] = bool(a.normals)
    if "simplify" in clean:
        line["simplify"] = dict({k: v for k, v in clean["simplify"].items() if k != "vmap"}, voxel=a.simplify, contraction=a.contraction)
    if "smooth" in clean:
        line["smooth"] = dict(clean["smooth"], iterations=a.smooth, method=a.smooth_method, weights=a.smooth_weights,
                              fix_boundary=bool(a.fix_boundary))
    if "fill" in clean:
        line["fill"] = dict(clean["fill"], max_edges=a.fill_holes, max_size=a.fill_max_size)
    return line
