"""Cleaning an extracted mesh on the device: the last stage of graph.yaml -> mesh -> evaluate_recon.

`weld` merges the bit-equal rows of a triangle soup (sls_mesh_weld: what `tsdf.weld_soup` does with `torch.unique`),
`cluster_triangles` labels the edge-connected clusters of triangles and counts boundary and non-manifold edges
(sls_mesh_clusters: union-find over triangles, driven by the sorted edge list), `keep_clusters` keeps the largest clusters
and those above a floor of triangles and compacts the mesh (sls_mesh_filter: the post-processing of the 2DGS mesher),
`vertex_normals` gives every vertex its area-weighted normal (sls_mesh_vertex_normals: Open3D's
`compute_vertex_normals`), `simplify_vertex_clustering` makes the mesh smaller (sls_mesh_simplify: Open3D's
`simplify_vertex_clustering`, average or quadric contraction), `vertex_adjacency` gives every vertex its distinct
neighbours in CSR form and `smooth` moves every vertex towards them (sls_mesh_adjacency, sls_mesh_smooth: Open3D's
`filter_smooth_taubin`, `filter_smooth_laplacian`, `filter_smooth_simple`), `boundary_loops` lists the boundary half-edges
of a mesh and the closed loops they form and `fill_holes` closes the small ones with a fan over their centroid
(sls_mesh_boundary_loops, sls_mesh_fill_holes: no refinement, no fairing, and chains that meet at a non-manifold vertex
stay open), `clean_mesh` chains them.
include/sls_mesh_math.h, include/sls_simplify_math.h, include/sls_smooth_math.h and include/sls_fill_math.h state every
rule, DESIGN.md section 2 ("Mesh cleaning", "Mesh simplification", "Mesh smoothing", "Mesh hole filling") the contract,
tests/mesh_ref.py, tests/simplify_ref.py, tests/smooth_ref.py and tests/fill_ref.py restate it in NumPy.  Device tensors
only; there is no CPU path.

Host reads: `weld`, `cluster_triangles`, `keep_clusters`, `simplify_vertex_clustering`, `vertex_adjacency`, `smooth`,
`boundary_loops`, `fill_holes` and `clean_mesh` one each (the status words, read once at the end: outputs are allocated at
capacity and sliced), `vertex_normals` none.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _abi
from .tsdf import _device_points, _stream

MAX_TRIANGLES = 1 << 29              # SLS_MESH_MAX_TRIANGLES


def _device_faces(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm device tensor (libsls_hip.so); there is no CPU fallback")
    t = t.detach()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be (T,3)")
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be int32 or int64")
    if t.shape[0] > MAX_TRIANGLES:
        raise ValueError(f"{name} holds more than {MAX_TRIANGLES} triangles")
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t.contiguous()


def _scratch(nbytes, dev):
    """(the tensor that owns the bytes, a 256-byte aligned address inside it)"""
    buf = torch.empty((int(nbytes) + 256,), dtype=torch.uint8, device=dev)
    return buf, (buf.data_ptr() + 255) & ~255


def _words(status):
    return status.cpu().numpy().view(np.uint32)


# ---- the launches: outputs at capacity, status words on the device, nothing read back --------------------------------
def _weld_launch(rows, status):
    """rows (N,3) float32 -> (vertices at capacity (N,3), index (N,) int32); status: 4 int32 words on the device."""
    lib, dev, N = _abi.lib(), rows.device, int(rows.shape[0])
    out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    index = torch.empty((N,), dtype=torch.int32, device=dev)
    nbytes = int(lib.sls_mesh_weld_scratch_bytes(N))
    keep, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_weld(N, rows.data_ptr(), out.data_ptr(), index.data_ptr(), status.data_ptr(), ptr, nbytes, _stream(dev)),
               "sls_mesh_weld")
    return out, index


def _clusters_launch(faces, n_vertices, status):
    """faces (T,3) int32 -> (labels (T,) int32, counts at capacity (T,) int32); status: 6 int32 words on the device."""
    lib, dev, T = _abi.lib(), faces.device, int(faces.shape[0])
    labels = torch.empty((T,), dtype=torch.int32, device=dev)
    counts = torch.empty((T,), dtype=torch.int32, device=dev)
    nbytes = int(lib.sls_mesh_clusters_scratch_bytes(T))
    keep, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_clusters(T, faces.data_ptr(), int(n_vertices), labels.data_ptr(), counts.data_ptr(), status.data_ptr(), ptr,
                                     nbytes, _stream(dev)), "sls_mesh_clusters")
    return labels, counts


def _filter_launch(vertices, faces, labels, counts, cluster_status, keep, min_triangles, status):
    """-> (vertices at capacity (V,3), faces at capacity (T,3), rows past the kept ones -1); status: 4 words."""
    lib, dev, V, T = _abi.lib(), vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    out_v = torch.empty((V, 3), dtype=torch.float32, device=dev)
    out_f = torch.full((T, 3), -1, dtype=torch.int32, device=dev)
    nbytes = int(lib.sls_mesh_filter_scratch_bytes(V, T))
    hold, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_filter(V, vertices.data_ptr(), T, faces.data_ptr(), labels.data_ptr(), counts.data_ptr(),
                                   cluster_status.data_ptr(), int(keep), int(min_triangles), out_v.data_ptr(), out_f.data_ptr(), None,
                                   status.data_ptr(), ptr, nbytes, _stream(dev)), "sls_mesh_filter")
    return out_v, out_f


def _normals_launch(vertices, faces):
    lib, dev, V, T = _abi.lib(), vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    nbytes = int(lib.sls_mesh_vertex_normals_scratch_bytes(V, T))
    hold, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_vertex_normals(V, vertices.data_ptr(), T, faces.data_ptr(), out.data_ptr(), ptr, nbytes, _stream(dev)),
               "sls_mesh_vertex_normals")
    return out


CONTRACTIONS = {"average": 0, "quadric": 1}


def _simplify_args(voxel_size, contraction, regularisation):
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {sorted(CONTRACTIONS)}, not {contraction!r}")
    voxel_size, regularisation = float(voxel_size), float(regularisation)
    if not (np.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError("voxel_size must be finite and > 0")
    if not (np.isfinite(regularisation) and regularisation >= 0):
        raise ValueError("regularisation must be finite and >= 0")
    return voxel_size, CONTRACTIONS[contraction], regularisation


def _simplify_launch(vertices, faces, voxel_size, contraction, regularisation, status):
    """-> (vertices at capacity (V,3), faces at capacity (T,3), rows past the kept ones -1, vmap (V,)); status: 8 words.
    `contraction` is the integer of the C entry."""
    lib, dev, V, T = _abi.lib(), vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    out_v = torch.empty((V, 3), dtype=torch.float32, device=dev)
    out_f = torch.full((T, 3), -1, dtype=torch.int32, device=dev)
    vmap = torch.empty((V,), dtype=torch.int32, device=dev)
    nbytes = int(lib.sls_mesh_simplify_scratch_bytes(V, T))
    hold, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_simplify(V, vertices.data_ptr(), T, faces.data_ptr(), float(voxel_size), int(contraction),
                                     float(regularisation), out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), status.data_ptr(), ptr,
                                     nbytes, _stream(dev)), "sls_mesh_simplify")
    return out_v, out_f, vmap


def _simplify_details(w):
    return {"vertices": int(w[0]), "triangles": int(w[1]), "nonfinite": int(w[2]), "out_of_grid": int(w[3]), "collapsed": int(w[4]),
            "duplicates": int(w[5]), "fallbacks": int(w[6])}


def _simplify_errors(w, voxel_size):
    if w[2]:
        raise ValueError(f"{int(w[2])} vertices that a triangle references hold a non-finite coordinate")
    if w[3]:
        raise ValueError(f"{int(w[3])} vertices lie 2^21 voxels or more from the mesh's minimum: voxel_size {voxel_size} is too small")


SMOOTH_METHODS = {"simple": 0, "laplacian": 1, "taubin": 2}
SMOOTH_WEIGHTS = {"uniform": 0, "inverse_distance": 1}


def _smooth_args(iterations, method, weights, lambda_, mu):
    if method not in SMOOTH_METHODS:
        raise ValueError(f"method must be one of {sorted(SMOOTH_METHODS)}, not {method!r}")
    if weights not in SMOOTH_WEIGHTS:
        raise ValueError(f"weights must be one of {sorted(SMOOTH_WEIGHTS)}, not {weights!r}")
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations must be an integer >= 0")
    lambda_, mu = float(lambda_), float(mu)
    if not (np.isfinite(lambda_) and np.isfinite(mu)):
        raise ValueError("lambda_ and mu must be finite")
    return int(iterations), SMOOTH_METHODS[method], SMOOTH_WEIGHTS[weights], lambda_, mu


def _smooth_launch(vertices, faces, iterations, method, weights, lambda_, mu, fix_boundary, status):
    """-> vertices (V,3): every row written; status: 8 words.  `method` and `weights` are the integers of the C entry."""
    lib, dev, V, T = _abi.lib(), vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    nbytes = int(lib.sls_mesh_smooth_scratch_bytes(V, T))
    hold, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_smooth(V, vertices.data_ptr(), T, faces.data_ptr(), int(method), int(weights), int(iterations), float(lambda_),
                                   float(mu), int(bool(fix_boundary)), out.data_ptr(), status.data_ptr(), ptr, nbytes, _stream(dev)),
               "sls_mesh_smooth")
    return out


def _smooth_details(w):
    return {"live": int(w[0]), "edges": int(w[1]), "boundary": int(w[2]), "nonfinite": int(w[3]), "degenerate": int(w[4]),
            "out_of_range": int(w[5]), "max_row": int(w[6])}


def _smooth_errors(w, ranges=True):
    if ranges and w[5]:
        raise _range_error(int(w[5]))
    if w[3]:
        raise ValueError(f"{int(w[3])} vertices that a triangle references hold a non-finite coordinate")


FILL_STATUS = ("vertices", "triangles", "halfedges", "loops", "filled", "skipped_edges", "skipped_size", "skipped_nonfinite",
               "open_halfedges", "complex_vertices", "degenerate", "out_of_range", "needed_vertices", "needed_triangles", "overflow")


def _fill_args(max_edges, max_size, capacity):
    if isinstance(max_edges, bool) or int(max_edges) != max_edges or max_edges < 3:
        raise ValueError("max_edges must be an integer >= 3")
    max_size = 0.0 if max_size is None else float(max_size)
    if not (np.isfinite(max_size) and max_size >= 0):
        raise ValueError("max_size must be finite and >= 0 (None or 0: no limit)")
    capacity = float(capacity)
    if not (np.isfinite(capacity) and capacity >= 0):
        raise ValueError("capacity must be finite and >= 0")
    return int(max_edges), max_size, capacity


def _fill_room(V, T, capacity):
    """(cap_vertices, cap_triangles): room for max(ceil(capacity T), 64) new triangles, and for the vertices they can bring —
    a new vertex comes with at least four new triangles"""
    cap_t = T + max(int(np.ceil(capacity * T)), 64)
    return V + (cap_t - T) // 4 + 1, cap_t


def _fill_launch(vertices, faces, in_counts, max_edges, max_size, capacity, status):
    """-> (vertices at capacity (cap_v,3), faces at capacity (cap_t,3), rows past the written ones -1); status: 16 words.
    `in_counts`: two int32 words on the device [V_live, T_live], or None."""
    lib, dev, V, T = _abi.lib(), vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    cap_v, cap_t = _fill_room(V, T, capacity)
    if cap_t > MAX_TRIANGLES:
        raise ValueError(f"the room for {cap_t} triangles is above {MAX_TRIANGLES}")
    out_v = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((cap_t, 3), dtype=torch.int32, device=dev)
    nbytes = int(lib.sls_mesh_fill_holes_scratch_bytes(V, T))
    hold, ptr = _scratch(nbytes, dev)
    _abi.check(lib.sls_mesh_fill_holes(V, vertices.data_ptr() if V else None, T, faces.data_ptr() if T else None,
                                       in_counts.data_ptr() if in_counts is not None else None, int(max_edges), float(max_size), cap_v,
                                       out_v.data_ptr(), cap_t, out_f.data_ptr(), status.data_ptr(), ptr if nbytes else None, nbytes,
                                       _stream(dev)), "sls_mesh_fill_holes")
    return out_v, out_f


def _fill_details(w):
    return {k: int(w[i]) for i, k in enumerate(FILL_STATUS)}


def _fill_errors(w):
    if w[14]:
        raise ValueError(f"no room to fill the holes: {int(w[13])} triangles and {int(w[12])} vertices are needed; raise `capacity`")


def _status(dev, n):
    return torch.zeros((n,), dtype=torch.int32, device=dev)


def _range_error(n):
    return ValueError(f"{n} triangles hold a vertex index outside the vertices")


def _cluster_details(w):
    return {"clusters": int(w[0]), "degenerate": int(w[1]), "out_of_range": int(w[2]), "boundary_edges": int(w[3]),
            "nonmanifold_edges": int(w[4])}


# ---- the public calls ------------------------------------------------------------------------------------------------
@torch.no_grad()
def weld_rows(rows: torch.Tensor):
    """`(vertices (V,3) float32, index (N,) int32)`: the unique rows of (N,3) float32 device rows, compared as integers, in
    ascending lexicographic order of (x, y, z) as signed int32, and the rank of every row.  One host read (V)."""
    rows = _device_points(rows, "rows")
    dev = rows.device
    with torch.cuda.device(dev):
        status = _status(dev, 4)
        out, index = _weld_launch(rows, status)
        V = int(_words(status)[0])                                  # the one host read
    return out[:V], index


@torch.no_grad()
def weld(soup: torch.Tensor):
    """A triangle soup (3T,3) with its bit-equal vertices merged: `(vertices (V,3) float32, faces (T,3) int32)`, exactly
    what `tsdf.weld_soup` returns (-0.0 and 0.0 stay apart, NaN payloads are compared as bits), by three stable radix sorts
    and a scan instead of `torch.unique`.  One host read (V)."""
    soup = _device_points(soup, "soup")
    if soup.shape[0] % 3:
        raise ValueError("soup must be (3T,3)")
    vertices, index = weld_rows(soup)
    return vertices, index.view(soup.shape[0] // 3, 3)


@torch.no_grad()
def cluster_triangles(faces: torch.Tensor, n_vertices: int, details: bool = False):
    """`(labels (T,) int32, cluster_count (C,) int32)`: the cluster of every triangle — triangles that share an undirected
    edge are joined, clusters are numbered in ascending order of their lowest triangle, a triangle with a repeated index
    carries -1 — and the triangles per cluster.  A face index outside [0, n_vertices) raises.  `details=True` adds
    dict(clusters, degenerate, out_of_range, boundary_edges, nonmanifold_edges): a mesh with neither boundary nor
    non-manifold edges is closed.  One host read (the status words)."""
    faces = _device_faces(faces, "faces")
    dev = faces.device
    with torch.cuda.device(dev):
        status = _status(dev, 8)
        labels, counts = _clusters_launch(faces, int(n_vertices), status)
        w = _words(status)                                          # the one host read
    if w[2]:
        raise _range_error(int(w[2]))
    if details:
        return labels, counts[:int(w[0])], _cluster_details(w)
    return labels, counts[:int(w[0])]


def _keep(vertices, faces, keep, min_triangles, details):
    dev = vertices.device
    with torch.cuda.device(dev):
        status = _status(dev, 16)
        labels, counts = _clusters_launch(faces, int(vertices.shape[0]), status[0:8])
        out_v, out_f = _filter_launch(vertices, faces, labels, counts, status[0:8], keep, min_triangles, status[8:12])
        w = _words(status)                                          # the one host read
    if w[2]:
        raise _range_error(int(w[2]))
    out_v, out_f = out_v[:int(w[8])], out_f[:int(w[9])]
    if details:
        d = _cluster_details(w)
        d.update(cluster_count=counts[:int(w[0])], labels=labels, n_min=int(w[10]))
        return out_v, out_f, d
    return out_v, out_f


@torch.no_grad()
def keep_clusters(vertices: torch.Tensor, faces: torch.Tensor, keep_clusters: int = 1, min_triangles: int = 50, details: bool = False):
    """The mesh with its small clusters dropped: `(vertices (V',3), faces (T',3) int32)`.  With
    n_min = max(min_triangles, the triangles of the k-th largest cluster), k = min(keep_clusters, clusters), a triangle
    stays iff it is non-degenerate and its cluster holds at least n_min triangles (ties at the threshold all stay);
    `keep_clusters <= 0`: the floor alone, `min_triangles <= 0`: no floor.  Kept triangles and the vertices they reference
    stay in input order.  `details=True` adds dict(clusters, cluster_count (a device tensor), labels, degenerate,
    out_of_range, boundary_edges, nonmanifold_edges — all of the INPUT mesh — and n_min).  One host read."""
    vertices = _device_points(vertices, "vertices")
    faces = _device_faces(faces, "faces")
    if faces.device != vertices.device:
        raise ValueError("vertices and faces must live on the same device")
    return _keep(vertices, faces, keep_clusters, min_triangles, details)


@torch.no_grad()
def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """(V,3) float32: per vertex the normalised sum of the un-normalised (area-weighted) normals (p1 - p0) x (p2 - p0) of
    its triangles, summed in ascending triangle index in float32 — bit-reproducible, equal to the header on the host.
    Triangles with a repeated or out-of-range index are skipped; a vertex without a triangle, or with a sum of zero or
    non-finite length, gets zeros.  Nothing is read back."""
    vertices = _device_points(vertices, "vertices")
    faces = _device_faces(faces, "faces")
    if faces.device != vertices.device:
        raise ValueError("vertices and faces must live on the same device")
    with torch.cuda.device(vertices.device):
        return _normals_launch(vertices, faces)


@torch.no_grad()
def simplify_vertex_clustering(vertices: torch.Tensor, faces: torch.Tensor, voxel_size: float, contraction: str = "average",
                               regularisation: float = 1e-3, details: bool = False):
    """The mesh with the vertices of every voxel of edge `voxel_size` merged into one: `(vertices (V',3), faces (T',3) int32)`
    (Open3D's `simplify_vertex_clustering`).  Only vertices that a triangle with three different indices inside the vertices
    references take part; the grid starts half a voxel below their minimum.  `contraction="average"` places a cluster at the
    float64 mean of its vertices, `"quadric"` at the minimum of the cluster's error quadric (area-weighted plane distances
    of every triangle with a corner in it), regularised towards that mean by `regularisation` times the quadric's trace — it
    falls back to the mean where the solve is singular or would move the vertex by more than a voxel.  Triangles whose
    corners do not fall into three different clusters leave, so do repeats of a kept triangle (the lowest input index stays;
    the opposite orientation is another triangle); kept triangles stay in input order with their smallest index first, the
    vertices leave in ascending voxel order.  A referenced vertex with a non-finite coordinate, or one 2^21 voxels or more
    from the minimum, raises.  `details=True` appends dict(vertices, triangles, nonfinite, out_of_grid, collapsed,
    duplicates, fallbacks, vmap — (V,) int32 on the device: the output vertex of every input vertex, -1 for one that left).
    Bit-reproducible: equal to include/sls_simplify_math.h run on the host.  One host read (the status words)."""
    vertices = _device_points(vertices, "vertices")
    faces = _device_faces(faces, "faces")
    dev = vertices.device
    if faces.device != dev:
        raise ValueError("vertices and faces must live on the same device")
    voxel_size, code, regularisation = _simplify_args(voxel_size, contraction, regularisation)
    with torch.cuda.device(dev):
        status = _status(dev, 8)
        out_v, out_f, vmap = _simplify_launch(vertices, faces, voxel_size, code, regularisation, status)
        w = _words(status)                                          # the one host read
    _simplify_errors(w, voxel_size)
    out = (out_v[:int(w[0])], out_f[:int(w[1])])
    if details:
        d = _simplify_details(w)
        d["vmap"] = vmap
        return out + (d,)
    return out


@torch.no_grad()
def vertex_adjacency(faces: torch.Tensor, n_vertices: int, details: bool = False):
    """The edge graph of a mesh in CSR form, on the device: `(offsets (V+1,) int32, neighbours (2E,) int32, boundary (V,)
    uint8)`.  `neighbours[offsets[v]:offsets[v+1]]` are the DISTINCT vertices that share an edge of a triangle with v, in
    ascending index (a repeated triangle, the opposite orientation and a non-manifold edge add nothing twice);
    `boundary[v]` is 1 iff v is an end of an edge that exactly one triangle owns.  Triangles with a repeated index (and rows
    of -1) take no part; a face index outside [0, n_vertices) raises.  `details=True` adds dict(live, edges, boundary,
    degenerate, out_of_range, max_row).  One host read (the status words, for E)."""
    faces = _device_faces(faces, "faces")
    dev, V, T = faces.device, int(n_vertices), int(faces.shape[0])
    if V < 0:
        raise ValueError("n_vertices must be >= 0")
    lib = _abi.lib()
    with torch.cuda.device(dev):
        status = _status(dev, 8)
        offsets = torch.empty((V + 1,), dtype=torch.int32, device=dev)
        neighbours = torch.empty((6 * T,), dtype=torch.int32, device=dev)
        boundary = torch.empty((V,), dtype=torch.uint8, device=dev)
        nbytes = int(lib.sls_mesh_adjacency_scratch_bytes(V, T))
        hold, ptr = _scratch(nbytes, dev)
        _abi.check(lib.sls_mesh_adjacency(V, T, faces.data_ptr(), offsets.data_ptr(), neighbours.data_ptr(), boundary.data_ptr(),
                                          status.data_ptr(), ptr, nbytes, _stream(dev)), "sls_mesh_adjacency")
        w = _words(status)                                          # the one host read
    if w[5]:
        raise _range_error(int(w[5]))
    out = (offsets, neighbours[:2 * int(w[1])], boundary)
    if details:
        d = _smooth_details(w)
        del d["nonfinite"]                                          # (the call sees no positions)
        return out + (d,)
    return out


@torch.no_grad()
def smooth(vertices: torch.Tensor, faces: torch.Tensor, iterations: int, method: str = "taubin", weights: str = "inverse_distance",
           lambda_: float = 0.5, mu: float = -0.53, fix_boundary: bool = False, details: bool = False):
    """The vertices (V,3) float32 after `iterations` smoothing sweeps over the edge graph; the faces stay as they are.
    `method="laplacian"`: every sweep moves a vertex by `lambda_` times the way to the weighted mean of its neighbours
    (Open3D's `filter_smooth_laplacian`); `"taubin"`: a sweep with `lambda_`, then one with `mu` (negative: it undoes the
    shrinkage; `filter_smooth_taubin`); `"simple"`: the mean of the vertex and its neighbours (`filter_smooth_simple`,
    `weights` is not used).  `weights="inverse_distance"` weighs a neighbour by 1 / (distance + 1e-12), `"uniform"` by 1.
    The neighbours are those of `vertex_adjacency`, the same for all sweeps; a vertex without one is copied bit for bit, and
    with `fix_boundary` so is every boundary vertex.  A referenced vertex with a non-finite coordinate raises, so does a face
    index outside the vertices.  `details=True` appends dict(live, edges, boundary, nonfinite, degenerate, out_of_range,
    max_row).  Bit-reproducible (float64 sums in a fixed order, no atomics): equal to include/sls_smooth_math.h run on the
    host.  One host read (the status words)."""
    vertices = _device_points(vertices, "vertices")
    faces = _device_faces(faces, "faces")
    dev = vertices.device
    if faces.device != dev:
        raise ValueError("vertices and faces must live on the same device")
    iterations, method, weights, lambda_, mu = _smooth_args(iterations, method, weights, lambda_, mu)
    with torch.cuda.device(dev):
        status = _status(dev, 8)
        out = _smooth_launch(vertices, faces, iterations, method, weights, lambda_, mu, fix_boundary, status)
        w = _words(status)                                          # the one host read
    _smooth_errors(w)
    return (out, _smooth_details(w)) if details else out


@torch.no_grad()
def boundary_loops(faces: torch.Tensor, n_vertices: int, details: bool = False):
    """The boundary of a mesh, on the device: `(halfedges (B,2) int32, loop (B,) int32, loop_edges (L,) int32)`.  A half-edge
    a -> b of a triangle is a boundary half-edge iff exactly one triangle owns the undirected edge; they are listed in
    ascending (a, b).  A vertex that exactly one of them leaves and exactly one enters is simple; chains through simple
    vertices alone close into loops, numbered in ascending order of their lowest vertex: `loop[h]` is the loop of half-edge
    h, -1 for an open one (a chain that touches a pinched vertex, a fin or a flipped triangle), `loop_edges[k]` the
    half-edges of loop k.  Triangles with a repeated index (and rows of -1) take no part; a face index outside
    [0, n_vertices) raises.  `details=True` adds dict(halfedges, loops, open_halfedges, complex_vertices, degenerate,
    out_of_range).  One host read (the status words)."""
    faces = _device_faces(faces, "faces")
    dev, V, T = faces.device, int(n_vertices), int(faces.shape[0])
    if V < 0:
        raise ValueError("n_vertices must be >= 0")
    lib = _abi.lib()
    with torch.cuda.device(dev):
        status = _status(dev, 16)
        halfedges = torch.empty((3 * T, 2), dtype=torch.int32, device=dev)
        loop = torch.empty((3 * T,), dtype=torch.int32, device=dev)
        loop_edges = torch.empty((T,), dtype=torch.int32, device=dev)
        nbytes = int(lib.sls_mesh_boundary_loops_scratch_bytes(V, T))
        hold, ptr = _scratch(nbytes, dev)
        _abi.check(lib.sls_mesh_boundary_loops(V, T, faces.data_ptr(), None, halfedges.data_ptr(), loop.data_ptr(), loop_edges.data_ptr(),
                                               status.data_ptr(), ptr if nbytes else None, nbytes, _stream(dev)), "sls_mesh_boundary_loops")
        w = _words(status)                                          # the one host read
    if w[11]:
        raise _range_error(int(w[11]))
    B, L = int(w[2]), int(w[3])
    out = (halfedges[:B], loop[:B], loop_edges[:L])
    if details:
        d = _fill_details(w)
        return out + ({k: d[k] for k in ("halfedges", "loops", "open_halfedges", "complex_vertices", "degenerate", "out_of_range")},)
    return out


@torch.no_grad()
def fill_holes(vertices: torch.Tensor, faces: torch.Tensor, max_edges: int = 64, max_size: float = None, capacity: float = 0.25,
               details: bool = False):
    """The mesh with its small holes closed: `(vertices (V',3), faces (T',3) int32)`.  Every loop of `boundary_loops` with at
    most `max_edges` half-edges, finite vertices and (with `max_size`) an axis-aligned bounding box whose diagonal is at most
    `max_size` is filled: a loop of three by one triangle, a longer one by a fan over a new vertex at the float64 mean of its
    vertices, oriented like the triangles along the rim.  The input vertices and faces come first, unchanged; the new ones
    follow in loop order.  It is a fan over a centroid and nothing more — no refinement, no fairing: a long or strongly
    non-planar rim can fold the fan over itself, which is what the two limits are for (`smooth` afterwards evens out the
    fans); open chains at complex vertices stay open.  The default of 64 edges is a judgement, not a measurement.
    `capacity` is the room for new triangles as a share of T (at least 64 triangles); where it does not suffice the call
    raises ValueError and names the triangles and vertices needed.  A face index outside the vertices raises.
    `details=True` appends dict(vertices, triangles, halfedges, loops, filled, skipped_edges, skipped_size,
    skipped_nonfinite, open_halfedges, complex_vertices, degenerate, out_of_range, needed_vertices, needed_triangles,
    overflow).  Bit-reproducible (float64 sums in a fixed order, no float atomics): equal to include/sls_fill_math.h run on
    the host.  One host read (the status words)."""
    vertices = _device_points(vertices, "vertices")
    faces = _device_faces(faces, "faces")
    dev = vertices.device
    if faces.device != dev:
        raise ValueError("vertices and faces must live on the same device")
    max_edges, max_size, capacity = _fill_args(max_edges, max_size, capacity)
    with torch.cuda.device(dev):
        status = _status(dev, 16)
        out_v, out_f = _fill_launch(vertices, faces, None, max_edges, max_size, capacity, status)
        w = _words(status)                                          # the one host read
    if w[11]:
        raise _range_error(int(w[11]))
    _fill_errors(w)
    out = (out_v[:int(w[0])], out_f[:int(w[1])])
    return out + (_fill_details(w),) if details else out


@torch.no_grad()
def clean_mesh(vertices: torch.Tensor, faces: torch.Tensor, *, weld: bool = True, keep_clusters: int = 1, min_triangles: int = 50,
               normals: bool = True, details: bool = False, simplify: float = None, contraction: str = "average",
               regularisation: float = 1e-3, smooth: int = None, smooth_method: str = "taubin",
               smooth_weights: str = "inverse_distance", smooth_lambda: float = 0.5, smooth_mu: float = -0.53,
               fix_boundary: bool = False, fill_holes: int = None, fill_max_size: float = None, fill_capacity: float = 0.25):
    """Weld, keep the largest clusters, optionally fill holes, simplify and smooth, compute vertex normals: `(vertices, faces)` or, with `normals`,
    `(vertices, faces, normals)`; `details=True` appends the dict of `keep_clusters` (the statistics are those of the
    welded mesh before the selection) plus `welded_vertices`.  `simplify=h` runs `simplify_vertex_clustering(h, contraction,
    regularisation)` after the selection and before the normals (`details` then holds its dict under "simplify", with `vmap`
    over the vertices at the selection's capacity); `simplify=None`: no such stage.  `smooth=n` runs `smooth(n, smooth_method,
    smooth_weights, smooth_lambda, smooth_mu, fix_boundary)` after the simplification and before the normals (`details` then
    holds its dict under "smooth"); `smooth=None`: no such stage.  `fill_holes=n` runs `fill_holes(max_edges=n, fill_max_size,
    fill_capacity)` after the selection and before the simplification: its live counts are the device words of the earlier
    stages, the later stages run at its capacity, `details` holds its dict under "fill", and too little room raises
    ValueError; `fill_holes=None`: no such stage.  `weld=True` merges the bit-equal rows of `vertices` and passes the faces
    through their ranks: for a soup (`faces` = arange) that is `weld`.  `keep_clusters=None`: no selection.  One host read for
    the whole chain: every stage runs at the capacity of its input (vertices beyond the welded count are referenced by
    nothing, face rows beyond the kept count are -1 and skipped), and the outputs are sliced at the end."""
    vertices = _device_points(vertices, "vertices")
    faces = _device_faces(faces, "faces")
    dev = vertices.device
    if faces.device != dev:
        raise ValueError("vertices and faces must live on the same device")
    T = int(faces.shape[0])
    select = keep_clusters is not None
    if simplify is not None:
        simplify, code, regularisation = _simplify_args(simplify, contraction, regularisation)
    if smooth is not None:
        smooth, s_method, s_weights, smooth_lambda, smooth_mu = _smooth_args(smooth, smooth_method, smooth_weights, smooth_lambda, smooth_mu)
    if fill_holes is not None:
        fill_holes, fill_max_size, fill_capacity = _fill_args(fill_holes, fill_max_size, fill_capacity)
    with torch.cuda.device(dev):
        status = _status(dev, 56)
        status[0] = int(vertices.shape[0])                          # (without a weld: V as it came)
        v, f = vertices, faces
        if weld:
            V = int(vertices.shape[0])
            v, index = _weld_launch(vertices, status[0:4])
            # the faces through the rank of every row (a gather: plumbing); a triangle with an index outside the vertices
            # keeps one (-1) and is counted by the cluster stage
            inside = ((faces >= 0) & (faces < V)).all(dim=1, keepdim=True)
            f = torch.where(inside, index[faces.clamp(0, max(V - 1, 0)).long()], torch.full_like(faces, -1)) if V else \
                torch.full_like(faces, -1)
        labels, counts = _clusters_launch(f, int(v.shape[0]), status[8:16])
        if select:
            v, f = _filter_launch(v, f, labels, counts, status[8:16], keep_clusters, min_triangles, status[16:20])
        if fill_holes is not None:
            if select:
                live = status[16:18]                                # [V', T'] of the selection, on the device
            else:
                live = torch.stack([status[0], torch.tensor(T, dtype=torch.int32, device=dev)])
            v, f = _fill_launch(v, f, live, fill_holes, fill_max_size, fill_capacity, status[40:56])
        if simplify is not None:
            v, f, vmap = _simplify_launch(v, f, simplify, code, regularisation, status[24:32])
        if smooth is not None:
            v = _smooth_launch(v, f, smooth, s_method, s_weights, smooth_lambda, smooth_mu, fix_boundary, status[32:40])
        n = _normals_launch(v, f) if normals else None
        w = _words(status)                                          # the one host read
    if w[10]:
        raise _range_error(int(w[10]))
    nv, nt = (int(w[16]), int(w[17])) if select else (int(w[0]), T)
    if fill_holes is not None:
        _fill_errors(w[40:])
        nv, nt = int(w[40]), int(w[41])
    if simplify is not None:
        _simplify_errors(w[24:], simplify)
        nv, nt = int(w[24]), int(w[25])
    if smooth is not None:
        _smooth_errors(w[32:], ranges=False)                        # (rows of -1 beyond the kept triangles are no error here)
    out = (v[:nv], f[:nt]) + ((n[:nv],) if normals else ())
    if details:
        d = _cluster_details(w[8:])
        d.update(cluster_count=counts[:int(w[8])], labels=labels, n_min=int(w[18]) if select else 0, welded_vertices=int(w[0]))
        if simplify is not None:
            d["simplify"] = dict(_simplify_details(w[24:]), vmap=vmap)
        if smooth is not None:
            d["smooth"] = _smooth_details(w[32:])
        if fill_holes is not None:
            d["fill"] = _fill_details(w[40:])
        return out + (d,)
    return out
