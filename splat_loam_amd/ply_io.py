"""On-disk model format of the reference: binary little-endian
PLY, one `vertex` element with float32 properties
`x y z opacity scale_0 scale_1 rot_0..rot_3 f_dc_0..f_dc_2` holding the RAW
(pre-activation) parameters (scene/gaussian_model.py:123-168; read back by
`load_ply`, :170-221, which looks properties up by name).  Written with NumPy
only (the reference uses `plyfile`, which produces the same byte layout for a
single all-float32 element), so models saved here load in the reference's
`mesh` / `eval_*` commands and vice versa.
"""
from __future__ import annotations

import os

import numpy as np

PROPS = ["x", "y", "z", "opacity", "scale_0", "scale_1", "rot_0", "rot_1", "rot_2", "rot_3",
         "f_dc_0", "f_dc_1", "f_dc_2"]
CLOUD_PROPS = ["x", "y", "z", "nx", "ny", "nz"]
COLOR_PROPS = ["red", "green", "blue"]


def save_ply(path, xyz, opacity_raw, scaling_raw, rotation_raw) -> None:
    def host(a):      # NumPy, or tensors on any device (the reference saves `.detach().cpu().numpy()`, gaussian_model.py:133-141)
        return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
    xyz, opacity_raw, scaling_raw, rotation_raw = (host(a) for a in (xyz, opacity_raw, scaling_raw, rotation_raw))
    n = xyz.shape[0]
    data = np.concatenate([xyz.reshape(n, 3), opacity_raw.reshape(n, 1), scaling_raw.reshape(n, 2),
                           rotation_raw.reshape(n, 4), np.zeros((n, 3), np.float32)], axis=1).astype("<f4")
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join(f"property float {p}\n" for p in PROPS) + "end_header\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(data.tobytes())


def _colored(rows, names, colors):
    """(vertex bytes, header lines) of float32 columns followed by `uchar red green blue` (e.g. `evaluation.error_colors`)"""
    colors = np.asarray(colors.detach().cpu().numpy() if hasattr(colors, "detach") else colors)
    if colors.dtype != np.uint8 or colors.shape != (len(rows), 3):
        raise ValueError("colors must be uint8 of shape (rows, 3)")
    rec = np.empty(len(rows), np.dtype([(p, "<f4") for p in names] + [(c, "u1") for c in COLOR_PROPS]))
    for k, p in enumerate(names):
        rec[p] = rows[:, k]
    for k, c in enumerate(COLOR_PROPS):
        rec[c] = colors[:, k]
    return rec.tobytes(), "".join(f"property float {p}\n" for p in names) + "".join(f"property uchar {c}\n" for c in COLOR_PROPS)


def save_point_cloud(path, points, normals, colors=None) -> None:
    """An oriented point cloud (`meshing.sample_surface`) as binary little-endian PLY: one `vertex` element with float32
    `x y z nx ny nz`, the property names Open3D's `read_point_cloud` looks up — the input of Poisson reconstruction.
    `colors` (N,3) uint8: the element gains `uchar red green blue`; without them the bytes are the same as ever."""
    def host(a):
        return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
    points, normals = host(points).reshape(-1, 3), host(normals).reshape(-1, 3)
    if points.shape != normals.shape:
        raise ValueError("points and normals must have the same number of rows")
    n = points.shape[0]
    data = np.concatenate([points, normals], axis=1).astype("<f4")
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    if colors is None:
        body, props = data.tobytes(), "".join(f"property float {p}\n" for p in CLOUD_PROPS)
    else:
        body, props = _colored(data, CLOUD_PROPS, colors)
    header += props + "end_header\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(body)


def save_mesh(path, vertices, faces, normals=None, colors=None) -> None:
    """A triangle mesh (`tsdf.TsdfVolume.extract`, `meshing.mesh_tsdf`) as binary little-endian PLY: a `vertex` element
    with float32 `x y z`, then a `face` element with `list uchar int vertex_indices` — what `load_mesh` reads back bit for
    bit, and the layout Open3D and MeshLab write for a plain triangle mesh.  `normals` (V,3), e.g. of
    `mesh_ops.vertex_normals`: the vertex element gains float32 `nx ny nz` (`load_point_cloud` returns them; `load_mesh`
    skips them); without them the bytes are the same as ever.  `colors` (V,3) uint8, e.g. of `evaluation.error_colors`:
    the vertex element gains `uchar red green blue` behind the floats (what MeshLab and Open3D show as vertex colours);
    without them, again, the same bytes."""
    def host(a, dt):
        return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=dt)
    vertices, faces = host(vertices, np.float32).reshape(-1, 3), host(faces, np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() > 0x7FFFFFFF):
        raise ValueError("a vertex index does not fit int32")
    props = "xyz"
    if normals is not None:
        normals = host(normals, np.float32).reshape(-1, 3)
        if normals.shape != vertices.shape:
            raise ValueError("vertices and normals must have the same number of rows")
        vertices, props = np.concatenate([vertices, normals], axis=1), ("x", "y", "z", "nx", "ny", "nz")
    rec = np.empty(len(faces), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, faces
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(vertices)
    if colors is None:
        body, lines = vertices.astype("<f4").tobytes(), "".join(f"property float {p}\n" for p in props)
    else:
        body, lines = _colored(vertices, list(props), colors)
    header += lines
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(body)
        f.write(rec.tobytes())


_KINDS = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1",
          "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "short": "<i2", "int16": "<i2", "ushort": "<u2",
          "uint16": "<u2", "char": "i1", "int8": "i1"}


def _parse_header(path):
    """(file bytes, offset of the data, [[element, count, [(property, dtype | None for a list, header tokens)]]])"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    if lines[0] != "ply" or "binary_little_endian" not in lines[1]:
        raise ValueError("only binary little-endian PLY is supported")
    elements = []                                   # in file order
    for ln in lines:
        tok = ln.split()
        if tok[:1] == ["element"]:
            elements.append([tok[1], int(tok[2]), []])
        elif tok[:1] == ["property"] and elements:
            if tok[1] == "list":
                elements[-1][2].append((tok[-1], None, tok))
            else:
                elements[-1][2].append((tok[2], _KINDS[tok[1]], tok))
    return blob, end, elements


def _read_vertices(path):
    """The `vertex` element of a binary little-endian PLY as a structured array, and its property names in file order.
    Elements in front of it must be free of list properties (their size is not known from the header otherwise)."""
    blob, offset, elements = _parse_header(path)
    for name, count, props in elements:
        if name == "vertex":
            if any(kind is None for _, kind, _ in props):
                raise ValueError("list properties on the vertex element are not supported")
            rec = np.frombuffer(blob, dtype=np.dtype([(p, k) for p, k, _ in props]), count=count, offset=offset)
            return rec, [p for p, _, _ in props]
        if any(kind is None for _, kind, _ in props):
            raise ValueError(f"element {name} with list properties comes before the vertices")
        offset += count * np.dtype([(p, k) for p, k, _ in props]).itemsize
    raise ValueError("no vertex element")


def load_ply(path) -> dict:
    """dict(xyz (N,3), opacity (N,1), scaling (N,S), rotation (N,4)) of raw parameters; properties are
    looked up by name like the reference does, so extra/reordered float properties are tolerated."""
    rec, names = _read_vertices(path)
    col = lambda name: np.asarray(rec[name], dtype=np.float32)
    scale_names = sorted([p for p in names if p.startswith("scale_")], key=lambda s: int(s.split("_")[-1]))
    rot_names = sorted([p for p in names if p.startswith("rot")], key=lambda s: int(s.split("_")[-1]))
    return dict(xyz=np.stack([col("x"), col("y"), col("z")], 1), opacity=col("opacity")[:, None],
                scaling=np.stack([col(s) for s in scale_names], 1), rotation=np.stack([col(s) for s in rot_names], 1))


def _colors(rec, names):
    """(N,3) uint8 of `red green blue` where the vertex element has all three as uchar, else None"""
    if all(c in names and rec.dtype[c] == np.uint8 for c in COLOR_PROPS):
        return np.stack([np.asarray(rec[c]) for c in COLOR_PROPS], 1)
    return None


def load_point_cloud(path, return_colors: bool = False):
    """`(points (N,3) float32, normals (N,3) float32 | None)` of a binary little-endian PLY point cloud: `x y z` as float
    or double (scan exports often store doubles; they are rounded to float32 once), `nx ny nz` where the file has all
    three.  Reads what `save_point_cloud` writes; other vertex properties and the elements behind the vertices (faces)
    are ignored.  `return_colors=True`: a third item, `uchar red green blue` as (N,3) uint8, or None without them."""
    rec, names = _read_vertices(path)
    for p in ("x", "y", "z"):
        if p not in names:
            raise ValueError(f"{path}: the vertex element has no property {p}")
        if rec.dtype[p].kind != "f":
            raise ValueError(f"{path}: property {p} is not float or double")
    col = lambda name: np.asarray(rec[name], dtype=np.float32)
    points = np.stack([col("x"), col("y"), col("z")], 1)
    normals = np.stack([col("nx"), col("ny"), col("nz")], 1) if all(p in names for p in ("nx", "ny", "nz")) else None
    return (points, normals, _colors(rec, names)) if return_colors else (points, normals)


def _xyz(path, rec, names):
    for p in ("x", "y", "z"):
        if p not in names:
            raise ValueError(f"{path}: the vertex element has no property {p}")
        if rec.dtype[p].kind != "f":
            raise ValueError(f"{path}: property {p} is not float or double")
    return np.stack([np.asarray(rec[p], dtype=np.float32) for p in ("x", "y", "z")], 1)


def load_mesh(path, return_colors: bool = False):
    """`(vertices (V,3) float32, faces (F,3) int32)` of a binary little-endian PLY triangle mesh, as Open3D writes one
    (a Poisson reconstruction): a `vertex` element with `x y z` as float or double (other vertex properties are
    skipped), then one `face` element whose only property is `list uchar int|uint vertex_indices` (or `vertex_index`).
    Every face must be a triangle; an ASCII or big-endian file, a face with another vertex count or a face element with
    further properties is refused with a ValueError.  Indices are not range-checked here (sls_mesh_sample counts the
    faces that point outside the vertices); a uint index above 2^31 - 1 is refused.  `return_colors=True`: a third item,
    the vertices' `uchar red green blue` as (V,3) uint8, or None without them."""
    blob, offset, elements = _parse_header(path)
    vertices = faces = colors = None
    for name, count, props in elements:
        lists = [tok for _, kind, tok in props if kind is None]
        if name == "face":
            if len(props) != 1 or len(lists) != 1:
                raise ValueError(f"{path}: the face element must hold exactly one list property")
            tok = lists[0]
            if len(tok) != 5 or tok[2] not in ("uchar", "uint8") or _KINDS.get(tok[3]) not in ("<i4", "<u4") or \
                    tok[4] not in ("vertex_indices", "vertex_index"):
                raise ValueError(f"{path}: unsupported face property `{' '.join(tok)}` (want list uchar int|uint vertex_indices)")
            rec_t = np.dtype([("n", "u1"), ("i", _KINDS[tok[3]], (3,))])
            if len(blob) - offset < count * rec_t.itemsize:
                raise ValueError(f"{path}: the face data is shorter than {count} triangles")
            rec = np.frombuffer(blob, dtype=rec_t, count=count, offset=offset)
            if count and not np.all(rec["n"] == 3):       # (a quad shifts every later record: the counts stop being 3)
                raise ValueError(f"{path}: only triangle meshes are supported (a face is not a triangle)")
            idx = rec["i"]
            if idx.dtype.kind == "u" and count and int(idx.max()) > 0x7FFFFFFF:
                raise ValueError(f"{path}: a vertex index does not fit int32")
            faces = np.ascontiguousarray(idx.astype(np.int32)).reshape(-1, 3)
            break                                           # (what follows the faces is not needed)
        if lists:
            raise ValueError(f"{path}: element {name} with list properties comes before the faces")
        rec_t = np.dtype([(p, k) for p, k, _ in props])
        if name == "vertex":
            vrec = np.frombuffer(blob, dtype=rec_t, count=count, offset=offset)
            vertices = _xyz(path, vrec, [p for p, _, _ in props])
            colors = _colors(vrec, [p for p, _, _ in props])
        offset += count * rec_t.itemsize
    if vertices is None:
        raise ValueError(f"{path}: no vertex element in front of the faces")
    if faces is None:
        raise ValueError(f"{path}: no face element")
    return (vertices, faces, colors) if return_colors else (vertices, faces)
