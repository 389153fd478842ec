"""include/sls_simplify_math.h compiled for the host against the NumPy restatement of tests/simplify_ref.py (no device
needed): faces, vertex map and status words equal; the average positions bit-equal on the lattice cases and within 1e-5 h
elsewhere; the quadric positions bit-equal (NumPy float64 and Python floats round every operation once, as the header
does); what the quadric buys on the cube; the properties every output has."""
import numpy as np
import pytest

import mesh_ref
import simplify_ref as ref
from mesh_ref import bits

CASES = ref.cases()
SPHERE = {"vertices": 1706, "triangles": 3408, "duplicates": 0, "fallbacks": 0, "closed": True}      # the restatement's answer


@pytest.fixture(scope="module")
def host():
    return ref.host()


@pytest.mark.parametrize("contraction", (ref.AVERAGE, ref.QUADRIC))
@pytest.mark.parametrize("case", sorted(CASES))
def test_header_equals_restatement(host, case, contraction):
    v, f, h = CASES[case]
    want_v, want_f, want_m, stats = ref.simplify(v, f, h, contraction)
    got_v, got_f, got_m, status = host.simplify(v, f, h, contraction)
    assert status == ref.status_words(stats), case
    assert np.array_equal(got_f, want_f) and np.array_equal(got_m, want_m)
    if contraction == ref.QUADRIC or ref.LATTICE(case):
        assert np.array_equal(bits(got_v), bits(want_v))
    elif len(want_v):
        assert np.abs(got_v.astype(np.float64) - want_v.astype(np.float64)).max() <= 1e-5 * h
    if contraction == ref.AVERAGE:
        assert stats["fallbacks"] == 0


def test_hand_case_counts():
    """what every hand case is there for, from the restatement"""
    want = {"collapse": dict(collapsed=2), "duplicates": dict(duplicates=2, collapsed=0), "bad_indices": dict(degenerate=4, vertices=16),
            "nonfinite": dict(nonfinite=2, degenerate=4), "vanish": dict(collapsed=3, vertices=16), "zero_area": dict(fallbacks=3, collapsed=1),
            "empty": dict(vertices=0, triangles=0), "one_voxel": dict(vertices=0, triangles=0, collapsed=18)}
    for case, words in want.items():
        v, f, h = CASES[case]
        out_v, out_f, vmap, stats = ref.simplify(v, f, h, ref.QUADRIC)
        assert {k: stats[k] for k in words} == words, (case, stats)
    v, f, h = CASES["duplicates"]                                   # the lower index stays; the opposite orientation stays
    out_v, out_f, vmap, _ = ref.simplify(v, f, h)
    rows = [tuple(r) for r in out_f.tolist()]
    a, b, c = sorted(vmap[[0, 1, 5]])
    assert rows[0] == (a, b, c) and rows.count((a, b, c)) == 1 and rows.count((a, c, b)) == 1 and len(out_f) == len(f) - 2
    v, f, h = CASES["bad_indices"]                                  # the far vertices moved no bounding box: the sheet as it is
    out_v, _, vmap, _ = ref.simplify(v, f, h)
    assert vmap[16] == -1 and vmap[17] == -1 and np.array_equal(np.sort(vmap[:16]), np.arange(16))
    v, f, h = CASES["vanish"]
    assert (ref.simplify(v, f, h)[2][16:] == -1).all()
    v, f, h = CASES["nonfinite"]
    assert (ref.simplify(v, f, h)[2][16:] == -1).all()


def test_out_of_grid_is_counted(host):
    v, f, h = ref.big_case()
    assert ref.simplify(v, f, h)[3]["out_of_grid"] == 2 and host.simplify(v, f, h)[3][3] == 2
    assert host.simplify(v, f, h, ref.QUADRIC)[3][2:4] == [0, 2]


def test_identity_voxel_keeps_every_live_vertex(host):
    """voxel_size = 1/32 on the lattice strip: every vertex is its own cluster — the vertices in key order, bit-equal, the
    faces only rotated"""
    v, f, h = CASES["strip_identity"]
    out_v, out_f, vmap, status = host.simplify(v, f, h)
    assert status == [len(v), len(f), 0, 0, 0, 0, 0, 1] and np.array_equal(np.sort(vmap), np.arange(len(v)))
    assert np.array_equal(bits(out_v[vmap]), bits(v))
    key = (v.astype(np.float64) - (v.min(0).astype(np.float64) - 0.5 * h)) // h
    assert np.array_equal(np.lexsort((key[:, 0], key[:, 1], key[:, 2])), np.argsort(vmap))
    assert np.array_equal(out_f, ref.rotate(vmap[f]))


@pytest.mark.parametrize("h", (1.0 / 6.0, 0.21, 0.5))
def test_cube_quadric_keeps_edges_and_corners(host, h):
    v, f = ref.cube()
    assert len(f) == 6912
    sharp, _, _, status = host.simplify(v, f, h, ref.QUADRIC, 1e-6)
    mean, _, _, _ = host.simplify(v, f, h, ref.AVERAGE)
    d_sharp, d_mean = ref.cube_distance(sharp).max() / h, ref.cube_distance(mean).max() / h
    print(f"cube h = {h:.3f}: worst distance from the surface {d_sharp:.3e} h (quadric, lambda 1e-6), {d_mean:.3f} h (average)")
    assert status[6] == 0 and len(sharp) == len(mean)
    assert d_sharp <= 1e-5                                          # the project's float bar
    assert d_mean > 0.1                                             # what the quadric buys


def test_sphere_counts(host):
    v, f = ref.sphere()
    assert len(f) == 36480
    for contraction in (ref.AVERAGE, ref.QUADRIC):
        out_v, out_f, _, status = host.simplify(v, f, 0.1, contraction)
        assert status[:2] == [SPHERE["vertices"], SPHERE["triangles"]] and status[5] == SPHERE["duplicates"] and status[6] == SPHERE["fallbacks"]
    edges = mesh_ref.clusters(out_f, len(out_v))[2]
    assert (edges["boundary_edges"] == 0 and edges["nonmanifold_edges"] == 0) == SPHERE["closed"] and mesh_ref.euler(out_f) == 2


@pytest.mark.parametrize("case", sorted(CASES))
def test_properties(host, case):
    v, f, h = CASES[case]
    out_v, out_f, vmap, status = host.simplify(v, f, h, ref.QUADRIC)
    nv, nt = status[0], status[1]
    degenerate = ref.simplify(v, f, h)[3]["degenerate"]
    assert len(f) == nt + status[4] + status[5] + degenerate        # the counts add up
    if nt:
        assert out_f.min() >= 0 and out_f.max() < nv and (out_f[:, 0] < out_f[:, 1]).all() and (out_f[:, 0] < out_f[:, 2]).all()
        assert (out_f[:, 1] != out_f[:, 2]).all()
        assert len(np.unique(out_f, axis=0)) == nt                  # no two kept faces are equal
        assert np.array_equal(np.unique(out_f), np.arange(nv))      # every output vertex is referenced
    assert vmap.min() >= -1 and vmap.max() < max(nv, 1) and (nv == 0 or set(vmap[vmap >= 0]) == set(range(nv)))
    # vmap against the faces: the kept faces are the images of input faces, in input order, without the repeats
    ok = mesh_ref.degenerate(f, len(v)) == 0
    image = vmap[np.where(ok[:, None], f, 0)]
    cand = ok & (image >= 0).all(1) & (image[:, 0] != image[:, 1]) & (image[:, 1] != image[:, 2]) & (image[:, 2] != image[:, 0])
    seen, rows = set(), []
    for row in map(tuple, ref.rotate(image[cand]).tolist() if cand.any() else []):
        if row not in seen:
            seen.add(row)
            rows.append(row)
    assert rows == [tuple(r) for r in out_f.tolist()]
    assert np.isfinite(out_v).all()
    if nv:                                                          # a vertex stays within its voxel's reach of its members
        for k in range(0, nv, max(nv // 50, 1)):
            assert np.abs(v[vmap == k].astype(np.float64) - out_v[k]).max() <= 2 * h
