"""include/sls_mesh_math.h run on the host (mesh_ref.host()) against its NumPy / pure-Python restatement (mesh_ref): weld
bit for bit, cluster labels, counts and edge statistics equal, the selection equal, float32 normals within 1e-5 of
float64 — and the figures of the marching-tetrahedra sphere.  No device needed."""
import numpy as np
import pytest

import mesh_ref as ref
from mesh_ref import bits
from tsdf_ref import CENTRE

WELD_CASES = ref.weld_cases()
CLUSTER_CASES = ref.cluster_cases()


@pytest.mark.parametrize("case", sorted(WELD_CASES))
def test_weld_header_equals_unique(case):
    rows = WELD_CASES[case]
    v, index = ref.host().weld(rows)
    want_v, want_i = ref.weld(rows)
    assert np.array_equal(bits(v), bits(want_v)) and np.array_equal(index, want_i)
    assert np.array_equal(bits(v[index]), bits(rows))                                   # every row finds itself again


def test_weld_order_is_signed_and_bitwise():
    v, _ = ref.host().weld(WELD_CASES["signed_zero"])
    assert len(v) == 5                                          # -0.0 and 0.0 stay apart, in x, y and z
    v, _ = ref.host().weld(WELD_CASES["nan_payloads"])
    assert len(v) == 5                                          # two payloads in x stay apart; the repeat of the first merges
    v, _ = ref.host().weld(WELD_CASES["negative"])
    x = v[:, 0].copy().view(np.int32)                           # signed order of the words: negative floats first, and among
    assert np.array_equal(x, np.sort(x)) and list(v[:, 0]) == [-1, -1, -3, 0.5, 1]      # them the smaller magnitude first
    v, _ = ref.host().weld(WELD_CASES["pass_order"])
    assert [tuple(r) for r in v.astype(int)] == sorted({tuple(r) for r in WELD_CASES["pass_order"].astype(int)})


@pytest.mark.parametrize("case", sorted(CLUSTER_CASES))
def test_clusters_header_equals_walk(case):
    faces, V = CLUSTER_CASES[case]
    labels, counts, stats = ref.host().clusters(faces, V)
    want_l, want_c, want_s = ref.clusters(faces, V)
    assert np.array_equal(labels, want_l) and np.array_equal(counts, want_c) and stats == want_s


def test_cluster_figures():
    c = {k: ref.clusters(*v) for k, v in CLUSTER_CASES.items() if k != "scene"}
    assert c["two_tets"][2]["clusters"] == 2 and list(c["two_tets"][1]) == [4, 4] and c["two_tets"][2]["boundary_edges"] == 0
    assert c["strip"][2]["clusters"] == 1 and c["strip"][1][0] == 4096
    assert c["fan"][2] == {"clusters": 1, "degenerate": 0, "out_of_range": 0, "boundary_edges": 6, "nonmanifold_edges": 1}
    assert list(c["degenerate"][0]) == [0, -1, 0, -1, -1, -1, 1] and c["degenerate"][2]["degenerate"] == 4
    assert c["degenerate"][2]["out_of_range"] == 2
    assert list(c["isolated"][0]) == [0] and c["isolated"][2]["boundary_edges"] == 3
    assert c["empty"][2]["clusters"] == 0
    labels, counts, stats = ref.clusters(*CLUSTER_CASES["scene"])
    assert stats["clusters"] == 7 and list(counts[2:]) == [1] * 5 and counts[0] == 7152 and counts[0] > counts[1] > 50
    assert list(labels[-5:]) == [2, 3, 4, 5, 6] and stats["boundary_edges"] == 15 and stats["nonmanifold_edges"] == 0


SELECTIONS = [(1, 50), (2, 50), (100, 2), (0, 50), (1, 0), (0, 0), (3, 0), (-1, -1)]


@pytest.mark.parametrize("keep,floor", SELECTIONS)
def test_selection_header_equals_rule(keep, floor):
    v, f = ref.floater_scene()
    got_v, got_f, got_n = ref.host().select(v, f, keep, floor)
    want_v, want_f, want_n = ref.select(v, f, keep, floor)
    assert got_n == want_n and np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_f, want_f)


def test_selection_figures():
    v, f = ref.floater_scene()
    _, counts, _ = ref.clusters(f, len(v))
    big, small = int(counts[0]), int(counts[1])
    assert ref.n_min(counts, 1, 50) == big and ref.n_min(counts, 2, 50) == small and ref.n_min(counts, 100, 2) == 2
    assert ref.n_min(counts, 0, 50) == 50 and ref.n_min(counts, 1, 0) == big and ref.n_min(counts, 0, 0) == 0
    assert ref.n_min(counts, 3, 0) == 1                         # the third largest is a floater: ties at 1 keep all five
    assert len(ref.select(v, f, 1, 50)[1]) == big and len(ref.select(v, f, 2, 50)[1]) == big + small
    assert len(ref.select(v, f, 100, 2)[1]) == big + small and len(ref.select(v, f, 3, 0)[1]) == len(f)
    faces, V = ref.TWO_TETS                                     # two equal-sized clusters at the threshold: both stay
    assert len(ref.select(np.zeros((V, 3), np.float32), faces, 1, 0)[1]) == 8


def test_normals_header_within_1e5_of_float64():
    for v, f in (ref.floater_scene(), (np.random.default_rng(2).normal(0, 1, (7, 3)).astype(np.float32), ref.DEGENERATE[0])):
        got = ref.host().normals(v, f)
        want, _ = ref.normals64(v, f)
        assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= 1e-5


def test_normals_zero_rules():
    # vertices 3, 4, 5 are referenced by nothing; the two triangles of vertex 0 cancel exactly
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [5, 5, 5], [0, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1], [6, 1, 2]], np.int32)               # vertex 0: n and -n; vertex 6: one triangle
    got = ref.host().normals(v, f)
    assert np.array_equal(bits(got[0]), bits(np.zeros(3))) and np.array_equal(bits(got[5]), bits(np.zeros(3)))
    assert np.array_equal(got[6], [0, 0, 1]) and np.array_equal(bits(got[3]), bits(np.zeros(3)))
    big = np.array([[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0]], np.float32)    # the cross product overflows: a non-finite sum
    assert np.array_equal(bits(ref.host().normals(big, np.array([[0, 1, 2]], np.int32))), bits(np.zeros((3, 3))))


def test_sphere_figures():
    soup = ref.sphere_soup()
    assert soup.shape == (21456, 3)                             # 7152 triangles
    v, index = ref.host().weld(soup)
    f = index.reshape(-1, 3)
    assert len(v) == 3578
    labels, counts, stats = ref.host().clusters(f, len(v))
    assert stats == {"clusters": 1, "degenerate": 0, "out_of_range": 0, "boundary_edges": 0, "nonmanifold_edges": 0}
    assert list(counts) == [7152] and (labels == 0).all()
    assert ref.euler(f) == 2
    n32 = ref.host().normals(v, f)
    n64, conditioning = ref.normals64(v, f)
    radial = v.astype(np.float64) - CENTRE
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (n32.astype(np.float64) * radial).sum(1)
    print("sphere: min dot %.4f, |n32 - n64| max %.2e, worst conditioning %.4f" % (dots.min(), np.abs(n32 - n64).max(), conditioning.min()))
    assert dots.min() >= 0.99                                   # every normal points outward, every vertex is compared
    assert np.abs(n32.astype(np.float64) - n64).max() <= 1e-5
