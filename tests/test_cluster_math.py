"""include/sls_cluster_math.h on the host, as plain C99 — the rule functions the kernels run and the serial all-pairs routine
— against the NumPy restatement (cluster_ref.py) on lattice clouds, array_equal throughout, and the rule cases worked by
hand: the saturation boundary at exactly eps, duplicates, min_points = 1 and beyond M, the bridge between two blobs, the
border of lower index than every core, and the selection rule."""
import numpy as np
import pytest

import cluster_ref as ref


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = ref.build_host(tmp_path_factory.mktemp("cluster_math"))
    if path is None:
        pytest.skip("no gcc")
    return path


def both(exe, tmp_path, pts, eps, min_points, keep=1, floor=0, what=""):
    want = ref.dbscan(pts, eps, min_points)
    got = ref.run_host(exe, tmp_path, pts, eps, min_points, keep, floor)
    assert got["rc"] == 0
    for key in ("status", "labels", "counts"):
        assert np.array_equal(got[key], want[key]), f"{what}: {key} differ: {got[key][:20]} {want[key][:20]}"
    index, sel = ref.select(want["labels"], want["counts"], keep, floor)
    assert np.array_equal(got["index"], index) and np.array_equal(got["select_status"], sel), f"{what}: selection differs"
    return want


@pytest.mark.parametrize("M", [0, 1, 2, 31, 33, 65, 257, 1000, 3000])
def test_header_equals_the_restatement(exe, tmp_path, M):
    pts = ref.lattice_cloud(M, M)
    for eps, mp, keep, floor in ((0.25, 4, 1, 0), (0.5, 10, 3, 0), (0.5, 1, 0, 5), (0.25, 2, 2, 40), (1.0, 100, 1, 0), (0.5, M + 1, 1, 0)):
        want = both(exe, tmp_path, pts, eps, mp, keep, floor, f"M={M} eps={eps} min_points={mp}")
        if mp == 1:                                                            # the components of the eps-graph
            assert want["status"][1] == M and want["status"][2] == 0 and want["status"][3] == 0
        if mp == M + 1:                                                        # more than the cloud holds: all noise
            assert want["status"][:5].tolist() == [0, 0, 0, M, 0] and np.all(want["labels"] == -1)
    if M >= 1000:
        assert want is not None and both(exe, tmp_path, pts, 0.5, 10)["status"][0] > 1


def test_saturation_boundary_at_exactly_eps(exe, tmp_path):
    """Neighbour counts of min_points - 1, min_points and min_points + 1, every neighbour AT distance eps or a copy: <= is
    inside, and a count that stops at min_points says the same as the full count."""
    for mp in (3, 10, 40, 100):
        pts, centres = ref.saturation_cloud(mp)
        want = both(exe, tmp_path, pts, 0.25, mp, what=f"saturation {mp}")
        assert want["core"][centres].tolist() == [False, True, True]
        assert want["status"][0] == 2 and want["counts"].tolist() == [mp, mp + 1]
        assert np.all(want["labels"][:centres[1]] == -1)                       # the first star: no core, so noise
        # just inside the radius nothing of this changes; just below it the arms are lost
        assert ref.run_host(exe, tmp_path, pts, 0.2500001, mp)["status"].tolist() == want["status"].tolist()
        assert ref.run_host(exe, tmp_path, pts, 0.2499999, mp)["status"][0] == 0


def test_duplicates(exe, tmp_path):
    pts = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (40, 1))
    want = both(exe, tmp_path, pts, 0.0625, 40, what="copies")
    assert want["status"].tolist() == [1, 40, 0, 0, 40, 40, 0, 1] and not want["labels"].any()
    assert both(exe, tmp_path, pts, 0.0625, 41)["status"][3] == 40


def test_bridge_stays_a_border_and_numbering_goes_by_core(exe, tmp_path):
    pts = ref.bridge_cloud()
    want = both(exe, tmp_path, pts, 0.25, 20, keep=1, what="bridge")
    assert want["status"].tolist() == [2, 54, 1, 0, 28, 55, 0, 1]
    assert not want["core"][0] and want["labels"][0] == 0                      # the bridge: a border, the lower number
    assert np.all(want["labels"][1:28] == 0) and np.all(want["labels"][28:] == 1) and want["counts"].tolist() == [28, 27]
    # the border's row (0) is lower than every core of its cluster: cluster 0 is still the one of the lowest CORE, row 1;
    # with the blobs swapped the bridge still takes number 0, now the other blob
    swapped = np.concatenate([pts[:1], pts[28:], pts[1:28]])
    got = both(exe, tmp_path, swapped, 0.25, 20, what="bridge swapped")
    assert got["labels"][0] == 0 and got["counts"].tolist() == [28, 27]
    # B moved away, so the bridge touches A alone: row 0 is A's lowest MEMBER, but B holds the lowest CORE (row 1) and is
    # cluster 0 — a numbering by lowest member would have made A cluster 0
    front = np.concatenate([pts[:1], pts[1:28] + np.float32(8.0), pts[28:]])
    got = both(exe, tmp_path, front, 0.25, 20, what="front border")
    assert got["labels"][0] == 1 and np.all(got["labels"][1:28] == 0) and got["counts"].tolist() == [27, 28] and got["status"][2] == 1


def test_selection_rule(exe, tmp_path):
    labels = np.array([0, 0, 0, 1, 1, 1, 2, 2, -1, 3, 3, 3, 4], np.int32)
    counts = np.array([3, 3, 2, 3, 1], np.int32)
    assert ref.select(labels, counts, 1, 0)[1].tolist() == [9, 3, 13, 1]      # three clusters tie at the first place: all stay
    assert ref.select(labels, counts, 4, 0)[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]
    assert ref.select(labels, counts, 0, 0)[1].tolist() == [12, 0, 13, 1]     # keep = 0: the floor alone, and noise still goes
    assert ref.select(labels, counts, -3, 3)[0].tolist() == [0, 1, 2, 3, 4, 5, 9, 10, 11]
    assert ref.select(labels, counts, 99, 0)[1].tolist() == [12, 1, 13, 1]
    assert ref.select(np.full(5, -1, np.int32), np.zeros(0, np.int32), 1, 0)[1].tolist() == [0, 0, 5, 1]
    # ... and the header's routine on a cloud with ties: two equal blobs and a smaller one
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float32) / 16
    pts = np.concatenate([g, g + np.float32(4.0), (g + np.float32(8.0))[:20], [[20.0, 0, 0]]]).astype(np.float32)
    for keep, floor, kept in ((1, 0, 54), (2, 0, 54), (3, 0, 74), (0, 0, 74), (0, 21, 54), (1, 28, 0), (5, 0, 74)):
        want = both(exe, tmp_path, pts, 0.25, 5, keep, floor, f"keep={keep} floor={floor}")
        assert want["status"][0] == 3 and ref.select(want["labels"], want["counts"], keep, floor)[1][0] == kept


def test_argument_errors_of_the_host_routine(exe, tmp_path):
    pts = ref.lattice_cloud(10, 1)
    for eps, mp in ((0.0, 3), (-1.0, 3), (float("nan"), 3), (float("inf"), 3), (2e19, 3), (1.0, 0), (1.0, -2)):
        assert ref.run_host(exe, tmp_path, pts, eps, mp)["rc"] == 1, (eps, mp)
    assert ref.run_host(exe, tmp_path, pts, 1.8e19, 3)["rc"] == 0             # (its square is finite)
