"""include/sls_fill_math.h compiled for the host with its sequential driver against the NumPy restatement of tests/fill_ref.py
(no device needed): the half-edges, the loop numbers, the loop lengths, the vertices, the faces with their -1 padding and all
16 status words equal on every case and setting — the driver labels components by a union-find, the restatement walks along
the next pointers — and the topological claims of the case table, on the restatement."""
import functools

import numpy as np
import pytest

import fill_ref as ref
import mesh_ref
from mesh_ref import bits

CASES = ref.cases()
SETTINGS = ref.settings()


@pytest.fixture(scope="module")
def host():
    return ref.host()


@functools.lru_cache(maxsize=None)
def _found(case):
    v, f, counts = CASES[case]
    return ref.loops(f, len(v), counts)


def _room(case):
    v, f, _ = CASES[case]
    return ref.room(len(v), len(f), 1.0)


def _filled(case, max_edges=128, max_size=0.0):
    v, f, counts = CASES[case]
    out_v, out_f, status = ref.fill(v, f, max_edges, max_size, *_room(case), counts=counts, found=_found(case))
    return out_v, out_f[:status[1]], dict(zip(ref.STATUS, status))


def _edges(faces, V):
    return mesh_ref.clusters(faces, V)[2]


@pytest.mark.parametrize("case", sorted(CASES))
def test_loops_header_equals_restatement(host, case):
    v, f, counts = CASES[case]
    he, loop, cycles, words = _found(case)
    got_he, got_loop, got_edges, status = host.loops(f, len(v), counts)
    assert status == (ref.loop_status(words) if len(v) and len(f) else ref.empty_status(len(v), len(f), counts, False)), case
    assert np.array_equal(got_he, he) and np.array_equal(got_loop, loop) and got_edges.tolist() == [len(c) for c in cycles]
    # every loop is a cycle of at least three half-edges over vertices that differ, numbered by its lowest vertex
    lowest = [int(he[c, 0].min()) for c in cycles]
    assert lowest == sorted(lowest) and all(len(c) >= 3 and len(set(he[c, 0].tolist())) == len(c) for c in cycles)
    for c in cycles:
        assert np.array_equal(he[c, 1], he[np.roll(c, -1), 0]) and he[c[0], 0] == he[c, 0].min()


@pytest.mark.parametrize("case", sorted(CASES))
def test_fill_header_equals_restatement(host, case):
    v, f, counts = CASES[case]
    VL, TL = ref.live(len(v), len(f), counts)
    cap_v, cap_t = _room(case)
    for max_edges, max_size in SETTINGS:
        want_v, want_f, want_s = ref.fill(v, f, max_edges, max_size, cap_v, cap_t, counts=counts, found=_found(case))
        got_v, got_f, status = host.fill(v, f, max_edges, max_size, cap_v, cap_t, counts=counts)
        assert status == want_s, (case, max_edges, max_size)
        assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_f, want_f), (case, max_edges, max_size)
        assert np.array_equal(bits(got_v[:VL]), bits(v[:VL])) and np.array_equal(got_f[:TL], f[:TL])     # the input comes first, unchanged
        assert (got_f[status[1]:] == -1).all() and len(got_f) == cap_t and status[0] == len(got_v) and status[15] == 1
        assert status[3] == status[4] + status[5] + status[6] + status[7] and status[14] == 0


def test_tetrahedron_cube_and_triangle():
    """L = 3: one triangle and no vertex, the result closed; L = 4: one centre; a single triangle is its own rim and is filled
    by its reverse — that is what the rule says"""
    v, f, s = _filled("tet_open")
    assert (s["loops"], s["filled"], s["vertices"], s["triangles"]) == (1, 1, 4, 4) and f[3].tolist() == [0, 3, 2]      # the face left out, (2, 0, 3), from its lowest vertex
    stats = _edges(f, 4)
    assert stats["boundary_edges"] == 0 and stats["nonmanifold_edges"] == 0 and mesh_ref.euler(f) == 2
    v, f, s = _filled("cube_open")
    assert (s["loops"], s["filled"], s["vertices"], s["triangles"], s["halfedges"]) == (1, 1, 9, 14, 4)
    assert bits(v[8]).tolist() == bits(np.float32([0.5, 0.5, 0.0])).tolist() and (f[10:, 2] == 8).all()
    stats = _edges(f, 9)
    assert stats["boundary_edges"] == 0 and stats["nonmanifold_edges"] == 0 and mesh_ref.euler(f) == 2
    v, f, s = _filled("triangle", 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 1]] and s["vertices"] == 3 and _edges(f, 3)["boundary_edges"] == 0


def test_sphere_closes_at_128_and_keeps_two_loops_at_64():
    v0, f0, _ = CASES["sphere_caps"]
    he, loop, cycles, words = _found("sphere_caps")
    assert sorted(len(c) for c in cycles) == sorted(ref.SPHERE_LOOPS) and words[8] == 0 and words[9] == 0
    v, f, s = _filled("sphere_caps", 128)
    stats = _edges(f, len(v))
    assert s["filled"] == 6 and stats["boundary_edges"] == 0 and stats["nonmanifold_edges"] == 0 and mesh_ref.euler(f) == 2
    assert len(v) == len(v0) + 5 and len(f) == len(f0) + sum(ref.SPHERE_LOOPS) - 3 + 1
    for k, c in enumerate(x for x in cycles if len(x) > 3):          # every new vertex lies inside its loop's bounding box
        p, new = v0[he[c, 0]], v[len(v0) + k]
        assert (new >= p.min(0)).all() and (new <= p.max(0)).all()
    v, f, s = _filled("sphere_caps", 64)
    assert (s["filled"], s["skipped_edges"]) == (4, 2) and _edges(f, len(v))["boundary_edges"] == 65 + 89 == 154
    v, f, s = _filled("sphere_caps", 128, ref.SIZE_SPLIT)
    assert (s["filled"], s["skipped_size"], s["skipped_edges"]) == (2, 4, 0)
    v, f, s = _filled("sphere_caps", 64, ref.SIZE_SPLIT)             # the first failing reason counts: edges before size
    assert (s["filled"], s["skipped_size"], s["skipped_edges"]) == (2, 2, 2)


def test_long_loops_follow_the_butterfly():
    """the loops of 65 and 100 of "rings": 64 lanes and the butterfly, not one sum after the other (the two orders differ in
    the last bits there, so a host or a device that took the short path would be caught; the loops of 64 take the short one)"""
    v0, _, _ = CASES["rings"]
    he, _, cycles, _ = _found("rings")
    assert sorted(len(c) for c in cycles) == [64, 64, 65, 65, 100, 100]
    differs = []
    for c in (x for x in cycles if len(x) > ref.LONG):
        p = v0[np.sort(he[c, 0])].astype(np.float64)
        serial = np.zeros((3,))
        for row in p:
            serial = serial + row
        differs.append(not np.array_equal((serial / len(c)).astype(np.float32), (ref.segment_sum(p) / len(c)).astype(np.float32)))
    print(differs)
    assert len(differs) == 4 and any(differs)


def test_complex_vertices_keep_their_chains_open():
    for case, want in (("pinch", dict(loops=1, filled=1, open_halfedges=8, complex_vertices=1)),
                       ("flipped", dict(loops=1, filled=1, open_halfedges=4, complex_vertices=2)),
                       ("fin", dict(loops=1, filled=1, open_halfedges=6, complex_vertices=2))):
        v, f, s = _filled(case)
        assert {k: s[k] for k in want} == want, (case, s)             # the one loop is the sheet's outer rim: 20 half-edges
        he, loop, cycles, _ = _found(case)
        assert [len(c) for c in cycles] == [20] and (f[len(CASES[case][1]):, 2] == len(CASES[case][0])).all()
    he, loop, _, _ = _found("pinch")
    corner = 2 * 6 + 2
    assert sorted(he[loop < 0].reshape(-1).tolist()).count(corner) == 4     # both holes' rims pass through the shared corner


def test_capacity_rows_are_ignored_and_new_vertices_start_at_the_live_count():
    v0, f0, (VL, TL) = CASES["at_capacity"]
    v, f, s = _filled("at_capacity")
    assert (s["loops"], s["filled"], s["degenerate"], s["out_of_range"]) == (3, 3, 4, 3) and len(v) == VL + 3 < len(v0) + 3
    assert np.array_equal(bits(v[:VL]), bits(v0[:VL])) and np.array_equal(f[:TL], f0[:TL]) and sorted(set(f[TL:, 2].tolist())) == [VL, VL + 1, VL + 2]
    assert np.isfinite(v[VL:]).all() and bits(v[21]).tolist() == [0x80000000] * 3
    same = ref.fill(v0[:VL], f0[:TL], 128, 0.0, *_room("at_capacity"))      # ... as if the rows beyond were not there
    assert np.array_equal(bits(same[0]), bits(v)) and np.array_equal(same[1][:same[2][1]], f)


def test_nan_rim_is_skipped_and_counted():
    v, f, s = _filled("nan_rim")
    assert (s["loops"], s["filled"], s["skipped_nonfinite"]) == (4, 3, 1) and np.isfinite(v[len(CASES["nan_rim"][0]):]).all()


def test_many_loops_pass_every_chunk():
    he, loop, cycles, words = _found("many_loops")
    assert words[3] == ref.MANY_CELLS ** 2 + 1 >= 3 * ref.CHUNK and words[2] == 25600 >= 3 * ref.CHUNK
    v, f, s = _filled("many_loops", 64)
    assert (s["filled"], s["skipped_edges"]) == (ref.MANY_CELLS ** 2, 1) and _edges(f, len(v))["boundary_edges"] == 636


def test_no_room_fills_nothing():
    v0, f0, _ = CASES["sphere_caps"]
    need = ref.fill(v0, f0, 128, 0.0, *_room("sphere_caps"), found=_found("sphere_caps"))[2]
    for cap_v, cap_t in ((need[12], need[13] - 1), (need[12] - 1, need[13])):
        v, f, s = ref.fill(v0, f0, 128, 0.0, cap_v, cap_t, found=_found("sphere_caps"))
        assert s[14] == 1 and s[12:14] == need[12:14] and s[0] == len(v0) and s[1] == len(f0) and s[4] == 0
        assert np.array_equal(bits(v), bits(v0)) and np.array_equal(f[:len(f0)], f0) and (f[len(f0):] == -1).all()
        got = ref.host().fill(v0, f0, 128, 0.0, cap_v, cap_t)
        assert got[2] == s and np.array_equal(bits(got[0]), bits(v)) and np.array_equal(got[1], f)
    exact = ref.host().fill(v0, f0, 128, 0.0, need[12], need[13])
    assert exact[2][14] == 0 and exact[2][4] == 6


def test_nothing_to_fill():
    for case in ("closed", "no_faces", "no_vertices"):
        v0, f0, _ = CASES[case]
        v, f, s = _filled(case)
        assert s["halfedges"] == 0 and s["loops"] == 0 and np.array_equal(bits(v), bits(v0)) and np.array_equal(f, f0)
