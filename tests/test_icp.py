"""sls_cloud_icp and its Python faces (splat_loam_amd/evaluation.py: register_icp, evaluate_recon(align=),
tools/cloud_align.py) on the device against the NumPy restatement (icp_ref.py).

Two kinds of input make the comparison bit for bit.  (1) Lattice inputs (multiples of 1/16) under a pose that is a signed
permutation with a lattice translation: p' stays on the lattice, the float32 d2 is exact, so the brute force's association IS
the kernel's, ties and points exactly on the gate included; from equal associations the header's float64 arithmetic and its
fixed order of summation give equal bits.  (2) Scenes where no association is in doubt: the restatement records for every
point of every pass the relative gap between the best and the second-best float64 d2 and between d2 and the gate, the test
asserts on the restatement ALONE that every gap exceeds 1e-4 — four decades above what float32 rounding of d2 can move —
and then float32 and float64 searches agree and pose, status words and sums are array_equal after every iteration count.
Where associations are NOT exact (a noisy room) the device is held to the restatement's own error to the truth."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_ref as ref
from splat_loam_amd import _abi, evaluation, ply_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4
# the smallest Ms whose partial rows exceed one round of the solve kernel's 256 threads: 256 blocks of 256 points, and one
SECOND_ROUND = ref.BLOCK * ref.BLOCK + 1


def raw_call(device, source, target, normals, init=None, method=ref.PLANE, max_distance=1.0, iterations=30, **params):
    """sls_cloud_icp itself: dict(status (20,) int64, system (32,) float64, index, dist2) as NumPy arrays."""
    prm, pose = evaluation._check_icp_args(max_distance, iterations, "plane" if method == ref.PLANE else "point", init, params)
    src = torch.tensor(np.ascontiguousarray(source, np.float32).reshape(-1, 3), device=device)
    tgt = torch.tensor(np.ascontiguousarray(target, np.float32), device=device)
    nrm = torch.tensor(np.ascontiguousarray(normals, np.float32), device=device) if normals is not None else None
    with torch.cuda.device(device):
        st = torch.cuda.current_stream(device).cuda_stream
        status, system, index, dist2 = evaluation._icp_enqueue(_abi.lib(), src, tgt, nrm, prm, pose, True, st)
    return dict(status=status.cpu().numpy(), system=system.cpu().numpy(), index=index.cpu().numpy(), dist2=dist2.cpu().numpy())


def pose_of(status):
    return status[6:18].copy().view(np.float64)


def same_as_ref(got, want, Ms, Mt, what):
    """status words, the 29 sums (and the three zeros behind them) and the association, bit for bit"""
    assert np.array_equal(got["status"], ref.status_words(want, Ms, Mt)), \
        f"{what}: status {got['status'][:6]} / {ref.status_words(want, Ms, Mt)[:6]}, pose {pose_of(got['status'])} / {want['pose']}"
    assert np.array_equal(got["system"][:ref.TERMS].view(np.int64), want["system"].view(np.int64)), \
        f"{what}: sums differ at {np.flatnonzero(got['system'][:ref.TERMS] != want['system'])}"
    assert np.all(got["system"][ref.TERMS:] == 0.0)
    assert np.array_equal(got["index"], want["index"]), what
    assert np.array_equal(got["dist2"].view(np.uint32), want["dist2"].view(np.uint32)), what


# ---- 1. one linearisation on the lattice -------------------------------------------------------------------------------
P_LATTICE = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])       # a quarter turn about z
T_LATTICE = np.array([0.5, -1.25, 2.0])
GATE_LATTICE = 0.75                                                             # g2 = 9/16: d = (3/4, 0, 0) lies exactly on it


def beside(tgt, dist):
    """a lattice point exactly `dist` along an axis from one target, every other target strictly farther away"""
    t64 = tgt.astype(np.float64)
    for j in range(len(t64)):
        for axis in range(3):
            for sign in (1.0, -1.0):
                p = t64[j].copy()
                p[axis] += sign * dist
                if np.all(np.delete(((t64 - p) ** 2).sum(1), j) > dist * dist):
                    return p
    raise AssertionError("no target with room beside it")


@functools.lru_cache(maxsize=None)
def lattice_case(Ms, Mt):
    rng = np.random.default_rng(77 * Ms + Mt)
    tgt = np.unique(rng.integers(-48, 49, (Mt * 2, 3)), axis=0)
    tgt = (tgt[rng.permutation(len(tgt))[:Mt]] / 16.0).astype(np.float32)
    assert len(tgt) == Mt
    if Mt > 9:
        tgt[5] = tgt[9]                                                         # two copies: the lower row wins
    nrm = rng.normal(size=(Mt, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    moved = rng.integers(-56, 57, (Ms, 3)) / 16.0
    # made by hand, Ms permitting: exactly on the gate, one step beyond it, on a target
    special = [beside(tgt, 0.75), beside(tgt, 0.8125), tgt[min(9, Mt - 1)]]
    for k, s in enumerate(special[:Ms]):
        moved[k] = s
    src = ((moved - T_LATTICE) @ P_LATTICE).astype(np.float32)                  # p = P^T (p' - t), exact
    init = ref.pose12(P_LATTICE, T_LATTICE)
    assert np.array_equal(ref.transform(init, src), moved.astype(np.float32))
    return src, tgt, nrm, init


@pytest.mark.parametrize("Ms,Mt", [(1, 40), (63, 40), (64, 300), (65, 300), (256, 700), (257, 700), (1500, 1), (SECOND_ROUND, 300)])
def test_one_linearisation_bit_for_bit(device, Ms, Mt):
    src, tgt, nrm, init = lattice_case(Ms, Mt)
    for method in (ref.PLANE, ref.POINT):
        want = ref.icp(src, tgt, nrm, init, method, GATE_LATTICE, 0)
        got = raw_call(device, src, tgt, nrm, init, method, GATE_LATTICE, 0)
        same_as_ref(got, want, Ms, Mt, f"Ms={Ms} Mt={Mt} method={method}")
        assert want["updates"] == 0 and want["flags"] == 0 and got["status"][18] == 2
    lin = want["passes"][0]
    g2 = ref.gate2(GATE_LATTICE)
    assert lin["inlier"][0] and lin["dist2"][0] == g2                           # the gate itself is inside
    if Ms >= 63:
        assert not lin["inlier"][1] and lin["dist2"][1] == np.float32(0.8125 ** 2) and lin["dist2"][2] == 0.0
        assert 0 < want["inliers"] < Ms                                         # both sides of the gate
        if Mt > 1:
            d = ref.dist2_f32(lin["moved"][:2048], tgt)
            assert ((d == d.min(1, keepdims=True)).sum(1) > 1).any()            # equally near targets: the lowest row wins


# ---- 2, 3, 4a. whole runs at unambiguous associations --------------------------------------------------------------------
TRUTH_WALLS = ref.pose12(ref.rotation([0.3, -0.5, 0.8], 0.012), [0.012, -0.009, 0.011])
GATE_WALLS = 0.2


@functools.lru_cache(maxsize=None)
def walls_case(method):
    """Three lattice walls (spacing 1/4 m); the source: every other target row moved by the inverse of TRUTH_WALLS — at most
    5 cm, well under half the spacing — plus twelve points with no counterpart within the gate.  The restatement's run to
    convergence, with its margins."""
    tgt, nrm = ref.walls(9)
    R, t = TRUTH_WALLS.reshape(3, 4)[:, :3], TRUTH_WALLS.reshape(3, 4)[:, 3]
    rng = np.random.default_rng(3)
    lost = np.array([2.6, 2.7, 2.9]) + rng.uniform(0.0, 0.4, (12, 3)) * [1, 1, 1]
    lost[:6] -= [0.0, 0.9, 1.3]
    src = ((np.concatenate([tgt[::2].astype(np.float64), lost]) - t) @ R).astype(np.float32)
    want = ref.icp(src, tgt, nrm, None, method, GATE_WALLS, 50, margins=True)
    return src, tgt, nrm, want


def result_after(want, n):
    """What `iterations = n` returns, from the passes of one longer run of the restatement (n <= its updates)."""
    lin = want["passes"][n]
    return dict(pose=lin["pose"], updates=n, flags=want["flags"] if n == want["updates"] else 0, inliers=int(lin["system"][28]),
                sum_r2=float(lin["system"][27]), system=lin["system"], index=lin["index"], dist2=lin["dist2"])


@pytest.mark.parametrize("method", [ref.PLANE, ref.POINT])
def test_whole_runs_bit_for_bit(device, method):
    src, tgt, nrm, want = walls_case(method)
    k = want["updates"]
    assert want["flags"] == ref.FLAG_CONVERGED and 2 <= k <= 20 and len(want["passes"]) == k + 1
    # THE CONDITION, on the restatement alone, every pass, every point: no association and no gate decision is in doubt
    for n, lin in enumerate(want["passes"]):
        assert lin["gap_nn"].min() > MARGIN and lin["gap_gate"].min() > MARGIN, (n, lin["gap_nn"].min(), lin["gap_gate"].min())
        assert lin["inlier"].sum() == len(src) - 12 and not lin["inlier"][-12:].any()
    for n in range(1, k + 1):
        got = raw_call(device, src, tgt, nrm, None, method, GATE_WALLS, n)
        same_as_ref(got, result_after(want, n), len(src), len(tgt), f"iterations={n} of {k}, method={method}")
    # 3. freeze: far more iterations than needed, and a second run
    a = raw_call(device, src, tgt, nrm, None, method, GATE_WALLS, 50)
    b = raw_call(device, src, tgt, nrm, None, method, GATE_WALLS, 50)
    same_as_ref(a, result_after(want, k), len(src), len(tgt), "iterations=50")
    for key in a:
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), f"two runs differ in {key}"
    # 4a. it registers: the bar is four times the restatement's own distance to the truth, measured here
    rot_ref, trans_ref = ref.pose_error(want["pose"], TRUTH_WALLS)
    rot, trans = ref.pose_error(pose_of(a["status"]), TRUTH_WALLS)
    print(f"walls method={method}: restatement {rot_ref:.3e} rad {trans_ref:.3e} m after {k} updates; device {rot:.3e} rad {trans:.3e} m")
    assert rot_ref < 1e-6 and trans_ref < 1e-6                                  # (float32 rounding of p' and of the source)
    assert rot <= 4 * rot_ref and trans <= 4 * trans_ref


# ---- 4b. a noisy room: associations are not exact, bits may differ --------------------------------------------------------
TRUTH_ROOM = ref.pose12(ref.rotation([0.2, 0.1, 1.0], 0.01), [0.05, -0.04, 0.02])
GATE_ROOM = 0.5


def room(n, seed):
    """n points on the six faces of a 10 x 8 x 3 m room, 5 mm of noise"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-5.0, -4.0, 0.0]), np.array([5.0, 4.0, 3.0])
    p = rng.uniform(lo, hi, (n, 3))
    face = rng.integers(0, 6, n)
    p[np.arange(n), face % 3] = np.where(face < 3, lo[face % 3], hi[face % 3])
    return (p + rng.normal(0, 0.005, p.shape)).astype(np.float32)


def test_it_registers_a_noisy_room(device):
    """(Hard associations on noisy clouds can end in a cycle of period two instead of a fixed point — the pairs flip back and
    forth and the step stays at 1e-4 — so nothing here rests on the convergence flag.)"""
    tgt, moved = room(3000, 1), room(1200, 2)
    R, t = TRUTH_ROOM.reshape(3, 4)[:, :3], TRUTH_ROOM.reshape(3, 4)[:, 3]
    src = ((moved.astype(np.float64) - t) @ R).astype(np.float32)
    nrm = evaluation.estimate_normals(torch.tensor(tgt, device=device), radius=None, max_nn=12, viewpoint=(0.0, 0.0, 1.5)).cpu().numpy()
    want = ref.icp(src, tgt, nrm, None, ref.PLANE, GATE_ROOM, 12)
    got = raw_call(device, src, tgt, nrm, None, ref.PLANE, GATE_ROOM, 12)
    rot_ref, trans_ref = ref.pose_error(want["pose"], TRUTH_ROOM)
    rot, trans = ref.pose_error(pose_of(got["status"]), TRUTH_ROOM)
    last = ref.linearize(src, tgt, nrm, want["pose"], ref.PLANE, GATE_ROOM, margins=True)
    doubtful = int(((last["gap_nn"] <= MARGIN) | (last["gap_gate"] <= MARGIN)).sum())
    print(f"room: restatement {rot_ref:.3e} rad {trans_ref:.3e} m, {want['updates']} updates, {want['inliers']} inliers, flags "
          f"{want['flags']}; device {rot:.3e} rad {trans:.3e} m, {got['status'][0]} updates, {got['status'][1]} inliers, flags "
          f"{got['status'][4]}; {doubtful} doubtful points")
    # it did register: from 1e-2 rad and 6.7 cm to within 5 mrad and two sigmas of the 5 mm noise
    assert want["updates"] >= 3 and rot_ref < 5e-3 and trans_ref < 1e-2
    assert rot <= 2 * rot_ref and trans <= 2 * trans_ref
    assert doubtful < 0.01 * len(src)                                           # on the restatement alone
    assert abs(int(got["status"][1]) - want["inliers"]) <= doubtful             # fitness = inliers / Ms
    assert want["inliers"] > 0.99 * len(src)


# ---- 5. refusals and edges -----------------------------------------------------------------------------------------------
def test_edges(device):
    tgt, nrm = ref.walls(9)
    src = tgt[::2] + np.float32([0.01, 0.0, 0.0])
    # a single plane holds three freedoms.  Without damping: not positive definite, the pose is kept bit for bit
    plane, pn = tgt[162:], nrm[162:] * 0 + np.float32([0, 0, 1])
    psrc = plane[::2] + np.float32([0.0, 0.0, 0.0625])
    init = ref.pose12(ref.rotation([0, 0, 1], 0.0), [0.0, 0.0, 0.0])
    got = raw_call(device, psrc, plane, pn, init, ref.PLANE, 0.2, 10, damping=0.0)
    want = ref.icp(psrc, plane, pn, init, ref.PLANE, 0.2, 10, damping=0.0)
    assert want["flags"] == ref.FLAG_NOT_PD and want["updates"] == 0
    same_as_ref(got, want, len(psrc), len(plane), "one plane, no damping")
    assert np.array_equal(pose_of(got["status"]), init)
    # with the default damping the three unobservable freedoms (x, y, rotation about z) stay at their initial values
    got = raw_call(device, psrc, plane, pn, init, ref.PLANE, 0.2, 10)
    T = pose_of(got["status"]).reshape(3, 4)
    assert got["status"][4] == ref.FLAG_CONVERGED and abs(T[2, 3] + 0.0625) < 1e-7
    assert abs(T[0, 3]) < 1e-9 and abs(T[1, 3]) < 1e-9 and abs(T[1, 0]) < 1e-9
    # fewer inliers than min_inliers keeps the initial pose bit for bit
    init = ref.pose12(ref.rotation([1, 2, 3], 0.004), [0.01, 0.0, -0.01])
    got = raw_call(device, src, tgt, nrm, init, ref.PLANE, 0.2, 10, min_inliers=len(src) + 1)
    assert got["status"][4] == ref.FLAG_FEW and got["status"][0] == 0 and got["status"][1] == len(src)
    assert np.array_equal(pose_of(got["status"]), init)
    same_as_ref(got, ref.icp(src, tgt, nrm, init, ref.PLANE, 0.2, 10, min_inliers=len(src) + 1), len(src), len(tgt), "too few inliers")
    # Ms = 0
    got = raw_call(device, np.zeros((0, 3), np.float32), tgt, nrm, init, ref.PLANE, 0.2, 10)
    assert np.array_equal(got["status"], ref.status_words(ref.icp(np.zeros((0, 3), np.float32), tgt, nrm, init), 0, len(tgt)))
    assert got["status"][4] == ref.FLAG_FEW and np.all(got["system"] == 0.0)
    # Mt = 1: every point pairs with the one target; the point method pulls the centroid onto it
    one = np.float32([[1.0, 2.0, 3.0]])
    want = ref.icp(src, one, None, None, ref.POINT, 8.0, 0)
    same_as_ref(raw_call(device, src, one, None, None, ref.POINT, 8.0, 0), want, len(src), 1, "Mt = 1")
    assert want["inliers"] == len(src) and np.all(want["index"] == 0)
    # a non-identity initial pose, far from the identity: the source is given in another frame
    far = ref.pose12(ref.rotation([0.0, 1.0, 0.2], 2.0), [3.0, -1.0, 0.5])
    R, t = far.reshape(3, 4)[:, :3], far.reshape(3, 4)[:, 3]
    fsrc = ((tgt[::2].astype(np.float64) - t) @ R).astype(np.float32)
    near = ref.pose12(ref.rotation([1, 1, 0], 0.01) @ R, t + [0.01, 0.01, -0.01])
    want = ref.icp(fsrc, tgt, nrm, near, ref.PLANE, 0.2, 30, margins=True)
    assert want["flags"] == ref.FLAG_CONVERGED and all(l["gap_nn"].min() > MARGIN and l["gap_gate"].min() > MARGIN for l in want["passes"])
    got = raw_call(device, fsrc, tgt, nrm, near, ref.PLANE, 0.2, 30)
    same_as_ref(got, want, len(fsrc), len(tgt), "a non-identity initial pose")
    assert max(ref.pose_error(pose_of(got["status"]), far)) < 1e-6
    # method="point" on a cloud without normals
    r = evaluation.register_icp(torch.tensor(src, device=device), torch.tensor(tgt, device=device), max_distance=0.2, method="point")
    assert r["converged"] and abs(float(r["target_T_source"][0, 3]) + 0.01) < 1e-6 and r["fitness"] == 1.0


# ---- 6. the Python faces ---------------------------------------------------------------------------------------------------
def test_register_icp_equals_the_raw_call(device):
    src, tgt, nrm, want = walls_case(ref.PLANE)
    raw = raw_call(device, src, tgt, nrm, None, ref.PLANE, GATE_WALLS, 30)
    t = lambda a: torch.tensor(a, device=device)
    r = evaluation.register_icp(t(src), t(tgt), t(nrm), max_distance=GATE_WALLS, return_details=True)
    assert np.array_equal(r["target_T_source"][:3].numpy().reshape(-1), pose_of(raw["status"]))
    assert r["target_T_source"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert r["updates"] == raw["status"][0] and r["inliers"] == raw["status"][1] and r["flags"] == raw["status"][4] and r["converged"]
    assert r["fitness"] == raw["status"][1] / len(src) and r["inlier_rmse"] == math.sqrt(raw["system"][27] / raw["system"][28])
    assert np.array_equal(r["system"].cpu().numpy(), raw["system"]) and np.array_equal(r["index"].cpu().numpy(), raw["index"])
    plain = evaluation.register_icp(t(src), t(tgt), t(nrm), max_distance=GATE_WALLS)
    assert "system" not in plain and torch.equal(plain["target_T_source"], r["target_T_source"])
    # init as 4x4, as 3x4 and as 12 numbers
    for init in (r["target_T_source"], r["target_T_source"][:3], r["target_T_source"][:3].reshape(-1).tolist()):
        again = evaluation.register_icp(t(src), t(tgt), t(nrm), init=init, max_distance=GATE_WALLS, iterations=0)
        assert torch.equal(again["target_T_source"], r["target_T_source"]) and again["updates"] == 0 and again["inliers"] == r["inliers"]
    # without normals the plane method estimates them first
    est = evaluation.register_icp(t(src), t(tgt), max_distance=GATE_WALLS)
    assert est["converged"] and max(ref.pose_error(est["target_T_source"][:3].numpy().reshape(-1), TRUTH_WALLS)) < 1e-3


def grid_mesh(n=60, size=3.0):
    """three mutually orthogonal n x n vertex grids, triangulated: (vertices float32, faces int32)"""
    g = np.linspace(0.0, size, n)
    a, b = (v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij"))
    z = np.zeros_like(a)
    verts = np.concatenate([np.stack([z, a, b], 1), np.stack([a, z, b], 1), np.stack([a, b, z], 1)]).astype(np.float32)
    i, j = (v.reshape(-1) for v in np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij"))
    q = i * n + j
    one = np.concatenate([np.stack([q, q + 1, q + n], 1), np.stack([q + 1, q + n + 1, q + n], 1)])
    return verts, np.concatenate([one + k * n * n for k in range(3)]).astype(np.int32)


def test_evaluate_recon_align(device):
    """A mesh moved by a known small motion, aligned, scores what the unmoved mesh scores.  How the bar carries through: the
    pose is found to within 1e-4 m over the mesh (asserted), so every sampled point moves by less than that; the metrics are
    means and fractions of nearest distances, 1-Lipschitz in the points, so the means move by at most 1e-4 m = 0.01 cm (plus
    the voxel down-sample, switched off here) and a fraction only by the points within 1e-4 m of its threshold (none: the
    distances of this scene lie far below 0.2 m)."""
    verts, faces = grid_mesh()
    rng = np.random.default_rng(5)
    reference = (verts[rng.integers(0, len(verts), 30000)] + rng.uniform(-0.02, 0.02, (30000, 3)) * [1, 1, 1]).astype(np.float32)
    R, t = TRUTH_ROOM.reshape(3, 4)[:, :3], TRUTH_ROOM.reshape(3, 4)[:, 3]
    moved = ((verts.astype(np.float64) - t) @ R).astype(np.float32)
    tt = lambda a: torch.tensor(a, device=device)
    kw = dict(down_sample_res=0.0, mesh_sample_point=40000, seed=3)
    base = evaluation.evaluate_recon(tt(reference), tt(verts), tt(faces), **kw)
    assert "Alignment" not in base
    skewed = evaluation.evaluate_recon(tt(reference), tt(moved), tt(faces), **kw)
    fixed = evaluation.evaluate_recon(tt(reference), tt(moved), tt(faces), align=dict(max_distance=0.3, iterations=30, max_points=5000), **kw)
    al = fixed["Alignment"]
    assert al["converged"] and al["fitness"] > 0.99
    found = al["target_T_source"].numpy()
    worst = np.abs(verts.astype(np.float64) - (moved.astype(np.float64) @ found[:3, :3].T + found[:3, 3])).max()
    print(f"evaluate_recon(align): vertices back to within {worst:.3e} m; chamfer {base['Chamfer_L1 (cm)']:.4f} / "
          f"{skewed['Chamfer_L1 (cm)']:.4f} moved / {fixed['Chamfer_L1 (cm)']:.4f} aligned")
    assert worst < 5e-3                             # the reference is the mesh + 2 cm of uniform noise: the pose is a fit to it
    assert skewed["Chamfer_L1 (cm)"] > base["Chamfer_L1 (cm)"] + 0.5
    for key in ("MAE_accuracy (cm)", "MAE_completeness (cm)", "Chamfer_L1 (cm)"):
        assert abs(fixed[key] - base[key]) <= 100 * worst, key
    for key in ("Precision [Accuracy] (%)", "Recall [Completeness] (%)", "F-score (%)"):
        assert fixed[key] == base[key] == 100.0, key


def test_cloud_align_round_trips_a_ply(device, tmp_path):
    src, tgt, nrm, want = walls_case(ref.POINT)
    ply_io.save_point_cloud(str(tmp_path / "source.ply"), src[:-12], np.zeros_like(src[:-12]))
    ply_io.save_point_cloud(str(tmp_path / "target.ply"), tgt, nrm)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cloud_align.py"), str(tmp_path / "source.ply"),
                          str(tmp_path / "target.ply"), str(tmp_path / "out.ply"), "--max-distance", str(GATE_WALLS), "--method", "point"],
                         check=True, capture_output=True, text=True).stdout
    pose = np.array([float(v) for v in out.strip().split("\n")[-1].split()])
    assert pose.shape == (12,) and max(ref.pose_error(pose, TRUTH_WALLS)) < 1e-6
    back = ply_io.load_point_cloud(str(tmp_path / "out.ply"))[0]
    assert back.shape == (len(src) - 12, 3) and np.abs(back - tgt[::2]).max() < 1e-6


def test_eval_recon_tool_aligns(device, tmp_path):
    import json
    verts, faces = grid_mesh(30)
    rng = np.random.default_rng(6)
    reference = (verts[rng.integers(0, len(verts), 8000)] + rng.uniform(-0.01, 0.01, (8000, 3))).astype(np.float32)
    R, t = TRUTH_ROOM.reshape(3, 4)[:, :3], TRUTH_ROOM.reshape(3, 4)[:, 3]
    ply_io.save_mesh(str(tmp_path / "mesh.ply"), ((verts.astype(np.float64) - t) @ R).astype(np.float32), faces)
    ply_io.save_point_cloud(str(tmp_path / "reference.ply"), reference, np.zeros_like(reference))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_recon.py"), str(tmp_path / "reference.ply"),
                          str(tmp_path / "mesh.ply"), "--align", "0.3", "--down-sample-res", "0", "--mesh-sample-point", "20000"],
                         check=True, capture_output=True, text=True).stdout
    res = json.loads(out.strip().split("\n")[-1])
    al = res["Alignment"]
    assert al["converged"] and al["fitness"] > 0.99 and len(al["target_T_source"]) == 12
    rot, trans = ref.pose_error(np.array(al["target_T_source"]), TRUTH_ROOM)
    assert rot < 2e-3 and trans < 5e-3 and res["F-score (%)"] == 100.0          # (a fit to 1 cm of noise, from 1e-2 rad and 6.7 cm)
