"""The registration kernels (sls_aligner.hip) against the float64 checker at EXACT associations (GPU).

test_aligner.py compares one geometry at 3e-3, with slack on the inlier count because a float32 association "may
land on the neighbour".  Here the query pixels whose discrete decisions lie near a threshold are given up
beforehand (`ref.harden`, at most 12 % of them), so no pixel is excused afterwards: counts are equal as integers
and H, b, chi2 are as close to float64 as the checker's own float32 restatement is (x 3, not below 1e-5) — a bar
that comes from the checker alone.  Four small shapes reach every block-, wave- and seam-level path
(aligner_cases.py; what the case set covers is asserted on the CPU in test_aligner_checker.py), the normals kernel
is pinned on the same shapes, and the solve kernel is replayed on the host in float64 from the device's own system:
one step to the last float32 bit, both branches of the exponential, every status path."""
import math

import numpy as np
import pytest

import aligner_autograd_ref as autograd_ref
import aligner_cases as ac
from oracle import aligner_ref as ref

pytestmark = pytest.mark.gpu

DAMPING = float(np.float32(1e-6))          # GSAlignerParams.damping as the kernel reads it


def _proj(K):
    proj = np.eye(4, dtype=np.float32)
    proj[:3, :3] = K.T
    return proj


class Rig:
    """One GSAligner per shape: scan A as the reference (its normals from sls_aligner_normals), the query, the
    parameters and the stored reference normals replaced per case."""

    def __init__(self, shape, device):
        import torch
        from gsaligner import GSAligner, GSAlignerParams
        self.sc = sc = ac.scene(shape)
        self.device = device
        self.t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)
        self.proj = self.t(_proj(sc["K"]))
        self.defaults = GSAlignerParams(image_height=sc["H"], image_width=sc["W"])
        self.al = GSAligner(**self.defaults.__dict__)
        self.al.set_reference(self.t(sc["dA"])[None], self.t(sc["pA"].reshape(-1, 3)), self.proj)
        self.ref_d, self.ref_p, self.ref_n = self.al._ref
        self.n_hip = self.ref_n.cpu().numpy()

    def normals_of(self, depth, points):
        self.al.set_reference(self.t(depth)[None], self.t(points.reshape(-1, 3)), self.proj)
        n = self.al._ref[2].cpu().numpy()
        self.al._ref = (self.ref_d, self.ref_p, self.ref_n)
        return n

    def setup(self, pname, normals, q_depth, q_points, **more):
        """Parameters by name (+ overrides), the reference triple with `normals`, the query."""
        self.al.params = type(self.defaults)(**dict(self.defaults.__dict__, **dict(ac.PARAMS[pname], **more)))
        self.al._ref = (self.ref_d, self.ref_p, self.t(np.asarray(normals).reshape(-1, 3)))
        self.al.set_query(self.t(q_depth)[None], self.t(np.asarray(q_points).reshape(-1, 3)), self.proj)
        return self.al

    def linearize(self, T):
        import torch
        return self.al.linearize(torch.tensor(np.asarray(T), dtype=torch.float32)).cpu().numpy()

    def align(self, T):
        import torch
        Tr, fitness, info = self.al.align(torch.tensor(np.asarray(T), dtype=torch.float32, device=self.device))
        assert Tr.dtype == torch.float32 and Tr.shape == (4, 4)
        return Tr.cpu().numpy(), fitness, info


@pytest.fixture(scope="module")
def rigs(device):
    return {shape: Rig(shape, device) for shape in ac.SHAPES}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ulp32(x):
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), 1.0).astype(np.float32)).astype(np.float64)


def _same_sums(s_a, s_b, det):
    """Two linearisations of the same inputs: integers equal, sums equal up to the order of the double atomics."""
    assert s_a[28] == s_b[28] and s_a[29] == s_b[29]
    dev = ac.scale_free(s_a[:30], det, s_b[:30])
    assert max(dev.values()) <= 1e-12, dev


# ---------------------------------------------------------------------------------------------- normals kernel
@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_normals_kernel_mask_and_values(rigs, shape):
    rig, sc = rigs[shape], ac.scene(shape)
    H, W, wrap = sc["H"], sc["W"], sc["cam"]["wrap"]
    for name, d, p in (("A", sc["dA"], sc["pA"]), ("B", sc["dB"], sc["pB"])):
        n_hip = rig.normals_of(d, p).reshape(H, W, 3).astype(np.float64)
        n_ref = ref.normals(sc["cam"], d, p, 0.5)
        mask = np.abs(n_hip).sum(-1) > 0
        assert np.array_equal(mask, np.abs(n_ref).sum(-1) > 0), "the checker's validity mask"
        assert not mask[0].any() and not mask[-1].any(), "rows 0 and H-1"
        if wrap:
            assert mask[:, 0].any() and mask[:, -1].any(), "a wrapping camera has normals in its first and last column"
        else:
            assert not mask[:, 0].any() and not mask[:, -1].any(), "columns 0 and W-1 of a camera that does not wrap"
        holes = np.argwhere(d <= 0.5)
        assert len(holes) >= 2
        for r, c in holes:                                   # the hole and its four neighbours
            for rr, cc in ((r, c), (r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                cc = cc % W if wrap else cc
                if 0 <= rr < H and 0 <= cc < W:
                    assert not mask[rr, cc], (name, r, c, rr, cc)
        err = float(np.abs(n_hip - n_ref).max())
        facing = float((n_hip * p.astype(np.float64)).sum(-1).max())
        print(f"\n[aligner parity] normals {shape} {name}: {int(mask.sum())} of {H * W}, max error {err:.2e}, max n.p {facing:.2e}")
        assert mask.sum() >= 5
        assert err <= 1e-5                                   # (the float32 restatement: 1.8e-7)
        assert facing <= 0.0, "normals face the sensor"
        assert np.abs(np.linalg.norm(n_hip[mask], axis=-1) - 1.0).max() <= 1e-6
    # the pixel at exactly depth_min is a hole of scan A: strict gate
    r0, c0 = sc["pinned"]
    assert sc["dA"][r0, c0] == np.float32(0.5)
    nA = rig.n_hip.reshape(H, W, 3)
    for rr, cc in ((r0, c0), (r0 - 1, c0), (r0 + 1, c0), (r0, c0 - 1), (r0, c0 + 1)):
        assert not nA[rr, cc].any()


# -------------------------------------------------------------------------- one linearisation, exact associations
@pytest.mark.parametrize("pname", list(ac.PARAMS))
@pytest.mark.parametrize("shape", list(ac.SHAPES))
def test_linearisation_at_exact_associations(rigs, shape, pname):
    rig, sc = rigs[shape], ac.scene(shape)
    for ti in range(ac.N_POSES):
        for nset in ac.NORMAL_SETS:
            c = ac.case(shape, pname, ti, nset, kernel_normals=rig.n_hip)
            s64, det, bars = c["s64"], c["det"], c["bars"]
            assert c["share"] <= ac.HARDEN_CAP, c["share"]
            assert all(v <= 1e-3 for v in bars.values()), ("badly conditioned case", bars)
            rig.setup(pname, c["normals"], c["q_depth"], sc["pB"])
            s_hip = rig.linearize(c["T"])
            dev = ac.scale_free(s64, det, s_hip[:30])
            print(f"\n[aligner parity] {c['id']}: inliers {int(s_hip[28])}/{int(s64[28])} valid {int(s_hip[29])}/{int(s64[29])} "
                  f"removed {c['share']:.4f} H {dev['H']:.2e} (bar {bars['H']:.2e}) b/S {dev['b']:.2e} (bar {bars['b']:.2e}) "
                  f"chi2 {dev['chi2']:.2e} (bar {bars['chi2']:.2e})")
            assert s_hip.shape == (32,) and s_hip[30] == 0 and s_hip[31] == 0
            assert int(s_hip[28]) == s_hip[28] == s64[28], "inliers"
            assert int(s_hip[29]) == s_hip[29] == s64[29], "valid query pixels"
            for k in ("H", "b", "chi2"):
                assert dev[k] <= bars[k], (c["id"], k, dev[k], bars[k])
            _same_sums(s_hip, rig.linearize(c["T"]), det)


@pytest.mark.parametrize("shape", ["24x200", "9x131"])
def test_hand_placed_query_pixels_meet_the_gates_nothing_else_reaches(rigs, shape):
    """At T = identity (no rounding in the pose): a point on the sensor's axis (rxy == 0) counts as valid and is no
    inlier; a point nearer than depth_min behind a valid depth likewise; points one and a half pixels beyond every
    side of the image are rejected (on the wrapping camera the columns come back in)."""
    rig, sc = rigs[shape], ac.scene(shape)
    H, W, cam = sc["H"], sc["W"], sc["cam"]
    c = ac.case(shape, "defaults", 0, "filled", kernel_normals=rig.n_hip)
    qd, qp = c["q_depth"].copy().reshape(-1), sc["pB"].copy().reshape(-1, 3)

    def at(col, row, rng=5.0):                               # the point that projects to the middle of pixel (row, col)
        az, el = (col - 0.5 - cam["cx"]) / cam["fx"], (row - 0.5 - cam["cy"]) / cam["fy"]
        return rng * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])

    placed = {"axis": (np.array([0.0, 0.0, 5.0]), 5.0), "near": (np.array([0.3, 0.0, 0.0]), 2.0),
              "left": (at(-2, H // 2), 5.0), "right": (at(W + 1, H // 2), 5.0),
              "above": (at(W // 2, -1), 5.0), "below": (at(W // 2, H), 5.0)}
    spots = np.flatnonzero(c["det"]["ok"])[:: max(1, int(c["det"]["ok"].sum()) // len(placed))][:len(placed)]
    assert len(spots) == len(placed)
    for k, (point, depth) in zip(spots, placed.values()):
        qp[k], qd[k] = point, depth
    args = (cam, c["prm"], sc["dA"], sc["pA"], c["normals"], qd, qp, c["T"])
    s64, det = ref.linearize(*args, details=True)
    where = dict(zip(placed, spots))
    assert det["valid"][spots].all() and s64[29] == c["s64"][29]
    assert det["rxy"][where["axis"]] == 0.0 and det["rho"][where["near"]] < 0.5
    assert det["row"][where["above"]] == -1 and det["row"][where["below"]] == H
    gone = ["axis", "near", "above", "below"] + ([] if cam["wrap"] else ["left", "right"])
    assert not det["ok"][[where[k] for k in gone]].any()
    if cam["wrap"]:
        assert det["j"][where["left"]] == (H // 2) * W + W - 2 and det["j"][where["right"]] == (H // 2) * W + 1
    else:
        assert det["col"][where["left"]] == -2 and det["col"][where["right"]] == W + 1
        assert s64[28] == c["s64"][28] - len(placed)
    dev32 = ac.scale_free(s64, det, ref.linearize(*args, dtype=np.float32))
    bars = {k: max(ac.RTOL, 3.0 * v) for k, v in dev32.items()}
    assert all(v <= 1e-3 for v in bars.values()), bars
    rig.setup("defaults", c["normals"], qd, qp)
    s_hip = rig.linearize(c["T"])
    dev = ac.scale_free(s64, det, s_hip[:30])
    print(f"\n[aligner parity] hand-placed {shape}: inliers {int(s_hip[28])}/{int(s64[28])} valid {int(s_hip[29])}/{int(s64[29])} {dev} bars {bars}")
    assert s_hip[28] == s64[28] and s_hip[29] == s64[29]
    for k in ("H", "b", "chi2"):
        assert dev[k] <= bars[k], (k, dev[k], bars[k])


# ------------------------------------------------------------------------------- the solve kernel, status paths
def _pair(rig, pair):
    """-> (parameter set, query depth hardened at identity, query points, the checker's details there)."""
    sc = rig.sc
    if pair == "A_vs_B":
        c = ac.case(sc["shape"], "defaults", 0, "kernel", kernel_normals=rig.n_hip)
        return "defaults", c["q_depth"], sc["pB"], c["s64"], c["det"]
    pname = "defaults" if pair == "A_vs_A" else "no_range"
    prm = ac.ref_params(pname)
    qd, share = ref.harden(sc["cam"], prm, sc["dA"], sc["pA"], rig.n_hip, sc["dA"], sc["pA"], np.eye(4))
    assert share <= ac.HARDEN_CAP
    s64, det = ref.linearize(sc["cam"], prm, sc["dA"], sc["pA"], rig.n_hip, qd, sc["pA"], np.eye(4), details=True)
    return pname, qd, sc["pA"], s64, det


def _check_statistics(rig, T_ret, fitness, info):
    """The result's statistics are those of a linearisation at the returned pose."""
    s = rig.linearize(T_ret)
    assert info["inliers"] == s[28] and info["valid_query"] == s[29]
    chi2_32 = np.float32(s[27])
    assert abs(info["chi2"] - float(chi2_32)) <= 2 * float(np.spacing(chi2_32)), (info["chi2"], s[27])
    fit_32 = np.float32(s[28] / s[29])
    assert abs(fitness - float(fit_32)) <= float(np.spacing(fit_32)), (fitness, s[28] / s[29])
    return s


@pytest.mark.parametrize("pair", ["A_vs_B", "A_vs_A", "A_vs_A_no_range"])
@pytest.mark.parametrize("shape", ["16x256", "9x131"])
def test_one_step_of_the_solve_kernel_replayed_in_float64(rigs, shape, pair):
    """One Gauss-Newton step from the device's own system: xi = solve(H + damping I, -b) and exp(xi) T0 on the host
    in float64 give the returned pose to the last float32 bit (Cholesky and LU differ by cond * 2^-52; the kernel
    casts once)."""
    import torch
    rig = rigs[shape]
    pname, qd, qp, s64, det = _pair(rig, pair)
    rig.setup(pname, rig.n_hip, qd, qp, num_iterations=1)
    T0 = np.eye(4)
    s0 = rig.linearize(T0)
    assert s0[28] == s64[28] >= 64 and s0[29] == s64[29]
    Hm = np.zeros((6, 6))
    Hm[np.triu_indices(6)] = s0[:21]
    Hm = Hm + Hm.T - np.diag(np.diag(Hm))
    xi = np.linalg.solve(Hm + DAMPING * np.eye(6), -s0[21:27])
    th = float(np.linalg.norm(xi[3:]))
    T1 = ref.se3_exp(xi) @ T0
    # the closed form against a matrix exponential that knows nothing of Rodrigues' formula
    T1_series = torch.linalg.matrix_exp(autograd_ref._hat(torch.tensor(xi))).numpy() @ T0
    assert np.abs(T1 - T1_series).max() <= 1e-14
    T_ret, fitness, info = rig.align(T0)
    print(f"\n[aligner parity] solve {shape} {pair}: theta {th:.3e} |xi| {np.linalg.norm(xi):.3e} "
          f"pose error [ulp] {float((np.abs(T_ret.astype(np.float64) - T1.astype(np.float32)) / _ulp32(T1)).max()):.2f}")
    assert info["iterations"] == 1
    if pair == "A_vs_A_no_range":
        # every residual is exactly 0: nothing moves, bit for bit
        assert not s0[21:28].any() and th == 0.0
        assert np.array_equal(_bits(T_ret), _bits(np.eye(4)))
        assert info["last_step"] == 0.0 and info["chi2"] == 0.0
        assert fitness == float(np.float32(s64[28] / s64[29]))
    else:
        assert th > 1e-3 if pair == "A_vs_B" else 0.0 < th < 1e-6, th      # the general / the small-angle branch
        assert np.all(np.abs(T_ret.astype(np.float64) - T1.astype(np.float32)) <= _ulp32(T1)), (T_ret, T1)
        assert np.array_equal(T_ret[3], [0, 0, 0, 1])
        step = np.float32(np.linalg.norm(xi))
        assert abs(info["last_step"] - float(step)) <= float(np.spacing(step))
    _check_statistics(rig, T_ret, fitness, info)
    _same_sums(s0, rig.linearize(T0), det)                              # the accumulators were cleared


def test_status_paths_leave_the_pose_alone(rigs):
    """num_iterations == 0, too few inliers, a system that is not positive definite: normal returns, the pose
    bit for bit the float32 start, the statistics those of a linearisation there."""
    rig = rigs["9x131"]
    pname, qd, qp, s64, det = _pair(rig, "A_vs_B")
    T0 = ac.f32(ref.se3_exp(np.array([0.02, -0.01, 0.005, 0.001, -0.002, 0.003])))
    rig.setup(pname, rig.n_hip, qd, qp)
    s0 = rig.linearize(T0)
    assert s0[28] >= 64
    det = ref.linearize(rig.sc["cam"], ac.ref_params(pname), rig.sc["dA"], rig.sc["pA"], rig.n_hip, qd, qp, T0,
                        details=True)[1]                                 # (the scale of b at T0)

    def run(**more):
        rig.setup(pname, rig.n_hip, qd, qp, **more)
        T_ret, fitness, info = rig.align(T0)
        assert np.array_equal(_bits(T_ret), _bits(T0)), more
        s = _check_statistics(rig, T_ret, fitness, info)
        _same_sums(s0, s, det)
        assert fitness == float(np.float32(s0[28] / s0[29]))
        return info

    info = run(num_iterations=0)
    assert info["iterations"] == 0 and info["last_step"] == 0.0
    info = run(num_iterations=3, min_inliers=int(s0[28]) + 1)
    assert info["iterations"] == 3 and info["last_step"] == 0.0
    info = run(num_iterations=2, damping=-1e30)                         # the diagonal goes negative: Cholesky refuses
    assert info["iterations"] == 2 and info["last_step"] == -1.0
    # with min_inliers AT the count the step is taken
    rig.setup(pname, rig.n_hip, qd, qp, num_iterations=1, min_inliers=int(s0[28]))
    T_ret, _, info = rig.align(T0)
    assert info["iterations"] == 1 and info["last_step"] > 0 and not np.array_equal(_bits(T_ret), _bits(T0))
    rig.setup(pname, rig.n_hip, qd, qp)
    _same_sums(s0, rig.linearize(T0), det)
