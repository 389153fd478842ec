"""The case set of the registration parity tests (test_aligner_checker.py on the CPU, test_aligner_parity.py on
the GPU): four small range images of the room of test_aligner.py with holes, four parameter sets, three poses,
two sets of reference normals; the bars, which come from the checker alone; and what a case covers."""
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import aligner_ref as ref                      # noqa: E402
from splat_loam_amd import synth                           # noqa: E402
from test_aligner import pose_of, room_scan                # noqa: E402

# name -> (H, W, horizontal field of view in degrees)
SHAPES = {
    "16x256": (16, 256, 360.0),      # P = 4096: 16 whole blocks, wrapping
    "9x131": (9, 131, 360.0),        # P = 1179: the last block has 155 live threads, W odd
    "24x200": (24, 200, 120.0),      # not wrapping, 18.75 blocks, columns fall off both sides
    "5x13": (5, 13, 360.0),          # P = 65: one block, the second wave has one live lane
}
# name -> fields of GSAlignerParams that differ from the defaults
PARAMS = {
    "defaults": {},
    "no_range": dict(range_weight=0.0),
    "depth_max9": dict(depth_max=9.0),
    "tight": dict(max_distance=0.3, max_angle_deg=60.0),
}
NORMAL_SETS = ("kernel", "filled")
N_POSES = 3
HARDEN_CAP = 0.12
RTOL = 1e-5


def ref_params(name, **more):
    kw = dict(PARAMS[name], **more)
    if "max_angle_deg" in kw:
        kw["min_cos_angle"] = math.cos(math.radians(kw.pop("max_angle_deg")))
    return ref.Params(**kw)


def f32(T):
    return np.asarray(T, np.float64).astype(np.float32).astype(np.float64)


def _holes(depth, points, seed):
    """3 % of the image without a return: depth 0 and the point at the origin."""
    d, p = depth.copy(), points.copy()
    rng = np.random.default_rng(seed)
    idx = rng.choice(d.size, size=max(1, round(0.03 * d.size)), replace=False)
    d.reshape(-1)[idx] = 0
    p.reshape(-1, 3)[idx] = 0
    return d, p


@functools.lru_cache(maxsize=None)
def scene(shape):
    H, W, hfov = SHAPES[shape]
    K = synth.spherical_K(H, W, hfov_deg=hfov).astype(np.float64)
    A, B = pose_of([0.0, 0.0, 0.0]), pose_of([0.35, -0.22, 0.06], yaw_deg=3.0, pitch_deg=0.4)
    dA, pA = _holes(*room_scan(K, H, W, A), seed=11)
    dB, pB = _holes(*room_scan(K, H, W, B), seed=12)
    prm = ref.Params()
    # one interior reference pixel at exactly depth_min: invalid (the gates are strict)
    r0, c0 = H // 2, W // 3
    assert dA[r0, c0] > prm.depth_min and 0 < r0 < H - 1 and 0 < c0 < W - 1
    pA[r0, c0] *= np.float32(prm.depth_min) / dA[r0, c0]
    dA[r0, c0] = prm.depth_min
    Tgt = np.linalg.inv(A) @ B
    poses = (np.eye(4), f32(Tgt), f32(ref.se3_exp(np.array([0.1, -0.05, 0.02, 0.004, -0.003, 0.02])) @ Tgt))
    return dict(shape=shape, K=K, H=H, W=W, cam=ref.cam_of(K, H, W), dA=dA, pA=pA, dB=dB, pB=pB, Tgt=Tgt, poses=poses,
                pinned=(r0, c0))


def filled(normals, depth, points, depth_min):
    """Every zero normal at a valid pixel replaced by -p/|p| (float32): border rows, and the border columns of
    a camera that does not wrap, can then be associated."""
    n = np.array(normals, np.float32).reshape(-1, 3)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    m = (np.abs(n).sum(1) == 0) & (np.asarray(depth).reshape(-1) > depth_min)
    n[m] = -p[m] / np.linalg.norm(p[m], axis=1, keepdims=True)
    return n


def scale_free(s, det, other):
    """Deviation of the system `other` from `s` in the norms of DESIGN.md section 7: H by max|H|, b per component
    by S_k = sum_i |w J_ik e_i|, chi2 relative (0 where the scale is 0 and the two agree)."""
    def over(d, scale):
        d, scale = np.asarray(d, np.float64), np.asarray(scale, np.float64)
        return float(np.max(np.where(d == 0, 0.0, d / np.where(scale > 0, scale, 1e-300)), initial=0.0))
    return dict(H=over(np.abs(other[:21] - s[:21]), np.abs(s[:21]).max()),
                b=over(np.abs(other[21:27] - s[21:27]), det["S_b"]),
                chi2=over(abs(other[27] - s[27]), abs(s[27])))


@functools.lru_cache(maxsize=None)
def _case(shape, pname, ti, nset, normals_key):
    sc = scene(shape)
    prm = ref_params(pname)
    n = _NORMALS[normals_key]
    if nset == "filled":
        n = filled(n, sc["dA"], sc["pA"], prm.depth_min)
    T = sc["poses"][ti]
    qd, share = ref.harden(sc["cam"], prm, sc["dA"], sc["pA"], n, sc["dB"], sc["pB"], T)
    args = (sc["cam"], prm, sc["dA"], sc["pA"], n, qd, sc["pB"], T)
    s64, det = ref.linearize(*args, details=True)
    s32 = ref.linearize(*args, dtype=np.float32)
    dev32 = scale_free(s64, det, s32)
    bars = {k: max(RTOL, 3.0 * v) for k, v in dev32.items()}
    return dict(scene=sc, prm=prm, T=T, normals=n, q_depth=qd, share=share, args=args, s64=s64, det=det, s32=s32,
                dev32=dev32, bars=bars, id=f"{shape}-{pname}-T{ti}-{nset}")


_NORMALS = {}


def case(shape, pname, ti, nset, kernel_normals=None):
    """One hardened case with its float64 system, details, float32 system and bars.  `kernel_normals`: the (P,3)
    float32 normals of scan A as the device produced them; without, the checker's float32 restatement."""
    sc = scene(shape)
    if kernel_normals is None:
        key = (shape, "checker")
        if key not in _NORMALS:
            _NORMALS[key] = ref.normals(sc["cam"], sc["dA"], sc["pA"], ref.Params().depth_min,
                                        dtype=np.float32).reshape(-1, 3)
    else:
        key = (shape, "device")
        _NORMALS[key] = np.asarray(kernel_normals, np.float32).reshape(-1, 3)
    return _case(shape, pname, ti, nset, key)


def all_ids():
    return [(sh, pn, ti, ns) for sh in SHAPES for pn in PARAMS for ti in range(N_POSES) for ns in NORMAL_SETS]


def coverage(c):
    """What the checker's details of case `c` reach: name -> number of query pixels."""
    sc, prm, d = c["scene"], c["prm"], c["det"]
    H, W, wrap = sc["H"], sc["W"], sc["cam"]["wrap"]
    qd = np.asarray(c["q_depth"], np.float64).reshape(-1)
    ok, j = d["ok"], d["j"]
    projected = d["valid"] & (d["rho"] > prm.depth_min) & (d["rxy"] > 1e-6)
    col_in = np.ones_like(ok) if wrap else (d["col"] >= 0) & (d["col"] < W)
    row_in = (d["row"] >= 0) & (d["row"] < H)
    seen = j >= 0
    ref_valid = seen & (d["dr"] > prm.depth_min)
    ref_near = ref_valid & (d["dr"] <= prm.depth_max)
    with np.errstate(invalid="ignore"):
        near = d["dist2"] <= prm.max_distance ** 2
        facing = d["cosang"] >= prm.min_cos_angle
    gated = ref_near & d["has_n"]
    c_w = np.where(seen, j % W, -1)
    r_w = np.where(seen, j // W, -1)
    # an interior inlier whose image gradient is zero has an invalid neighbour (the scene has no flat range)
    inner_c = ok & (r_w >= 0) & (wrap | ((c_w > 0) & (c_w < W - 1)))
    inner_r = ok & (r_w > 0) & (r_w < H - 1)
    rd = np.asarray(sc["dA"], np.float64)
    cl, cr = (c_w - 1) % W, (c_w + 1) % W
    hole_lr = (rd[np.clip(r_w, 0, H - 1), cl] <= prm.depth_min) | (rd[np.clip(r_w, 0, H - 1), cr] <= prm.depth_min)
    hole_ud = (rd[np.clip(r_w - 1, 0, H - 1), np.clip(c_w, 0, W - 1)] <= prm.depth_min) | \
              (rd[np.clip(r_w + 1, 0, H - 1), np.clip(c_w, 0, W - 1)] <= prm.depth_min)
    cnt = lambda m: int(np.count_nonzero(m))
    return {
        "query beyond depth_max": cnt(qd > prm.depth_max),
        "column off the image, left": cnt(projected & ~col_in & row_in & (d["col"] < 0)),
        "column off the image, right": cnt(projected & ~col_in & row_in & (d["col"] >= W)),
        "row off the image": cnt(projected & col_in & ~row_in),
        "reference invalid": cnt(seen & ~ref_valid),
        "reference beyond depth_max": cnt(ref_valid & ~ref_near & d["has_n"]),
        "reference normal zero": cnt(ref_near & ~d["has_n"]),
        "max_distance alone": cnt(gated & ~near & facing),
        "min_cos_angle alone": cnt(gated & near & ~facing),
        "inlier across the seam": cnt(ok & ((d["col"] < 0) | (d["col"] >= W))) if wrap else 0,
        "inlier at c == 0": cnt(ok & (c_w == 0)),
        "inlier at c == W-1": cnt(ok & (c_w == W - 1)),
        "inlier at c == 0, not wrapping": 0 if wrap else cnt(ok & (c_w == 0)),
        "inlier at c == W-1, not wrapping": 0 if wrap else cnt(ok & (c_w == W - 1)),
        "inlier at r == 0": cnt(ok & (r_w == 0)),
        "inlier at r == H-1": cnt(ok & (r_w == H - 1)),
        "gu zero beside a hole": cnt(inner_c & hole_lr & (d["gu"] == 0)),
        "gv zero beside a hole": cnt(inner_r & hole_ud & (d["gv"] == 0)),
        "gu non-zero": cnt(ok & (d["gu"] != 0)),
        "gv non-zero": cnt(ok & (d["gv"] != 0)),
        "|e_g| <= huber_delta": cnt(ok & (np.abs(d["e_g"]) <= prm.huber_delta)),
        "|e_g| > huber_delta": cnt(ok & (np.abs(d["e_g"]) > prm.huber_delta)),
        "|e_r| <= range_huber": cnt(ok & (np.abs(d["e_r"]) <= prm.range_huber)) if prm.range_weight > 0 else 0,
        "|e_r| > range_huber": cnt(ok & (np.abs(d["e_r"]) > prm.range_huber)) if prm.range_weight > 0 else 0,
    }
