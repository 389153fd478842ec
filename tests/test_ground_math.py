"""include/sls_ground_math.h on the host, as plain C99 — the very functions the kernels run, the 64 lanes emulated — against
the NumPy restatement (ground_ref.py) bit for bit, and cases worked by hand: bin numbers on axes and boundaries, an exact
lattice plane, a wall, the elevation / flatness rule, the noise skip, the point-count thresholds, and a synthetic street the
restatement must segment usefully."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ground_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "sls_ground_math.h"
/* in: M int32, SlsGroundParams, M x 3 floats
 * out: M bytes (label), M int32 (bin), BINS x 8 doubles, BINS x 4 int32, 8 uint32 */
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int32_t M;
    SlsGroundParams prm;
    if (argc != 3 || !in || !out || fread(&M, 4, 1, in) != 1 || fread(&prm, sizeof prm, 1, in) != 1) return 2;
    if (sizeof prm != 72 || SLS_GROUND_BINS != 504) return 3;
    float *xyz = malloc(12 * (size_t)M + 4);
    uint8_t *label = malloc((size_t)M + 4);
    int32_t *bin = malloc(4 * (size_t)M + 4), *info = malloc(16 * SLS_GROUND_BINS);
    double *planes = malloc(64 * SLS_GROUND_BINS);
    uint32_t status[8];
    if (fread(xyz, 12, (size_t)M, in) != (size_t)M) return 2;
    if (sls_ground_segment_host(M, xyz, &prm, label, bin, planes, info, status)) return 4;
    fwrite(label, 1, (size_t)M, out); fwrite(bin, 4, (size_t)M, out); fwrite(planes, 64, SLS_GROUND_BINS, out);
    fwrite(info, 16, SLS_GROUND_BINS, out); fwrite(status, 4, 8, out);
    fclose(in); fclose(out);
    return 0;
}
'''


def pack_params(p):
    return struct.pack("<7f4f4f3i", p["sensor_height"], p["min_range"], p["max_range"], p["th_seeds"], p["th_dist"],
                       p["uprightness_thr"], p["noise_margin"], *p["elevation_thr"], *p["flatness_thr"], p["num_lpr"],
                       p["num_iter"], p["num_min_pts"])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("ground_math")
    (d / "ground_math.c").write_text(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           str(d / "ground_math.c"), "-o", str(d / "ground_math"), "-lm"])
    return str(d / "ground_math")


def run_host(exe, tmp_path, points, **kw):
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    M, B = len(P), ref.BINS
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", M) + pack_params(ref.params(**kw)) + P.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    o = np.cumsum([0, M, 4 * M, 64 * B, 16 * B, 32])
    assert len(raw) == o[-1]
    return {"label": np.frombuffer(raw[o[0]:o[1]], np.uint8), "bin": np.frombuffer(raw[o[1]:o[2]], np.int32),
            "planes": np.frombuffer(raw[o[2]:o[3]], np.float64).reshape(B, 8),
            "info": np.frombuffer(raw[o[3]:o[4]], np.int32).reshape(B, 4), "status": np.frombuffer(raw[o[4]:o[5]], np.uint32)}


def same(got, want, what):
    for key in ("label", "bin", "info", "status"):
        assert np.array_equal(got[key], want[key]), f"{what}: {key} differ"
    bad = np.flatnonzero((got["planes"].view(np.uint64) != want["planes"].view(np.uint64)).any(1))
    assert bad.size == 0, f"{what}: planes differ in bins {bad[:5]}: {got['planes'][bad[:2]]} {want['planes'][bad[:2]]}"


def both(exe, tmp_path, points, what="by hand", **kw):
    want = ref.segment(points, **kw)
    same(run_host(exe, tmp_path, points, **kw), want, what)
    return want


@pytest.mark.parametrize("M", ref.SMALL)
def test_header_equals_the_restatement_small(exe, tmp_path, M):
    both(exe, tmp_path, ref.small_cloud(M), f"M={M}")
    both(exe, tmp_path, np.tile(np.array([[3.0, 0.5, -1.7]], np.float32), (M, 1)), f"M={M} identical")


def test_header_equals_the_restatement_one_bin(exe, tmp_path):
    want = both(exe, tmp_path, ref.one_bin(), "one bin")
    assert (want["info"][:, 0] == 3000).sum() == 1 and want["status"][1] > 1000


def test_header_equals_the_restatement_all_bins(exe, tmp_path):
    want = both(exe, tmp_path, ref.all_bins(), "all bins")
    assert want["status"][2] == 24 and want["status"][0] == 20000 - 60
    states = want["info"][:, 3]
    assert states[3] == ref.FEW and states[100] == ref.EMPTY and states[40] >= ref.DEGENERATE
    assert (states == ref.GROUND).sum() > 400


@pytest.mark.parametrize("kw", ref.VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_header_equals_the_restatement_parameters(exe, tmp_path, kw):
    a = both(exe, tmp_path, ref.bumpy(4000, 9), str(kw), **kw)
    # the parameter is read (eight rounds have converged to what three give: they are held against one round)
    b = ref.segment(ref.bumpy(4000, 9), **({"num_iter": 1} if kw == {"num_iter": 8} else {}))
    assert not np.array_equal(a["planes"], b["planes"])


def test_header_equals_the_restatement_street(exe, tmp_path):
    both(exe, tmp_path, ref.street_scan()[0], "street")


# ---- by hand -----------------------------------------------------------------------------------------------------------
def test_bin_numbers():
    p = ref.params()
    r = ref.boundaries(p)
    assert r[0] == p["min_range"] and r[4] == 80.0 and np.allclose(r[1:4], (12.3625, 22.025, 41.35), atol=1e-5)

    def b(x, y, z=0.0):
        return int(ref.bins(np.array([[x, y, z]], np.float32), p)[0])
    # the axes: diamond angle exactly 0, 1, 2, 3 -> the first sector of each quarter (16 sectors in zone 0: 0, 4, 8, 12)
    assert [b(5, 0), b(0, 5), b(-5, 0), b(0, -5)] == [0, 4, 8, 12]
    assert [b(5, -0.0), b(-0.0, 5)] == [0, 4]
    # zone 1 (32 sectors, base 32), zone 2 (54: 13.5 per quarter, base 160), zone 3 (32, base 376): ring 0
    assert [b(13, 0), b(0, 13), b(-13, 0), b(0, -13)] == [32, 40, 48, 56]
    assert [b(23, 0), b(0, 23), b(-23, 0), b(0, -23)] == [160, 173, 187, 200]       # floor(13.5), floor(27), floor(40.5)
    assert [b(42, 0), b(0, 42), b(-42, 0), b(0, -42)] == [376, 384, 392, 400]
    # the diagonals: a = 0.5, 1.5, 2.5, 3.5
    assert [b(4, 4), b(-4, 4), b(-4, -4), b(4, -4)] == [2, 6, 10, 14]
    # a diamond angle just below 4 is the last sector; sector boundaries: a = 0.25 exactly -> sector 1 of 16
    assert b(5, -1e-6) == 15 and b(3, 1) == 1 and b(3.0001, 1) == 0
    # rho exactly at the boundaries: r0 is inside, r4 is outside; r1 ... r3 as float64 are not float32 numbers, so the
    # float32 neighbours on either side fall into the two zones
    f = np.float32
    assert b(f(p["min_range"]), 0) == 0 and b(np.nextafter(f(p["min_range"]), f(0)), 0) == -1
    assert b(np.nextafter(f(80), f(0)), 0) == 376 + 3 * 32 and b(80, 0) == -1 and b(0, -80) == -1
    for k, (below, above) in enumerate(((16, 32), (32 + 3 * 32, 160), (160 + 3 * 54, 376))):
        edge = f(r[k + 1])
        lo, hi = (edge, np.nextafter(edge, f(100))) if float(edge) < r[k + 1] else (np.nextafter(edge, f(0)), edge)
        assert b(lo, 0) == below and b(hi, 0) == above, k
    # the ring boundary inside zone 0: (r0 + r1) / 2
    mid = (r[0] + r[1]) / 2
    assert b(mid - 1e-3, 0) == 0 and b(mid + 1e-3, 0) == 16
    # no bin: the origin, the sensor's own column, non-finite rows
    assert b(0, 0) == -1 and b(0.0, -0.0) == -1 and b(1, 1) == -1 and b(np.nan, 5) == -1 and b(5, np.inf) == -1
    assert b(5, 5, np.nan) == -1 and b(5, 5, -np.inf) == -1
    # concentric indices
    assert [ref.place(k) for k in (0, 15, 16, 31, 32, 159, 160, 375, 376, 503)] == \
        [(0, 0), (0, 0), (0, 1), (0, 1), (1, 2), (1, 5), (2, 6), (2, 9), (3, 10), (3, 13)]


def test_bin_numbers_in_the_header(exe, tmp_path):
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-90, 90, (20000, 3)), rng.integers(-20, 20, (5000, 3)).astype(np.float64),
                          [[0, 0, 0], [np.nan, 1, 1], [3, 1, 0], [2.7, 0, 0], [80, 0, 0]]]).astype(np.float32)
    got = run_host(exe, tmp_path, pts)
    assert np.array_equal(got["bin"], ref.bins(pts, ref.params()))
    got = run_host(exe, tmp_path, pts, max_range=33.0, min_range=0.5)
    assert np.array_equal(got["bin"], ref.bins(pts, ref.params(max_range=33.0, min_range=0.5)))


def test_horizontal_lattice_plane(exe, tmp_path):
    """z = -h exactly on a 0.5 m lattice: xz = yz = zz = 0 exactly, so only the (0, 1) rotation acts — every fitted bin has
    the normal (0, 0, 1), d = h and l0 = 0 exactly, and all its points are ground."""
    h = np.float32(1.723)
    g = np.arange(-160, 161) * 0.5
    pts = np.array([[x, y, h] for x in g for y in g], np.float32) * np.array([1, 1, -1], np.float32)
    res = both(exe, tmp_path, pts, "lattice")
    n = res["info"][:, 0]
    fitted = n >= 10
    assert fitted.sum() > 450
    assert np.all(res["info"][fitted, 3] == ref.GROUND) and np.all(res["info"][~fitted, 3] <= ref.FEW)
    assert np.all(res["planes"][fitted, :3] == (0.0, 0.0, 1.0)) and np.all(res["planes"][fitted, 3] == float(h))
    assert np.all(res["planes"][fitted, 4] == -float(h)) and np.all(res["planes"][fitted, 5] == 0.0)
    assert np.all(res["planes"][fitted, 6] > 0.0)
    inside = res["bin"] >= 0
    assert np.array_equal(res["label"] != 0, inside & fitted[np.maximum(res["bin"], 0)])
    assert np.all(res["info"][fitted, 2] == n[fitted]) and res["status"][1] == n[fitted].sum()


def test_vertical_wall_alone(exe, tmp_path):
    """A wall x = 15, alone in its bins: the plane's normal is horizontal -> NOT_UPRIGHT, nothing is ground."""
    res = both(exe, tmp_path, ref.wall(), "wall")
    used = res["info"][:, 0] >= 10
    assert used.sum() >= 2 and np.all(res["info"][used, 3] == ref.NOT_UPRIGHT) and res["status"][1] == 0
    assert not res["label"].any() and np.all(np.abs(res["planes"][used, 2]) < 1e-6)


def test_elevated_patch_rough_or_flat(exe, tmp_path):
    """Patchwork's slope rule in ring 0: a patch above -h + elevation_thr[0] is ground only if it is flat."""
    flat, rough, low = ref.elevated_patch("flat"), ref.elevated_patch("rough"), ref.elevated_patch("low")
    a, b = both(exe, tmp_path, flat, "elevated flat"), both(exe, tmp_path, rough, "elevated rough")
    k = int(a["bin"][0])
    assert np.all(a["bin"] == k) and ref.place(k)[1] == 0
    assert a["planes"][k, 4] == -1.0 > -1.723 + 0.523                              # the elevated branch is the one taken
    assert a["info"][k, 3] == ref.GROUND and a["label"].all() and a["planes"][k, 5] == 0.0
    assert b["info"][k, 3] == ref.ELEVATED_ROUGH and not b["label"].any()
    assert b["planes"][k, 5] / b["planes"][k, 5:].sum() >= 5e-4 and b["planes"][k, 2] > 0.99
    # the same rough patch at ground level passes: the rule reads the elevation first
    assert both(exe, tmp_path, low, "rough at ground level")["info"][k, 3] == ref.GROUND
    # ... and in ring 1 the bound is flatness_thr[1] = 7.25e-4 at elevation_thr[1]: jitter that is rough in ring 0
    # (flatness 5e-4 ... 7.25e-4) is still ground there
    mid = both(exe, tmp_path, ref.elevated_patch("ring1"), "elevated ring 1")
    k1 = int(mid["bin"][0])
    flatness = mid["planes"][k1, 5] / mid["planes"][k1, 5:].sum()
    assert ref.place(k1)[1] == 1 and mid["planes"][k1, 4] > -1.723 + 0.746 and 5e-4 < flatness < 7.25e-4
    assert mid["info"][k1, 3] == ref.GROUND and mid["label"].any()


def test_noise_skip_in_zone_0_only(exe, tmp_path):
    """Returns below -noise_margin * h (reflections under the road) are not seeds in zone 0; in zone 1 they are.
    The patch: 288 road points at -1.723 +- 0.01 and 12 at -2.6 +- 0.01, below -1.1 * 1.723 = -1.895."""
    near, far = both(exe, tmp_path, ref.noise_patch(5.0), "noise zone 0"), both(exe, tmp_path, ref.noise_patch(13.0), "noise zone 1")
    kn, kf = int(near["bin"][0]), int(far["bin"][0])
    assert ref.place(kn)[0] == 0 and ref.place(kf)[0] == 1 and np.all(near["bin"] == kn) and np.all(far["bin"] == kf)
    # zone 0: the 12 are skipped; lpr is the mean of the 20 lowest road points, about -1.73, so all 288 road points (<=
    # -1.713 < lpr + 0.5) are seeds; the 12 lie BELOW the road's plane, signed distance < th_dist, so they are candidates
    # of every later round and the plane moves by 12 / 300 of 0.88 m at the most
    assert near["info"][kn].tolist() == [300, 288, 300, ref.GROUND] and abs(near["planes"][kn, 4] + 1.723) < 0.05
    # zone 1: no skip; lpr is the mean of the 12 and the 8 lowest road points, (12 * -2.6 + 8 * -1.73) / 20 = -2.25 +-
    # 0.01; lpr + 0.5 = -1.75 lies below every road point (>= -1.733), so the seeds are the 12 alone; the road lies
    # 0.87 m above their plane, beyond th_dist, so the 12 stay the candidates; mean_z = -2.6 is not elevated: GROUND
    assert far["info"][kf].tolist() == [300, 12, 12, ref.GROUND] and abs(far["planes"][kf, 4] + 2.6) < 0.01
    assert far["label"].sum() == 12 and far["label"][:12].all()
    # with the margin raised out of reach zone 0 does what zone 1 does
    off = both(exe, tmp_path, ref.noise_patch(5.0), "noise margin off", noise_margin=5.0)
    assert off["info"][kn].tolist() == [300, 12, 12, ref.GROUND]


def test_point_count_thresholds(exe, tmp_path):
    ten = ref.ten_points()
    k = int(ref.bins(ten, ref.params())[0])
    nine = both(exe, tmp_path, ten[:9], "nine")
    assert nine["info"][k].tolist() == [9, 0, 0, ref.FEW] and not nine["label"].any() and not nine["planes"].any()
    full = both(exe, tmp_path, ten, "ten")
    assert full["info"][k, 0] == 10 and full["info"][k, 3] == ref.GROUND and full["label"].all()
    same_pt = both(exe, tmp_path, np.tile(ten[:1], (10, 1)), "ten identical")
    assert same_pt["info"][k].tolist() == [10, 10, 10, ref.DEGENERATE] and not same_pt["label"].any()
    assert not same_pt["planes"].any()
    assert both(exe, tmp_path, ten[:9], "nine of nine", num_min_pts=9)["info"][k, 3] == ref.GROUND
    assert both(exe, tmp_path, np.zeros((0, 3), np.float32), "empty")["status"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]


def test_street_precision_and_recall():
    """A condition of usefulness: at the defaults the restatement finds the street's ground with precision >= 0.9 and
    recall >= 0.9 over the points that have a bin."""
    pts, truth = ref.street_scan()
    res = ref.segment(pts)
    use = res["bin"] >= 0
    lab = res["label"][use] != 0
    tp = (lab & truth[use]).sum()
    precision, recall = tp / lab.sum(), tp / truth[use].sum()
    print(f"street 64 x 1024: {use.sum()} points with a bin, {truth[use].sum()} ground, precision {precision:.4f}, "
          f"recall {recall:.4f}, states {np.bincount(res['info'][:, 3], minlength=6).tolist()}")
    assert truth[use].sum() > 10000 and (~truth[use]).sum() > 5000
    assert precision >= 0.9 and recall >= 0.9
