"""Host side of the two-cloud nearest-neighbour query (sls_nn_query, sls_nn_stats, splat_loam_amd/evaluation.py):
scratch sizes, every argument error (all checked before a launch: no device needed), the point-cloud PLY reader, the
refusal of CPU tensors and the NumPy restatement against a KD-tree."""
import numpy as np
import pytest
import torch

import nn_ref
from splat_loam_amd import _abi, evaluation, ply_io

E_ARG, E_SCRATCH = -1, -3
FAKE = 0x10000          # a non-null, 256-byte aligned address that is never dereferenced: the checks come first
STATS_BYTES = 32768     # SLS_NN_STATS_SCRATCH_BYTES


def test_scratch_bytes_edge_cases():
    lib = _abi.lib()
    assert lib.sls_nn_scratch_bytes(0, 10) == 0 and lib.sls_nn_scratch_bytes(-1, 10) == 0
    assert lib.sls_nn_scratch_bytes(10, -1) == 0
    for Mt, Mq in ((1, 0), (1, 1), (255, 100), (256, 256), (257, 129), (6000, 4000), (1000, 2000000), (2000000, 1000)):
        n = lib.sls_nn_scratch_bytes(Mt, Mq)
        assert n % 256 == 0 and n >= STATS_BYTES                        # the query's scratch serves sls_nn_stats
        assert n >= lib.sls_knn_scratch_bytes(Mt)                       # the target's index ...
        assert n >= 32 * Mt + 32 * Mq                                   # ... + codes, indices (x2) and float4 per point
        assert n >= lib.sls_sort_scratch_bytes(max(Mt, Mq))             # the sorter runs over the larger cloud too
    assert lib.sls_nn_scratch_bytes(1000, 500) <= lib.sls_nn_scratch_bytes(1000, 501)
    assert lib.sls_nn_scratch_bytes(1000, 500) <= lib.sls_nn_scratch_bytes(1001, 500)
    header = open(_abi.LIB_PATH.replace("splat_loam_amd/libsls_hip.so", "include/sls_abi.h")).read()
    assert f"#define SLS_NN_STATS_SCRATCH_BYTES {STATS_BYTES}" in header


def test_nn_query_argument_errors_need_no_device():
    lib = _abi.lib()
    need = lib.sls_nn_scratch_bytes(100, 50)

    def call(Mt=100, t=FAKE, Mq=50, q=FAKE, d=FAKE, i=FAKE, s=FAKE, n=need):
        return lib.sls_nn_query(Mt, t, Mq, q, d, i, s, n, None)
    assert call(Mt=0) == E_ARG and b"Mt < 1" in lib.sls_last_error()
    assert call(Mt=-5) == E_ARG
    assert call(Mt=0, Mq=0) == E_ARG                                    # an empty target is an error even with no query
    assert call(Mq=-1) == E_ARG and b"Mq" in lib.sls_last_error()
    assert call(Mq=0, t=None, q=None, d=None, i=None, s=None, n=0) == 0     # no query: success, nothing touched
    for kw in ({"t": None}, {"q": None}, {"d": None}, {"s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    for off in (1, 4, 16, 128, 255):
        assert call(s=FAKE + off) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=need - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(n=0) == E_SCRATCH
    assert call(i=None, n=need - 1) == E_SCRATCH                        # (a null index is legal: the size check is reached)
    with pytest.raises(RuntimeError, match="scratch too small"):
        _abi.check(call(n=need - 1), "sls_nn_query")


def test_nn_stats_argument_errors_need_no_device():
    lib = _abi.lib()

    def call(M=10, d=FAKE, trunc=0.5, thr=0.2, inc=0, out=FAKE, s=FAKE, n=STATS_BYTES):
        return lib.sls_nn_stats(M, d, trunc, thr, inc, out, s, n, None)
    assert call(M=-1) == E_ARG and b"negative M" in lib.sls_last_error()
    for kw in ({"d": None}, {"out": None}, {"s": None}, {"M": 0, "out": None}, {"M": 0, "s": None}):
        assert call(**kw) == E_ARG and b"null pointer" in lib.sls_last_error(), kw
    assert call(trunc=float("nan")) == E_ARG and call(thr=float("nan")) == E_ARG
    assert call(s=FAKE + 64) == E_ARG and b"aligned" in lib.sls_last_error()
    assert call(n=STATS_BYTES - 1) == E_SCRATCH and b"scratch too small" in lib.sls_last_error()
    assert call(M=0, d=None, n=0) == E_SCRATCH                          # M == 0 still writes the four words: it needs its scratch


def _write_ply(path, header_props, rec):
    header = "ply\nformat binary_little_endian 1.0\ncomment a scan export\nelement vertex %d\n" % len(rec)
    header += "".join(f"property {k} {n}\n" for k, n in header_props)
    header += "element face 0\nproperty list uchar int vertex_indices\nend_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def test_point_cloud_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.normal(0, 30, (1237, 3)).astype(np.float32)
    nrm = rng.normal(0, 1, (1237, 3)).astype(np.float32)
    ply_io.save_point_cloud(tmp_path / "a.ply", pts, nrm)
    p2, n2 = ply_io.load_point_cloud(tmp_path / "a.ply")
    assert p2.dtype == np.float32 and np.array_equal(p2, pts) and np.array_equal(n2, nrm)
    ply_io.save_point_cloud(tmp_path / "t.ply", torch.from_numpy(pts), torch.from_numpy(nrm))      # tensors too
    assert np.array_equal(ply_io.load_point_cloud(tmp_path / "t.ply")[0], pts)
    # double-typed coordinates, no normals, an extra property in between, an (empty) face element behind
    pd = rng.normal(0, 30, (311, 3))
    rec = np.empty(311, np.dtype([("x", "<f8"), ("y", "<f8"), ("intensity", "u1"), ("z", "<f8")]))
    rec["x"], rec["y"], rec["z"], rec["intensity"] = pd[:, 0], pd[:, 1], pd[:, 2], 7
    _write_ply(tmp_path / "d.ply", [("double", "x"), ("double", "y"), ("uchar", "intensity"), ("double", "z")], rec)
    p3, n3 = ply_io.load_point_cloud(tmp_path / "d.ply")
    assert n3 is None and p3.dtype == np.float32 and np.array_equal(p3, pd.astype(np.float32))
    # only two of the three normal components: no normals
    rec = np.zeros(5, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4")]))
    _write_ply(tmp_path / "n.ply", [("float", n) for n in ("x", "y", "z", "nx", "ny")], rec)
    assert ply_io.load_point_cloud(tmp_path / "n.ply")[1] is None
    # an empty cloud, a missing coordinate, integer coordinates, an ASCII file
    ply_io.save_point_cloud(tmp_path / "e.ply", np.zeros((0, 3)), np.zeros((0, 3)))
    assert ply_io.load_point_cloud(tmp_path / "e.ply")[0].shape == (0, 3)
    _write_ply(tmp_path / "m.ply", [("float", "x"), ("float", "y")], np.zeros(2, np.dtype([("x", "<f4"), ("y", "<f4")])))
    with pytest.raises(ValueError, match="no property z"):
        ply_io.load_point_cloud(tmp_path / "m.ply")
    _write_ply(tmp_path / "i.ply", [("int", "x"), ("int", "y"), ("int", "z")],
               np.zeros(2, np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4")])))
    with pytest.raises(ValueError, match="not float or double"):
        ply_io.load_point_cloud(tmp_path / "i.ply")
    (tmp_path / "ascii.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="little-endian"):
        ply_io.load_point_cloud(tmp_path / "ascii.ply")


def test_evaluation_refuses_cpu_tensors():
    a, b = torch.zeros((4, 3)), torch.ones((5, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.nearest(a, b)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.cloud_metrics(a, b)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.crop_union_mask(a, b)
    with pytest.raises(RuntimeError, match="device tensor"):
        evaluation.nearest(a.numpy(), b)


def _order_terms(M):
    """the float64 terms (0.0 where an entry does not count) of the three sums the device tests pin at size M"""
    import signdist_ref
    d2, sd = nn_ref.stats_order_dist2(M), nn_ref.stats_order_signed(M)
    out = []
    for inc in (False, True):
        d, counted = nn_ref._stats_terms(d2, 0.5, inc)
        out.append(np.where(counted, d.astype(np.float64), 0.0))
    out.append(np.where(np.abs(sd) < np.float32(0.5), sd.astype(np.float64), 0.0))
    assert signdist_ref.stats_device_order(sd, 0.5)[2] == nn_ref.device_sum(out[2])
    return out


@pytest.mark.parametrize("M", nn_ref.STATS_ORDER_SIZES)
def test_restated_device_sum_is_a_sum(M):
    """nn_ref.device_sum, the order the device tests pin bit for bit, on those tests' own terms against the exactly
    rounded sum (math.fsum), to 1e-12 of the sum: every term passes through fewer than 30 additions (2 strided, 6 + 3 in
    the block, 4 + 6 + 3 in the final block), so the two differ by less than 30 * 2^-53 of the sum of magnitudes, which
    is the sum itself for the distances and, asserted, at most 10 times its magnitude for the signed terms: 3.4e-14."""
    import math
    assert nn_ref.device_sum(np.zeros(0)) == 0.0
    for v in _order_terms(M):
        exact = math.fsum(v)
        assert math.fsum(np.abs(v)) <= 10.0 * abs(exact)
        assert abs(nn_ref.device_sum(v) - exact) <= 1e-12 * abs(exact)


@pytest.mark.parametrize("M", [m for m in nn_ref.STATS_ORDER_SIZES if m > 1])
def test_order_tests_data_tells_orders_apart(M):
    """What makes the device tests a pin of the ORDER: on their own terms (nn_ref.STATS_ORDER_SEEDS) the documented order
    gives other bits than NumPy's sum, than a left-to-right sum, than the documented order with its butterfly run upwards
    (offsets 1 .. 32) and, from three waves on, than the waves added 3 .. 0."""
    for v in _order_terms(M):
        want = nn_ref.device_sum(v)
        assert want != float(v.sum())
        assert want != float(np.cumsum(v)[-1])
        assert want != nn_ref.device_sum(v, butterfly=nn_ref.BUTTERFLY[::-1])
        if M > 128:
            assert want != nn_ref.device_sum(v, waves=nn_ref.WAVES[::-1])


def test_restatement_lowest_index_and_metrics():
    """The restatement itself: ties go to the lowest index; the metric block on a case worked by hand."""
    target = np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 3, 0]], np.float32)
    d2, idx = nn_ref.nearest(target, np.array([[0, 0, 0], [1, 0, 0], [0, 2.5, 0]], np.float32))
    assert d2.tolist() == [1.0, 0.0, 0.25] and idx.tolist() == [0, 0, 3]
    assert nn_ref.stats(np.array([0.0, 0.25, 0.25, 1.0, np.inf], np.float32), 0.5, 0.5, False) == (1, 1, 0.0, 5)
    assert nn_ref.stats(np.array([0.0, 0.25, 0.25, 1.0, np.inf], np.float32), 0.5, 0.5, True) == (5, 1, 2.0, 5)
    ref = np.array([[0, 0, 0], [1, 0, 0], [10, 0, 0]], np.float32)
    est = np.array([[0, 0, 0.125], [1, 0.25, 0], [5, 0, 0]], np.float32)
    m = nn_ref.cloud_metrics(ref, est, threshold=0.2, truncation_acc=0.5, truncation_com=0.5)
    assert m["n_accuracy"] == 2 and m["n_completeness"] == 3
    assert m["accuracy_m"] == 0.1875 and m["precision"] == 0.5
    assert m["completeness_m"] == (0.125 + 0.25 + 0.5) / 3 and m["recall"] == 1 / 3
    assert m["chamfer_l1_m"] == 0.5 * (m["accuracy_m"] + m["completeness_m"])
    assert abs(m["fscore"] - 2 * 0.5 / 3 / (0.5 + 1 / 3)) < 1e-15
    far = nn_ref.cloud_metrics(ref, est + 100.0)
    assert np.isnan(far["accuracy_m"]) and np.isnan(far["precision"]) and far["n_accuracy"] == 0 and far["recall"] == 0.0
    assert nn_ref.crop_union_mask(ref, est, 1.2).tolist() == [True, True, False]


def test_restatement_agrees_with_kdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(8)
    target = rng.normal(0, 10, (5000, 3)).astype(np.float32)
    query = np.concatenate([rng.normal(0, 12, (3000, 3)), target[:50]]).astype(np.float32)
    d2, idx = nn_ref.nearest(target, query)
    dist, kidx = spatial.cKDTree(target.astype(np.float64)).query(query.astype(np.float64), k=1)
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)
    assert np.array_equal(idx, kidx)                # (continuous coordinates: no ties beyond the exact copies, which are unique rows)
    assert np.all(d2[-50:] == 0) and np.array_equal(idx[-50:], np.arange(50))


def test_nn_math_header_on_the_host(tmp_path):
    """include/sls_nn_math.h as plain C99: on lattice inputs its float32 distance equals the float64 one bit for bit (the
    claim the device tests rest on), the packed key orders like (distance, index), and the statistics' term is the
    restatement's."""
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "nn_math.c"
    src.write_text(r'''
#include <stdio.h>
#include "sls_nn_math.h"
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    float r[8];
    while (fread(r, 4, 8, in) == 8) {
        float d2 = sls_nn_dist2(r[0], r[1], r[2], r[3], r[4], r[5]), d = -1.0f;
        uint64_t key = sls_nn_key(d2, (uint32_t)r[6]);
        int kept = sls_nn_stats_term(d2, r[7], 0, &d), any = sls_nn_stats_term(d2, r[7], 1, &d);
        fwrite(&d2, 4, 1, out); fwrite(&key, 8, 1, out); fwrite(&d, 4, 1, out);
        fwrite(&kept, 4, 1, out); fwrite(&any, 4, 1, out);
    }
    fclose(out);
    return 0;
}
''')
    exe = tmp_path / "nn_math"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "include"), str(src),
                           "-o", str(exe), "-lm"])
    rng = np.random.default_rng(4)
    n = 20000
    rows = np.empty((n, 8), np.float32)
    rows[:, :6] = rng.integers(-1024, 1025, (n, 6)) / 16.0
    rows[: n // 2, 3:6] = rows[: n // 2, :3] + rng.integers(-8, 9, (n // 2, 3)) / 16.0      # near pairs: the truncation bites
    rows[:, 6] = rng.integers(0, 1 << 24, n)
    rows[:, 7] = rng.choice(np.array([0.25, 0.5, 0.4330127], np.float32), n)
    rows.tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.dtype([("d2", "<f4"), ("key", "<u8"), ("d", "<f4"), ("kept", "<i4"), ("any", "<i4")]))
    assert len(got) == n
    q, t = rows[:, :3].astype(np.float64), rows[:, 3:6].astype(np.float64)
    d64 = ((t - q) ** 2).sum(1)
    assert np.array_equal(got["d2"].astype(np.float64), d64)                    # exact on the lattice
    assert np.array_equal(got["key"], (got["d2"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows[:, 6].astype(np.uint64))
    order = np.lexsort((rows[:, 6], got["d2"]))
    assert np.all(np.diff(got["key"][order].astype(object)) >= 0)               # the key orders like (distance, index)
    tau2 = rows[:, 7] * rows[:, 7]
    kept = got["d2"] < tau2
    assert np.array_equal(got["kept"] != 0, kept) and np.all(got["any"] == 1) and 0.05 < kept.mean() < 0.8
    assert np.array_equal(got["d"], np.where(kept, np.sqrt(got["d2"]), rows[:, 7]).astype(np.float32))
